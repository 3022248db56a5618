// Host side of the 32x32x16-MFMA convolution (conv_m32_kernel.h): eligibility, weight packing,
// tile search, launch.  See the kernel header for the design and the measurements behind it.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

namespace scpose {

int32_t conv_m32_dispatch_bf16(int mr, int wm, int nr, int occ, const ConvLaunch& L, size_t lds, hipStream_t st);
int32_t conv_m32_dispatch_f16(int mr, int wm, int nr, int occ, const ConvLaunch& L, size_t lds, hipStream_t st);
int32_t conv_m32p_dispatch_bf16(int stride, int mr, int nr, int c16, const ConvLaunch& L, size_t lds, hipStream_t st);
int32_t conv_m32p_dispatch_f16(int stride, int mr, int nr, int c16, const ConvLaunch& L, size_t lds, hipStream_t st);

// kernel variants built (keep in step with m32_dispatch / m32p_dispatch): occ = resident workgroups
// per CU of the single-role kernel (1, 2), or 3 = the producer/consumer kernel (512 threads, one per CU);
// nb16 > 0: the producer/consumer kernel with 16x16x32 consumers and nb16 columns of 16 pixels per consumer wave
// (conv_m32p_kernel.h, C16) -- the ONLY family of the layers conv_m16_eligible() names, whatever the batch, so that a
// frame's sums are formed in one order; nr then only sizes the tile (nb16 * 16 = nr * 32 pixels)
struct M32Variant { int mr, wm, nr, occ, nb16; };
static const M32Variant kVariants[] = {
  {3, 1, 3, 1, 0}, {3, 1, 2, 2, 0}, {3, 1, 1, 3, 0}, {3, 1, 2, 3, 0}, {3, 1, 3, 3, 0},
  {2, 1, 2, 1, 0}, {2, 1, 4, 1, 0}, {2, 1, 3, 2, 0}, {2, 1, 1, 3, 0}, {2, 1, 2, 3, 0}, {2, 1, 3, 3, 0},
  {3, 1, 1, 3, 2}, {3, 1, 2, 3, 4}, {3, 1, 3, 3, 5}, {3, 1, 3, 3, 6},
  {kMrep48, 1, 4, 3, 8},   // 48-row blocks, eight columns per consumer wave (512-pixel tile groups)
};

// 16x16x32 consumers: stride-1 3x3 layers with 96-row Cout blocks whose input is a whole number of 32-channel pairs of plane
// pairs (the consumers process 2-plane groups in pairs) and has at least the three 2-plane chunks the producer/consumer
// schedule needs: 96 -> 96, 192 -> 192, 384 -> 384 of HRNet-W48.  SCPOSE_M16=0 (development) keeps them on 32x32x16.
static bool conv_m16_eligible(const PackedConv& pc) {
  static const char* e = dev_env("SCPOSE_M16");
  if (pc.mrep == kMrep48) return true;   // (conv_m32_choose checked the layer; this family has no 32x32x16 form)
  return pc.ks == 3 && pc.stride == 1 && pc.mrep == 3 && pc.wm == 1 && pc.cp == 2 && (pc.cin / 16) % 2 == 0 && pc.cin / 16 >= 3 && !(e && atoi(e) == 0);
}

bool conv_m32_choose(int cin, int cout, int ks, int stride, int* mr, int* wm, int* cp) {
  static const char* e = dev_env("SCPOSE_M32");
  if (e && atoi(e) == 0) return false;
  static const char* e2 = dev_env("SCPOSE_M32_S2");
  if (ks != 3 || cin % 16 != 0) return false;
  // stride 2 (fuse down paths, transition): producer/consumer kernel only, which needs >= 3 K-chunks;
  // measured 1.4-1.7x faster than the 16x16x32 kernel on these input-heavy layers (SCPOSE_M32_S2=0 disables)
  if (stride != 1 && !(stride == 2 && (cout % 96 == 0 || cout % 64 == 0 || cout == 48) && cin / 16 >= 3 && !(e2 && atoi(e2) == 0))) return false;
  int m = 0, w = 1;
  if (cout % 96 == 0) m = 3;          // Cout blocks of 96 (HRNet-W48: 96, 192, 384)
  else if (cout % 64 == 0) m = 2;     // Cout blocks of 64 (HRNet-W32: 64, 128, 256; layer1)
  else if (cout == 48 && (stride == 2 || cin >= 96)) {
    // stride 2 (input-bound): one 64-row block with 16 rows of padding.  Stride 1 with a deep K (transition1, 256 -> 48: MFMA-bound):
    // a 48-row block on the 16x16x32 consumers' 3 x 8 form when K is a whole number of 32-channel pairs of plane pairs -- the 64-row
    // form spent a quarter of its MFMAs on the padding rows (SCPOSE_M48=0, development: the 64-row form)
    static const char* e48 = dev_env("SCPOSE_M48");
    m = (stride == 1 && (cin / 16) % 2 == 0 && cin / 16 >= 4 && !(e48 && atoi(e48) == 0)) ? kMrep48 : 2;
  }
  else return false;
  *mr = m; *wm = w;
  const int planes = cin / 8;
  // whole K in one chunk with resident weights when it fits comfortably, else stream 2-plane chunks
  const int mt = m == kMrep48 ? 48 : 32 * m * w;
  const size_t whole = (size_t)(planes / 2) * 9 * 2 * mt * 16;
  // (stride 2 runs on the producer/consumer kernel only, which needs >= 3 K-chunks: always stream 2-plane chunks there --
  // a single resident chunk, e.g. 48 -> 64, would pass create and then find no tiling at the first forward)
  *cp = (m != kMrep48 && stride == 1 && cout == mt && whole <= 60 * 1024 && planes <= 6) ? planes : 2;
  return true;
}

size_t pack_conv_weights_m32(const float* w, int cout, int cin, int ks, int mt, int cp, int dtype,
                             uint16_t* dst, int* nchunks_out, int* ksteps_full_out) {
  const int planes = cin / 8, kk = ks * ks;
  const int nchunks = (planes + cp - 1) / cp;
  const int ksteps_full = (cp / 2) * kk;
  const int n_mblk = (cout + mt - 1) / mt;
  const size_t chunk_elems = (size_t)ksteps_full * 2 * mt * 8;
  const size_t total = (size_t)n_mblk * nchunks * chunk_elems;
  if (nchunks_out) *nchunks_out = nchunks;
  if (ksteps_full_out) *ksteps_full_out = ksteps_full;
  if (!dst) return total * 2;
  memset(dst, 0, total * 2);
  for (int mb = 0; mb < n_mblk; ++mb)
    for (int c = 0; c < nchunks; ++c) {
      const int plane0 = c * cp;
      const int pl = (planes - plane0) < cp ? (planes - plane0) : cp;
      uint16_t* base = dst + ((size_t)mb * nchunks + c) * chunk_elems;
      for (int pp = 0; pp < pl / 2; ++pp)
        for (int tap = 0; tap < kk; ++tap)
          for (int kg = 0; kg < 2; ++kg) {
            const int st = pp * kk + tap;
            const int plane = plane0 + 2 * pp + kg;
            for (int r = 0; r < mt; ++r) {
              const int co = mb * mt + r;   // natural channel order
              if (co >= cout) continue;
              uint16_t* d = base + ((size_t)(st * 2 + kg) * mt + r) * 8;
              for (int j = 0; j < 8; ++j)
                d[j] = host_f32_to_16(w[((size_t)co * cin + plane * 8 + j) * kk + tap], dtype);
            }
          }
    }
  return total * 2;
}

// producer/consumer kernel, K-chunks of `cp` planes (a launch-time choice: the packed image of a 2*cp-plane chunk is the
// images of its two cp-plane chunks back to back, and K is accumulated in the same order whatever the chunking):
// weights stay resident (all chunks in LDS) when the layer has one Cout block and they fit
struct M32pChunking { int cp, nchunks, ksteps_full; };
static M32pChunking m32p_chunking(const PackedConv& pc, int cp) { return {cp, (pc.cin / 8) / cp, (cp / 2) * pc.ks * pc.ks}; }
// LDS bytes of one weight-chunk buffer / of the bias vector (the kernels' layout: [bias][W ...][X x2][retire buffer])
static size_t m32_lds_w(const PackedConv& pc, int ksteps_full) { return (size_t)ksteps_full * 2 * pc.mt * 16; }
static size_t m32_lds_bias(const PackedConv& pc) { return (((size_t)pc.n_mblk * pc.mt * 4) + 511) & ~(size_t)511; }
// (pxcap = pixel slots of a tile group = rows of the retire buffer: 4 waves x nr x 32, or 4 x nb16 x 16)
static int m32_pxcap(int wn, int nr, int nb16) { return nb16 > 0 ? wn * nb16 * 16 : wn * nr * 32; }
static int m32p_wbufs(const PackedConv& pc, const M32pChunking& ck, int plane_stride, int pxcap) {
  const size_t rest = m32_lds_bias(pc) + 2 * (size_t)ck.cp * plane_stride + (size_t)(pc.mt / 8) * pxcap * 16;
  return (pc.n_mblk == 1 && ck.nchunks > 2 && rest + ck.nchunks * m32_lds_w(pc, ck.ksteps_full) <= 160 * 1024) ? ck.nchunks : 2;
}
static size_t m32p_lds_bytes(const PackedConv& pc, const M32pChunking& ck, int plane_stride, int pxcap) {
  return m32_lds_bias(pc) + m32p_wbufs(pc, ck, plane_stride, pxcap) * m32_lds_w(pc, ck.ksteps_full) + 2 * (size_t)ck.cp * plane_stride + (size_t)(pc.mt / 8) * pxcap * 16;
}
static size_t m32_lds_bytes(const PackedConv& pc, int plane_stride) {   // single-role kernel: one weight buffer when the whole K is resident
  return 1024 + m32_lds_bias(pc) + ((pc.nchunks == 1 && pc.n_mblk == 1) ? 1 : 2) * m32_lds_w(pc, pc.ksteps_full) + 2 * (size_t)pc.cp * plane_stride;
}

// development switches that restrict the tile search (tools_dev/README.md), read once; `any` bypasses the layer's memo.
// occ / nr / nb16: one kernel family / column count / column count of the 16x16x32 consumers; cpmul: cap of the K-chunk depth
// multiplier; cus: size small layers for a share of the chip; th, tw: one producer/consumer tile (nr / nb16: any value given restricts)
struct M32SearchSwitches { int occ = 0, nr = 0, nb16 = 0, cpmul = 4, cus = 0, th = 0, tw = 0; bool has_nr = false, has_nb16 = false, any = false; };
static M32SearchSwitches m32_read_switches() {
  M32SearchSwitches s;
  auto rd = [&s](const char* name, int* v) { const char* e = dev_env(name); if (e) { *v = atoi(e); s.any = true; } return e != nullptr; };
  rd("SCPOSE_M32_OCC", &s.occ); s.has_nr = rd("SCPOSE_M32_NR", &s.nr); s.has_nb16 = rd("SCPOSE_M16_NB", &s.nb16); rd("SCPOSE_M32_CPMUL", &s.cpmul); rd("SCPOSE_M32_CUS", &s.cus);
  if (const char* e = dev_env("SCPOSE_M32_TILE")) { sscanf(e, "%d,%d", &s.th, &s.tw); s.any = true; }
  return s;
}

// single-role kernel: maximise useful MFMA columns, prefer two workgroups per CU (one computes while the other is stalled in its
// memory instructions), then pixels per weight chunk
static double m32_single_score(const M32Variant& v, double eff, int wn, int hh, int hw, int th, int tw) {
  // measured preference: producer/consumer for 96-row blocks, two workgroups per CU for 64-row blocks
  const double pref = v.occ == 3 ? (v.mr == 3 ? 1.5 : 1.1) : v.occ == 2 ? 1.25 : 1.0;
  return eff * pref / (1.0 + 2.0 / (wn * v.nr)) - 0.02 * (double)(hh * hw) / (th * tw);
}

// producer/consumer kernel: a cycle model fitted to the phase stamps: stage = max(consumer MFMAs, producer bytes
// at ~13 B/clk) + barrier, but never shorter than the round trip of the stage's LDS-DMA (small tiles: the stage count, not the
// MFMAs, sets the time -> deeper K-chunks); items are quantised per CU
static double m32p_cycles(const PackedConv& pc, const M32Variant& v, const M32pChunking& ck, int cap, int ps, int npix, int tw, long items, int cus) {
  const double per_cu = (double)((items + cus - 1) / cus);
  const double mr_eff = v.mr == kMrep48 ? 1.5 : (double)v.mr;   // 32-row units of the Cout block
  const double mfma = mr_eff * (cap / 128.0) * (ck.cp / 2) * pc.ks * pc.ks * 32.0 * 1.35;
  const bool res_w = m32p_wbufs(pc, ck, ps, cap) > 2;
  const double bytes = (res_w ? 0.0 : (double)m32_lds_w(pc, ck.ksteps_full)) + (double)ck.cp * ps + 2.0 * pc.mt * npix * 2 / ck.nchunks;
  double stage = (mfma > bytes / 13.0 ? mfma : bytes / 13.0) + 700.0;
  if (stage < 2600.0) stage = 2600.0;
  // 16x16x32 consumers read B fragments as 16 consecutive pixel slots: with a tile width that is a multiple of 16 a column
  // never straddles two halo rows and its ds_read_b128 lane groups meet no bank twice (96 -> 96 @48 x 48: 8 x 48 instead of
  // 16 x 24 tiles, -1.2 % measured, profiles/round4_m16_tile_choices.txt) -- a tie-break, not a term of the model
  return per_cu * (ck.nchunks * stage + mr_eff * (cap / 128.0) * 16 * 25.0) * ((v.nb16 > 0 && tw % 16 != 0) ? 1.02 : 1.0);
}

// (1) the search over kVariants: the best single-role tiling s (highest score; items_s = its work items) and the best
// producer/consumer one p (fewest cycles); occ == 0: none found
struct M32SearchResult { M32Tiling s, p; long items_s = 0; };
static M32SearchResult m32_search(const PackedConv& pc, const M32SearchSwitches& sw, int N, int Ho, int Wo, int cus) {
  const int wn = 4 / pc.wm, k2 = pc.ks / 2;
  const bool m16 = conv_m16_eligible(pc);
  const int tw_cand[8] = {Wo, 64, 48, 32, 24, 16, 12, 8};
  M32SearchResult r;
  double best_s = -1e30, best_p = 1e30;
  for (const M32Variant& v : kVariants) {
    if (v.mr != pc.mrep || v.wm != pc.wm || (sw.occ && v.occ != sw.occ) || (sw.has_nr && v.nr != sw.nr)) continue;
    if (m16 != (v.nb16 > 0)) continue;   // the layer's kernel family does not depend on the batch (see kVariants)
    if (sw.has_nb16 && v.nb16 > 0 && v.nb16 != sw.nb16) continue;
    const int cap = m32_pxcap(wn, v.nr, v.nb16);
    if (v.occ == 3 && (pc.nchunks < 3 || (pc.cin / 8) % pc.cp != 0)) continue;   // retire-buffer schedule needs >= 3 equal chunks
    if (pc.stride == 2 && v.occ != 3) continue;
    const int halo_cap = v.occ == 2 ? 512 : 1024;
    const size_t lds_cap = v.occ == 2 ? 80 * 1024 : 160 * 1024;
    for (int ti = 0; ti < 8; ++ti) {
      const int tw = tw_cand[ti];
      if (tw > Wo || tw > cap || (ti > 0 && tw >= Wo)) continue;
      if (sw.tw > 0 && v.occ == 3 && tw != sw.tw) continue;
      for (int th = 1; th <= Ho && th * tw <= cap; ++th) {
        if (sw.th > 0 && v.occ == 3 && th != sw.th) continue;
        const int hh = (th - 1) * pc.stride + 1 + 2 * k2, hw = (tw - 1) * pc.stride + 1 + 2 * k2;
        for (int nseg = 1; nseg <= 8; ++nseg) {
          if (nseg * th * tw > cap || nseg * hh * hw > halo_cap) break;
          const int ps = (nseg * hh * hw * 16 + 255) & ~255;
          if (v.occ != 3 && m32_lds_bytes(pc, ps) > lds_cap) break;
          const int tx = (Wo + tw - 1) / tw, ty = (Ho + th - 1) / th;
          const long items = (((long)N * tx * ty + nseg - 1) / nseg) * pc.n_mblk;
          if (v.occ == 3) {
            bool any = false;
            for (int mul = 1; mul <= sw.cpmul; mul *= 2) {
              const int cp = pc.cp * mul;
              if ((mul > 1 && pc.cp != 2) || (pc.cin / 8) % cp != 0) continue;
              const M32pChunking ck = m32p_chunking(pc, cp);
              if (ck.nchunks < 3 || m32p_lds_bytes(pc, ck, ps, cap) > lds_cap) continue;
              any = true;
              const double cost = m32p_cycles(pc, v, ck, cap, ps, nseg * th * tw, tw, items, cus);
              if (cost < best_p) { best_p = cost; r.p = {th, tw, nseg, v.nr, ps, 3, cp, v.nb16}; }
            }
            if (!any) break;
            continue;
          }
          const double eff = (double)Ho * Wo / ((double)tx * ty / nseg * cap);
          const double score = m32_single_score(v, eff, wn, hh, hw, th, tw);
          if (score > best_s) { best_s = score; r.s = {th, tw, nseg, v.nr, ps, v.occ, pc.cp, 0}; r.items_s = items; }
        }
      }
    }
  }
  return r;
}

// (2) measured preference: producer/consumer for 96-row blocks and for stride 2, two workgroups per CU for 64-row blocks --
// unless those would leave the chip under-filled (at most one round of items: small batches, deep branches), where the
// layer is a chain of DMA round trips and the small-tile producer/consumer candidates are 1.7-2x faster
// (W32 batch 64: 128->128 @16x16 30.8 -> 14.9 us, 256->256 @8x8 40.1 -> 23.0 us before deeper chunks)
static M32Tiling m32_choose_tiling(const PackedConv& pc, const M32SearchResult& r, int cus) {
  const bool take_p = r.p.occ != 0 && (r.s.occ == 0 || pc.mrep == 3 || pc.mrep == kMrep48 || pc.stride == 2 || pc.cout == 48 || r.items_s <= (long)cus * r.s.occ);
  return take_p ? r.p : r.s;
}

// (3) pick the tiling (remembered in the layer), fill the launch descriptor, dispatch
int32_t conv_launch_m32(const PackedConv& pc, ConvLaunch& L, hipStream_t stream) {
  static const M32SearchSwitches sw = m32_read_switches();
  const int wn = 4 / pc.wm, k2 = pc.ks / 2;
  const int cus_all = conv_device_cus();
  // a share of the chip only for layers that cannot fill it anyway (<= 64 k output pixels: chains of DMA round trips, whose
  // duration hardly depends on the CU count -- W32 256x256 batch 64 captured forward 3.39 -> 3.07 ms with half the chip each)
  const int share = sw.cus > 0 ? sw.cus : L.cu_share;
  const int cus = (share > 0 && share < cus_all && (long)L.N * L.Ho * L.Wo <= 65536) ? share : cus_all;
  // the search depends on (layer, N, Ho, Wo, CUs) only: its result is remembered in the layer (a forward launches the
  // same shapes every time; small batches are launch-bound on the host)
  PackedConv::TileMemo& memo = pc.m32_memo[cus != cus_all];
  if (sw.any || memo.n != L.N || memo.ho != L.Ho || memo.wo != L.Wo || memo.cus != cus) {
    const M32Tiling chosen = m32_choose_tiling(pc, m32_search(pc, sw, L.N, L.Ho, L.Wo, cus), cus);
    SCP_REQUIRE(chosen.occ != 0, "conv m32: no tiling for %dx%d output", L.Ho, L.Wo);
    memo = {L.N, L.Ho, L.Wo, cus, chosen};
  }
  const M32Tiling& t = memo.t;
  const bool pcons = t.occ == 3;   // producer/consumer kernel
  L.th = t.th; L.tw = t.tw; L.nt = t.nseg;
  L.tiles_x = (L.Wo + L.tw - 1) / L.tw;
  L.tiles_y = (L.Ho + L.th - 1) / L.th;
  L.halo_h = (L.th - 1) * pc.stride + 1 + 2 * k2;
  L.halo_w = (L.tw - 1) * pc.stride + 1 + 2 * k2;
  L.plane_stride = t.ps;
  const M32pChunking ck = pcons ? m32p_chunking(pc, t.cp) : M32pChunking{pc.cp, pc.nchunks, pc.ksteps_full};
  L.cp = ck.cp; L.nchunks = ck.nchunks; L.ksteps_full = ck.ksteps_full; L.n_mblk = pc.n_mblk;
  L.lds_w = (int32_t)m32_lds_w(pc, ck.ksteps_full);
  L.lds_x = ck.cp * L.plane_stride;
  L.lds_bias = (int32_t)m32_lds_bias(pc);
  const int pxcap = m32_pxcap(wn, t.nr, t.nb16);
  L.nbuf_w = pcons ? m32p_wbufs(pc, ck, L.plane_stride, pxcap) : (pc.nchunks == 1 && pc.n_mblk == 1) ? 1 : 2;
  L.nbuf_x = 2;
  L.wreg_chunks = 1;
  const size_t lds = pcons ? m32p_lds_bytes(pc, ck, L.plane_stride, pxcap) : m32_lds_bytes(pc, L.plane_stride);
  if (!pcons) {   // the single-role kernel's residual loads
    L.zero16 = conv_zero_page();
    SCP_REQUIRE(L.zero16, "conv: cannot allocate the zero page");
  }
  L.tiles_total = L.N * L.tiles_x * L.tiles_y;
  { static const char* e = dev_env("SCPOSE_NST"); const int v = e ? atoi(e) : 0;   // producer/consumer kernel: stages that store the previous tile
    L.store_stages = (pcons && v > 0 && v <= pc.nchunks - 2) ? v : 0; }
  L.items_total = ((L.tiles_total + L.nt - 1) / L.nt) * pc.n_mblk;
  { static const char* e = dev_env("SCPOSE_DBG"); L.dbg = e ? atoi(e) : 0; }
  if (!kDevBuild) L.dbg &= 32;   // shipped library: only the host-side "print the tile choice" bit means anything (common.h: SCP_DBG)
  L.in_bytes = (uint32_t)blocked_bytes(L.N, L.cin_planes, L.H, L.W);   // both fit: conv_launch splits the batch
  L.out_bytes = (uint32_t)blocked_bytes(L.N, (pc.cout + 7) / 8, L.Ho, L.Wo);
  L.dbg_buf = nullptr;
  if (L.dbg & 8) L.dbg_buf = conv_dbg_buffer(stream);
  if (L.dbg & 32)
    fprintf(stderr, "m32 %d->%d %dx%d N=%d: mr=%d nr=%d nb16=%d occ=%d cp=%d tile %dx%d nseg=%d halo %dx%d lds=%zu items=%d\n", pc.cin, pc.cout, L.Ho, L.Wo, L.N,
            pc.mrep, t.nr, t.nb16, t.occ, L.cp, L.th, L.tw, L.nt, L.halo_h, L.halo_w, lds, L.items_total);
  L.fd_npix = make_fastdiv(L.th * L.tw); L.fd_tw = make_fastdiv(L.tw);
  L.fd_hp = make_fastdiv(L.halo_h * L.halo_w); L.fd_halo_w = make_fastdiv(L.halo_w);
  L.fd_tiles_img = make_fastdiv(L.tiles_x * L.tiles_y); L.fd_tiles_x = make_fastdiv(L.tiles_x);
  L.fd_nmblk = make_fastdiv(pc.n_mblk);
  int grid = cus * (t.occ == 2 ? 2 : 1);
  if (grid > L.items_total) grid = L.items_total;
  L.items_per_wg = (L.items_total + grid - 1) / grid;
  L.grid = (L.items_total + L.items_per_wg - 1) / L.items_per_wg;
  conv_dbg_set_grid(L.grid);
  if (pcons) {
    static const char* wr_env = dev_env("SCPOSE_M32_WREG");
    L.wreg_chunks = (pc.n_mblk == 1 && ck.nchunks == 6 && ck.cp == 2 && pc.stride == 1 && pc.mrep == 3 && (t.nb16 > 0 ? t.nb16 == 6 : t.nr == 3) && !(wr_env && atoi(wr_env) == 0)) ? 6 : 1;
    // t.nb16 > 0: 16x16x32 consumers (conv_m32p_kernel.h, C16; round 4) -- see conv_m16_eligible
    if (pc.dtype == SCPOSE_DT_BF16) return conv_m32p_dispatch_bf16(pc.stride, pc.mrep, t.nr, t.nb16, L, lds, stream);
    return conv_m32p_dispatch_f16(pc.stride, pc.mrep, t.nr, t.nb16, L, lds, stream);
  }
  if (pc.dtype == SCPOSE_DT_BF16) return conv_m32_dispatch_bf16(pc.mrep, pc.wm, t.nr, t.occ, L, lds, stream);
  return conv_m32_dispatch_f16(pc.mrep, pc.wm, t.nr, t.occ, L, lds, stream);
}

}  // namespace scpose
