// Gather convolution for gfx950 on v_mfma_f32_16x16x32_{bf16,f16}: the two ResNet layers whose input and output grids differ
// by a factor of two and that therefore fit none of the staged-halo kernels --
//   * ConvTranspose2d k in {4, 3, 2}, stride 2 (+ folded BN, bias, ReLU): pose_resnet's deconv_layers;
//   * Conv2d 1x1 stride 2 (+ folded BN, optional residual / ReLU): the `downsample` projections of layer2..layer4.
//
// Both are one kernel.  Work is indexed by a BASE position m = (n, my, mx) and a CLASS c; an output element of class c sits at
// (so * my + py_c, so * mx + px_c) and sums, over the class's taps t and all input channels, W_c,t[co][ci] * x[ci][si * my + dy_t][si * mx + dx_t].
//   transposed conv (si = 1, so = 2): class = output parity (oy & 1, ox & 1).  Output row oy = 2 iy - p + ky receives kernel rows
//     ky == (oy + p) mod 2 only, from iy = my + (py + p - ky) / 2: at most two rows and two columns, i.e. an ordinary convolution
//     over a window of <= 2 x 2 input pixels (k = 4: four 2 x 2 windows; k = 3: 1x1, 1x2, 2x1, 2x2; k = 2: four 1x1).  The base
//     grid is the input grid, H x W.
//   1x1 stride 2 (si = 2, so = 1): one class, one tap (0, 0); the base grid is the output grid.
// GEMM view per class: D[cout][base pixel] = sum_k Wt[cout][k] X[k][pixel], k = (tap, input plane, 8 channels), K = taps * Cin: every
// tap of an output element is accumulated in f32 and the sum is rounded ONCE (head.hip's route rounds a 16-bit tap map per tap).
//   * A operand = weights: pre-packed on the host in fragment order [class][16-row Cout tile][k-step][lane][8], so that a wave's
//     A fragment is one coalesced 1 KB read (L2-resident: every workgroup of the launch reads the same few hundred KB).
//   * B operand = activations: lane (pixel l & 15, k-group l >> 4) reads the 16-byte vector of 8 channels of plane 4 * kstep + (l >> 4)
//     at its pixel's tap position straight from the blocked [N][C/8][H][W][8] input -- there is no halo to stage, a tap window is
//     <= 2 x 2 -- or zero when the position lies outside the map or the plane beyond Cin (Cin = 16 * odd: half a k-step of padding).
//   * A workgroup is four waves.  Transposed conv: the four waves are the four parity classes of ONE 16-pixel input tile, so the
//     tile's input vectors come from HBM once and from the CU's cache for the other three classes, and the four classes of a tile
//     are written by the workgroup that read it.  1x1 stride 2: the four waves take four consecutive pixel tiles.
//   * An accumulator lane holds 4 consecutive Cout of one pixel: 8 contiguous bytes of the blocked output.
// Every index is bounds-checked against the tensor it addresses; offsets are 64-bit.
#include "common.h"
#include "conv_device.h"

namespace scpose {

template <int DT, int MR>
__global__ __launch_bounds__(256) void conv_gather_kernel(const GatherLaunch p) {
  typedef typename DtOf<DT>::type T;
  typedef typename FragOf<T>::type Frag;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cls = p.nclass == 4 ? wv : 0;
  const long long tile = p.nclass == 4 ? (long long)blockIdx.x : (long long)blockIdx.x * 4 + wv;
  const long long total = (long long)p.N * p.Hb * p.Wb;
  if (tile * 16 >= total) return;   // (whole wave; no barrier in this kernel)
  const GatherClass gc = p.cls[cls];
  const int px = lane & 15, q = lane >> 4;
  const long long m = tile * 16 + px;
  const bool live = m < total;
  const long long mm = live ? m : 0;
  const int mx = (int)(mm % p.Wb), my = (int)((mm / p.Wb) % p.Hb), n = (int)(mm / ((long long)p.Wb * p.Hb));
  const int planes = p.cin / 8, pgroups = (planes + 3) / 4;
  const int tile0 = blockIdx.y * MR;   // first 16-row Cout tile of this workgroup
  const uint4* const wbase = reinterpret_cast<const uint4*>(p.w) + gc.w_off;   // fragment units of 16 bytes
  const int ksteps = gc.ntaps * pgroups;

  f32x4 acc[MR];
#pragma unroll
  for (int r = 0; r < MR; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};

  int ks = 0;
  for (int t = 0; t < gc.ntaps; ++t) {
    const int iy = p.si * my + gc.dy[t], ix = p.si * mx + gc.dx[t];
    const bool inb = live && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    for (int pg = 0; pg < pgroups; ++pg, ++ks) {
      const int plane = pg * 4 + q;
      uint4 bv = make_uint4(0u, 0u, 0u, 0u);
      if (inb && plane < planes)
        bv = reinterpret_cast<const uint4*>(p.in)[(((size_t)n * planes + plane) * p.H + iy) * p.W + ix];
      const Frag b = __builtin_bit_cast(Frag, bv);
#pragma unroll
      for (int r = 0; r < MR; ++r) {
        const uint4 av = wbase[((size_t)(tile0 + r) * ksteps + ks) * 64 + lane];
        acc[r] = mfma16<T>(__builtin_bit_cast(Frag, av), b, acc[r]);
      }
    }
  }

  if (!live) return;
  const int oy = p.so * my + gc.py, ox = p.so * mx + gc.px;
  if (oy >= p.Ho || ox >= p.Wo) return;
  const int cplanes = p.cout / 8;
#pragma unroll
  for (int r = 0; r < MR; ++r) {
    const int co = (tile0 + r) * 16 + 4 * q;   // this lane's 4 consecutive output channels
    if (co >= p.cout) continue;
    const size_t o = ((((size_t)n * cplanes + (co >> 3)) * p.Ho + oy) * p.Wo + ox) * 8 + (co & 4);   // 16-bit elements
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = acc[r][j] + p.bias[co + j];
    if (p.res) {
      const uint2 rv = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p.res) + o);
      v[0] += from_bits<T>((uint16_t)(rv.x & 0xffffu)); v[1] += from_bits<T>((uint16_t)(rv.x >> 16));
      v[2] += from_bits<T>((uint16_t)(rv.y & 0xffffu)); v[3] += from_bits<T>((uint16_t)(rv.y >> 16));
    }
    if (p.relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
    }
    uint2 ov;
    ov.x = pack2<T>(v[0], v[1]);
    ov.y = pack2<T>(v[2], v[3]);
    *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.out) + o) = ov;
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// kernel rows / columns that reach output parity `par` of ConvTranspose2d(k, stride 2, padding p), with the input offset of each
static int deconv_axis_taps(int k, int pad, int par, int kidx[2], int off[2]) {
  int n = 0;
  for (int kk = 0; kk < k; ++kk)
    if (((par + pad - kk) & 1) == 0) { kidx[n] = kk; off[n] = (par + pad - kk) / 2; ++n; }   // (exact: the numerator is even)
  return n;
}

// w: folded f32 weights as Conv2d stores them, [cout][cin][kk] with kk = ks * ks; taps: for each class the kernel positions summed
static int32_t gather_upload(const float* w, const float* bias, int cout, int cin, int kk, int dtype, GatherPacked* gp,
                             const int (*tapk)[4]) {
  const int planes = cin / 8, pgroups = (planes + 3) / 4, tiles = cout / 16;
  size_t frags = 0;
  for (int c = 0; c < gp->nclass; ++c) { gp->cls[c].w_off = (long long)frags; frags += (size_t)tiles * gp->cls[c].ntaps * pgroups * 64; }
  std::vector<uint16_t> host(frags * 8, 0);
  for (int c = 0; c < gp->nclass; ++c)
    for (int tl = 0; tl < tiles; ++tl)
      for (int t = 0; t < gp->cls[c].ntaps; ++t)
        for (int pg = 0; pg < pgroups; ++pg)
          for (int lane = 0; lane < 64; ++lane) {
            const int co = tl * 16 + (lane & 15), plane = pg * 4 + (lane >> 4);   // A operand: row = lane & 15, k-group = lane >> 4
            if (plane >= planes) continue;
            uint16_t* d = host.data() + ((size_t)gp->cls[c].w_off + ((size_t)tl * gp->cls[c].ntaps * pgroups + (size_t)t * pgroups + pg) * 64 + lane) * 8;
            for (int j = 0; j < 8; ++j) d[j] = host_f32_to_16(w[((size_t)co * cin + plane * 8 + j) * kk + tapk[c][t]], dtype);
          }
  gp->cin = cin; gp->cout = cout; gp->dtype = dtype;
  SCP_CHECK_HIP(hipMalloc(&gp->d_w, host.size() * 2));
  SCP_CHECK_HIP(hipMalloc(&gp->d_bias, (size_t)cout * sizeof(float)));
  SCP_CHECK_HIP(hipMemcpy(gp->d_w, host.data(), host.size() * 2, hipMemcpyHostToDevice));
  SCP_CHECK_HIP(hipMemcpy(gp->d_bias, bias, (size_t)cout * sizeof(float), hipMemcpyHostToDevice));
  return SCPOSE_OK;
}

static int32_t gather_check(const char* who, int cout, int cin, int dtype) {
  SCP_REQUIRE(cin > 0 && cin % 16 == 0, "%s: Cin=%d must be a multiple of 16", who, cin);
  SCP_REQUIRE(cout > 0 && cout % 16 == 0, "%s: Cout=%d must be a multiple of 16", who, cout);
  SCP_REQUIRE(dtype == SCPOSE_DT_BF16 || dtype == SCPOSE_DT_F16, "%s: dtype %d", who, dtype);
  return SCPOSE_OK;
}

int32_t deconv_upload(const float* w, const float* bias, int cout, int cin, int k, int dtype, GatherPacked* gp) {
  SCP_REQUIRE(k == 4 || k == 3 || k == 2, "deconv: kernel size %d unsupported (4, 3 or 2)", k);
  { const int32_t rc = gather_check("deconv", cout, cin, dtype); if (rc != SCPOSE_OK) return rc; }
  const int pad = k == 2 ? 0 : 1;   // (output_padding 1 for k = 3, else 0: the output is 2H x 2W for all three)
  gp->nclass = 4; gp->si = 1; gp->so = 2; gp->ks = k;
  int tapk[4][4];
  for (int c = 0; c < 4; ++c) {
    const int py = c >> 1, px = c & 1;
    int ky[2], oy[2], kx[2], ox[2];
    const int ny = deconv_axis_taps(k, pad, py, ky, oy), nx = deconv_axis_taps(k, pad, px, kx, ox);
    GatherClass& g = gp->cls[c];
    g.py = py; g.px = px; g.ntaps = ny * nx;
    for (int a = 0; a < ny; ++a)
      for (int b = 0; b < nx; ++b) { g.dy[a * nx + b] = oy[a]; g.dx[a * nx + b] = ox[b]; tapk[c][a * nx + b] = ky[a] * k + kx[b]; }
  }
  return gather_upload(w, bias, cout, cin, k * k, dtype, gp, tapk);
}

int32_t conv1x1s2_upload(const float* w, const float* bias, int cout, int cin, int dtype, GatherPacked* gp) {
  { const int32_t rc = gather_check("conv 1x1 s2", cout, cin, dtype); if (rc != SCPOSE_OK) return rc; }
  gp->nclass = 1; gp->si = 2; gp->so = 1;
  gp->cls[0] = GatherClass{};
  gp->cls[0].ntaps = 1;
  const int tapk[1][4] = {{0, 0, 0, 0}};
  return gather_upload(w, bias, cout, cin, 1, dtype, gp, tapk);
}

void gather_free(GatherPacked* gp) {
  if (gp->d_w) (void)hipFree(gp->d_w);
  if (gp->d_bias) (void)hipFree(gp->d_bias);
  gp->d_w = nullptr; gp->d_bias = nullptr;
}

void gather_out_size(const GatherPacked& gp, int H, int W, int* Ho, int* Wo) {
  if (gp.so == 2) { *Ho = 2 * H; *Wo = 2 * W; }
  else { *Ho = (H - 1) / 2 + 1; *Wo = (W - 1) / 2 + 1; }
}

int32_t gather_launch(const GatherPacked& gp, const void* in, int N, int H, int W, const void* res, int relu, void* out,
                      hipStream_t stream) {
  SCP_REQUIRE(gp.d_w && in && out, "conv gather: null argument");
  SCP_REQUIRE(N > 0 && H > 0 && W > 0, "conv gather: bad shape N=%d H=%d W=%d", N, H, W);
  GatherLaunch L{};
  L.in = in; L.w = gp.d_w; L.bias = gp.d_bias; L.res = res; L.out = out;
  L.N = N; L.H = H; L.W = W;
  gather_out_size(gp, H, W, &L.Ho, &L.Wo);
  L.Hb = gp.so == 2 ? H : L.Ho; L.Wb = gp.so == 2 ? W : L.Wo;
  L.cin = gp.cin; L.cout = gp.cout; L.nclass = gp.nclass; L.si = gp.si; L.so = gp.so; L.relu = relu;
  for (int c = 0; c < gp.nclass; ++c) L.cls[c] = gp.cls[c];
  const long long tiles = ((long long)N * L.Hb * L.Wb + 15) / 16;
  const long long gx = gp.nclass == 4 ? tiles : (tiles + 3) / 4;
  SCP_REQUIRE(gx < (1ll << 31), "conv gather: %lld pixel tiles exceed the grid", gx);
  const bool mr4 = gp.cout % 64 == 0;
  const dim3 grid((unsigned)gx, (unsigned)(gp.cout / (mr4 ? 64 : 16)));
  const bool bf = gp.dtype == SCPOSE_DT_BF16;
  if (mr4) { if (bf) conv_gather_kernel<0, 4><<<grid, 256, 0, stream>>>(L); else conv_gather_kernel<1, 4><<<grid, 256, 0, stream>>>(L); }
  else { if (bf) conv_gather_kernel<0, 1><<<grid, 256, 0, stream>>>(L); else conv_gather_kernel<1, 1><<<grid, 256, 0, stream>>>(L); }
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
