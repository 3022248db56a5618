// Host-only driver of the conv_m32 tile search (csrc/conv_m32.hip): no GPU, nothing is launched.  The kernel dispatch
// functions and the few device helpers the search calls are stubbed here; every call of conv_launch_m32 prints the chosen
// tiling (the library's own SCPOSE_DBG=32 line, on stderr) and the launch fields that follow from it.  Use it to compare two
// revisions of the search: build this file against each csrc/ and diff the listings, which must be identical.
//   hipcc --offload-host-only -x hip -std=c++17 -I spacecraft-pose-estimation_amd/csrc tools_dev/m32_tilings.cpp -o /tmp/m32_tilings
//   /tmp/m32_tilings > listing.txt 2>&1   (SCPOSE_DEV=1 SCPOSE_M32_OCC=3 /tmp/m32_tilings ... for the search's development switches)
// Shapes: every 3x3 layer of HRNet-W48 at 384x384 (batch 256, 16, 1) and of HRNet-W32 at 256x256 (batch 64, 16), sized for the
// whole chip (256 CUs) and for a share of it (128).  Layers conv_m32_choose() rejects run on other kernels and print "not m32".
#include "conv_m32.hip"
#include <stdarg.h>

namespace scpose {
void set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); }
const char* dev_env(const char* name) {   // as util.cpp, except that SCPOSE_DBG=32 is always on
  if (!strcmp(name, "SCPOSE_DBG")) return "32";
  const char* e = getenv("SCPOSE_DEV");
  return e && atoi(e) != 0 ? getenv(name) : nullptr;
}
int conv_device_cus() { return 256; }
const void* conv_zero_page() { static const char z[256] = {0}; return z; }
unsigned long long* conv_dbg_buffer(hipStream_t) { return nullptr; }
void conv_dbg_set_grid(int) {}
uint16_t host_f32_to_16(float, int) { return 0; }
static int32_t show(const char* k, int a, int b, int c, int d, const ConvLaunch& L, size_t lds) {
  printf("  -> %s(%d,%d,%d,%d) lds=%zu grid=%d items_per_wg=%d ps=%d cp=%d nchunks=%d ksteps=%d lds_w=%d lds_x=%d lds_bias=%d nbuf_w=%d wreg_chunks=%d store_stages=%d buf=%u/%u\n",
         k, a, b, c, d, lds, L.grid, L.items_per_wg, L.plane_stride, L.cp, L.nchunks, L.ksteps_full, L.lds_w, L.lds_x, L.lds_bias, L.nbuf_w, L.wreg_chunks,
         L.store_stages, L.in_bytes, L.out_bytes);
  return 0;
}
int32_t conv_m32_dispatch_bf16(int mr, int wm, int nr, int occ, const ConvLaunch& L, size_t lds, hipStream_t) { return show("m32", mr, wm, nr, occ, L, lds); }
int32_t conv_m32_dispatch_f16(int mr, int wm, int nr, int occ, const ConvLaunch& L, size_t lds, hipStream_t) { return show("m32", mr, wm, nr, occ, L, lds); }
int32_t conv_m32p_dispatch_bf16(int s, int mr, int nr, int c16, const ConvLaunch& L, size_t lds, hipStream_t) { return show("m32p", s, mr, nr, c16, L, lds); }
int32_t conv_m32p_dispatch_f16(int s, int mr, int nr, int c16, const ConvLaunch& L, size_t lds, hipStream_t) { return show("m32p", s, mr, nr, c16, L, lds); }
}  // namespace scpose

using namespace scpose;

struct Layer { PackedConv pc; bool m32; };
static Layer make_layer(int cin, int cout, int stride) {   // the variant-1 part of conv_upload (conv_igemm.hip)
  Layer l;
  PackedConv& pc = l.pc;
  pc.cin = cin; pc.cout = cout; pc.ks = 3; pc.stride = stride; pc.dtype = SCPOSE_DT_BF16;
  l.m32 = conv_m32_choose(cin, cout, 3, stride, &pc.mrep, &pc.wm, &pc.cp);
  if (!l.m32) return l;
  pc.variant = 1;
  pc.mt = pc.mrep == kMrep48 ? 48 : 32 * pc.mrep * pc.wm;
  pc.n_mblk = (cout + pc.mt - 1) / pc.mt;
  pc.wbytes = pack_conv_weights_m32(nullptr, cout, cin, 3, pc.mt, pc.cp, pc.dtype, nullptr, &pc.nchunks, &pc.ksteps_full);
  return l;
}

static void run(Layer& l, int N, int Ho, int share) {
  const PackedConv& pc = l.pc;
  if (!l.m32) { printf("%d->%d s%d %dx%d N=%d: not m32\n", pc.cin, pc.cout, pc.stride, Ho, Ho, N); return; }
  ConvLaunch L = {};
  L.N = N; L.Ho = L.Wo = Ho; L.H = L.W = Ho * pc.stride; L.cin_planes = pc.cin / 8; L.cout = pc.cout; L.cu_share = share;
  printf("share=%d s%d ", share, pc.stride);
  if (conv_launch_m32(pc, L, nullptr) != 0) printf("  -> error\n");
}

int main() {
  setvbuf(stdout, nullptr, _IONBF, 0);   // keep stdout in step with the library's stderr line
  struct Net { int c, size, nb, batch[3]; } nets[] = {{48, 384, 3, {256, 16, 1}}, {32, 256, 2, {64, 16, 0}}};
  for (const Net& net : nets) {
    const int h0 = net.size / 4;
    std::vector<Layer> layers; std::vector<int> ho;
    auto add = [&](int cin, int cout, int stride, int out) { layers.push_back(make_layer(cin, cout, stride)); ho.push_back(out); };
    add(64, 64, 1, h0);                                       // layer1 Bottleneck conv2
    add(256, net.c, 1, h0); add(256, 2 * net.c, 2, h0 / 2);   // transition1
    for (int i = 0; i < 4; ++i) {
      add(net.c << i, net.c << i, 1, h0 >> i);                // BasicBlocks of branch i
      if (i > 0 && i < 3) add(net.c << i, net.c << (i + 1), 2, h0 >> (i + 1));   // transition2, transition3
      for (int j = i + 1; j < 4; ++j) {                       // fuse down path i -> j: stride-2 steps at every size on the way
        for (int k = i + 1; k < j; ++k) add(net.c << i, net.c << i, 2, h0 >> k);
        add(net.c << i, net.c << j, 2, h0 >> j);
      }
    }
    for (int b = 0; b < net.nb; ++b)
      for (int share : {0, 128})
        for (size_t i = 0; i < layers.size(); ++i) {
          run(layers[i], net.batch[b], ho[i], share);
          run(layers[i], net.batch[b], ho[i], share);   // second launch of the same shape: the memo's answer
        }
  }
  return 0;
}
