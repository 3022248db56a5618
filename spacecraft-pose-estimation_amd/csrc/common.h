// Internal declarations shared by the gfx950 kernels and the host-side plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdarg.h>
#include <stdio.h>
#include <string>
#include <vector>
#include <string.h>

#include "../../include/scpose.h"

namespace scpose {

// ---- error plumbing (thread-local message, int status; nothing throws across the ABI) ----
void set_error(const char* fmt, ...);
const char* dev_env(const char* name);   // getenv() for development switches; null unless SCPOSE_DEV=1 (util.cpp)
const char* last_error();

#define SCP_CHECK_HIP(expr)                                                         \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      ::scpose::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                          __FILE__, __LINE__);                                      \
      return SCPOSE_E_HIP;                                                          \
    }                                                                               \
  } while (0)

#define SCP_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      ::scpose::set_error(__VA_ARGS__);   \
      return SCPOSE_E_INVALID;            \
    }                                     \
  } while (0)

// Development instrumentation and ablation switches (phase stamps, "skip the MFMA loop" and the like) exist only in
// the DEVELOPMENT build of the library (make dev -> libscpose_hip_dev.so, -DSCPOSE_DEV_BUILD, loaded by tools_dev/ through
// SCPOSE_DEV=1).  In the shipped libscpose_hip.so these fold to constants at compile time: its kernels contain no
// switchable wrong-results path and never read the dbg fields of their launch descriptors.
#ifdef SCPOSE_DEV_BUILD
#define SCP_DBG(p, bits) ((p).dbg & (bits))
#define SCP_DBG_BUF(p) ((p).dbg_buf)
#define SCP_DEV_ONLY(x) (x)
constexpr bool kDevBuild = true;
#else
#define SCP_DBG(p, bits) (0)
#define SCP_DBG_BUF(p) (static_cast<unsigned long long*>(nullptr))
#define SCP_DEV_ONLY(x) (0)
constexpr bool kDevBuild = false;
#endif

// Kernels that use more than 64 KB of dynamic LDS must be opted in with hipFuncSetAttribute, which applies to the
// device that is current at the call.  One memo per kernel instantiation, indexed by device: the attribute is set the
// first time that instantiation is launched on each device (idempotent per-device memoisation like conv_zero_page();
// never a per-process flag, which would leave a second device of the same process without the opt-in).
struct LdsOptIn {
  bool done[16] = {false};
};
int32_t lds_opt_in(const void* kernel, int bytes, LdsOptIn* memo);

// Exact unsigned division by a launch-time constant (n < 2^31): q = (mulhi(n, mul) + n*add) >> shift.
struct FastDiv {
  uint32_t mul, shift, add, d;
};
inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f; f.d = d ? d : 1;
  uint32_t s = 0;
  while ((2u << s) <= f.d) ++s;                 // s = floor(log2 d)
  if ((f.d & (f.d - 1)) == 0) { f.mul = 0; f.add = 1; f.shift = s; }
  else { f.mul = (uint32_t)((((uint64_t)1 << (32 + s)) / f.d) + 1); f.add = 0; f.shift = s; }
  return f;
}

// Carves one caller-owned workspace into consecutive 256-byte aligned regions.  base == nullptr only adds the sizes up: a
// *_workspace_bytes entry point and its launch run the same carving function, so the two cannot disagree.
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Carve {
  uint8_t* base;
  size_t off = 0;
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off; }
};

// Little-endian loads from a byte position of any alignment (file formats: payloads start wherever the bytes before them end)
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
template <class T>
__device__ __forceinline__ T ld_as(const uint8_t* p) {
  T v;
  __builtin_memcpy(&v, p, sizeof(T));
  return v;
}
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return ld_as<uint32_t>(p); }
__device__ __forceinline__ int64_t ld64(const uint8_t* p) { return ld_as<int64_t>(p); }

// ---- 32-bit buffer descriptors ---------------------------------------------------------------
// The convolution kernels address their tensors through raw buffer descriptors (conv_pipe_kernel.h: make_buf): base + 32-bit
// offset, num_records = the tensor's bytes, which must stay below kBufLimit -- the offset given to padding lanes (BUF_OOB) has
// to lie past every tensor.  There is no second, 64-bit form of that traffic.  One rule covers larger batches: a launch whose
// largest buffer-addressed tensor would not fit runs as several launches over consecutive frame ranges, every pointer
// advanced by its frame size (for_frame_ranges: conv_launch, bottleneck, fuse_down, fused BasicBlock).  Inside a range every
// tensor fits, so the kernel a frame runs on never depends on the batch.
constexpr size_t kBufLimit = 0xfffffff0ull;
inline size_t blocked_bytes(int n, int planes, int h, int w) { return (size_t)n * planes * h * w * 16; }   // [N][C/8][H][W][8] x 16 bit
inline bool fits_buf(size_t bytes) { return bytes < kBufLimit; }
// frames per launch: the largest range whose largest tensor (frame_bytes per frame, itself fits_buf) fits; cap > 0 = a smaller
// range, with which tests force the split on a small batch
inline int buf_max_frames(size_t frame_bytes, int cap = 0) {
  const int max_n = (int)(kBufLimit / frame_bytes);
  return cap > 0 && cap < max_n ? cap : max_n;
}
// the two development switches of the split, read once (util.cpp): SCPOSE_MAXN caps the range, SCPOSE_DBG bit 32 prints each range
struct FrameRangeSwitches { int cap; bool print; };
const FrameRangeSwitches& frame_range_switches();
// launch(n0, n) for consecutive ranges of the N frames, until one fails.  frame_bytes: bytes per frame of the launch's largest
// buffer-addressed tensor; name_fmt, ...: printf form of the launch's name, formatted only for the error and the debug line
template <class Launch>
__attribute__((format(printf, 4, 5))) int32_t for_frame_ranges(int N, size_t frame_bytes, Launch&& launch, const char* name_fmt, ...) {
  const FrameRangeSwitches& sw = frame_range_switches();
  char name[96] = "";
  if (sw.print || !fits_buf(frame_bytes)) {
    va_list ap;
    va_start(ap, name_fmt);
    vsnprintf(name, sizeof(name), name_fmt, ap);
    va_end(ap);
  }
  SCP_REQUIRE(fits_buf(frame_bytes), "%s: one frame (%zu bytes) does not fit a 32-bit buffer descriptor", name, frame_bytes);
  const int max_n = buf_max_frames(frame_bytes, sw.cap);
  for (int n0 = 0; n0 < N; n0 += max_n) {
    const int n = N - n0 < max_n ? N - n0 : max_n;
    if (sw.print) fprintf(stderr, "%s N=%d: frames %d..%d\n", name, N, n0, n0 + n);
    const int32_t rc = launch(n0, n);
    if (rc != SCPOSE_OK) return rc;
  }
  return SCPOSE_OK;
}

// ---- 3x3 / 1x1 implicit-GEMM convolution ---------------------------------------------------
// Device-side description of one convolution launch.  All tensors are "blocked":
// [N][C/8][H][W][8] 16-bit elements.
struct ConvLaunch {
  const void* in;      // blocked input  N x Cin x H x W
  const void* wpk;     // packed weights (see pack_conv_weights)
  const float* bias;   // f32 [n_mblk*MT] (zero padded)
  const void* res;     // optional blocked residual, shape of out
  void* out;           // blocked output, or f32 NCHW when out_nchw_f32
  int32_t N, H, W, Ho, Wo;
  int32_t cin_planes;  // Cin/8
  int32_t cout;        // real Cout (for store masks)
  int32_t th, tw;      // output tile (th*tw <= 64*NREP)
  int32_t tiles_x, tiles_y;
  int32_t halo_w, halo_h;
  int32_t plane_stride;  // LDS bytes per staged input plane
  int32_t cp;            // planes per K-chunk (even)
  int32_t nchunks;
  int32_t ksteps_full;   // k-steps (32 deep) of a full chunk
  int32_t n_mblk;        // Cout blocks of MT
  int32_t relu;
  int32_t out_nchw_f32;
  int32_t store_stages;  // conv_m32p: stages that store the previous tile, when SCPOSE_NST overrides the kernel's own count; else 0
  // pipelined (persistent) variant
  const void* zero16;    // >= 16 zero bytes in global memory: what a masked lane of the 64-bit residual loads reads (conv_pipe, conv_m32; conv_m32p does not read it)
  int32_t items_total;   // (tile, Cout block) work items
  int32_t items_per_wg;
  int32_t grid;          // persistent workgroups
  int32_t lds_w, lds_x;  // bytes of one weight-chunk / input-chunk LDS buffer
  int32_t lds_bias;      // bytes reserved for the bias vector in LDS
  int32_t nbuf_w, nbuf_x;  // LDS buffers: weights 1 (resident) or 2, inputs 2 or 3
  int32_t tiles_total;   // N * tiles_x * tiles_y
  int32_t nt;            // pixel tiles per wave group processed one after the other on one staged weight chunk
  int32_t wreg_chunks;   // conv_m32p: K-chunks of weights held in producer registers (6 or 1)
  FastDiv fd_npix, fd_tw, fd_hp, fd_halo_w, fd_tiles_img, fd_tiles_x, fd_nmblk;   // conv_m32: divisions by launch constants
  uint32_t in_bytes, out_bytes;   // bytes of the input / output (= residual) tensors of this frame range: num_records of their
                                  // buffer descriptors (conv_pipe_kernel.h: dma16_buf), always set.  conv_pipe and conv_m32 address
                                  // only their input that way (output and residual through 64-bit pointers); conv_pipe leaves out_bytes 0.
  unsigned long long* dbg_buf;  // development build only (SCP_DBG_BUF): per-workgroup phase cycle sums (dbg & 8), else null
  int32_t dbg;           // development build only (SCP_DBG; the shipped library's kernels read neither field): bits 1 skip MFMA loop, 2 skip epilogue, 4 skip input DMA, 8 phase stamps
                         // bit 32 is the one bit the shipped library honours: the host prints the m32 tile choice (and for_frame_ranges its ranges)
  int32_t cu_share;      // host only: CUs to size the layer for (0 = the whole chip)
};

// Per-layer choice of kernel variant + tiling.
struct ConvConfig {
  int ks, stride;      // 1|3, 1|2
  int mrep, nrep;      // 16x16 MFMA tiles per wave along Cout / pixels
  int th, tw;          // output tile
  int cp;              // input planes (8 channels each) per K chunk
};

// A tiling of conv_launch_m32: th x tw output tile, nseg tiles per work item, nr (16x16x32 consumers: nb16) MFMA columns per wave,
// ps = bytes of a staged halo plane, occ = kernel family (1 / 2 workgroups per CU, 3 = producer/consumer), cp = planes per K-chunk
struct M32Tiling { int th = 0, tw = 0, nseg = 0, nr = 0, ps = 0, occ = 0, cp = 0, nb16 = 0; };

struct PackedConv {
  int cin, cout, ks, stride, dtype;
  int mt;              // cout block (16*mrep)
  int n_mblk;
  int cp, nchunks, ksteps_full;
  size_t wbytes;       // packed weight bytes
  void* d_w = nullptr;     // device packed weights
  float* d_bias = nullptr; // device bias (n_mblk*mt)
  int mrep;
  int variant = 0;     // 0: 16x16x32 MFMA kernel (conv_pipe), 1: 32x32x16 kernel (conv_m32)
  int wm = 1;          // variant 1: waves along Cout (mt = 32*mrep*wm)
  // streaming 1x1 kernel (conv1x1.hip): weights [k-step][k-group][cout_pad1][8] and bias in MFMA row order, when eligible
  void* d_w1 = nullptr;
  float* d_b1 = nullptr;
  size_t w1_bytes = 0;
  int cout_pad1 = 0;
  // tiling chosen by conv_launch_m32 for the last (N, Ho, Wo, CUs) seen (the search is a function of those and the layer only)
  struct TileMemo { int n = -1, ho = 0, wo = 0, cus = 0; M32Tiling t; };
  mutable TileMemo m32_memo[2];   // [0] whole chip, [1] a share of it (concurrent lanes)
  // register-weight stride-2 kernel (conv_s2r.hip): weights [k-step][cout block][k-group][row][8], bias in MFMA row order
  void* d_ws2 = nullptr;
  float* d_bs2 = nullptr;
};
bool conv_s2r_config(int cin, int cout, int stride, int* planes, int* nblk, int* g);
size_t conv_s2r_pack(const float* w, int cout, int cin, int dtype, uint16_t* dst);
void conv_s2r_pack_bias(const float* bias, int cout, float* dst);
int32_t conv_s2r_launch(const PackedConv& pc, const void* in, int N, int H, int W, int relu, void* out, hipStream_t stream);
bool conv1x1_stream_eligible(const PackedConv& pc);
int32_t conv1x1_stream_launch(const PackedConv& pc, const void* in, int N, int H, int W, const void* res, int relu,
                              void* out, hipStream_t stream);

// Pick (mrep, cp) for a layer independent of the spatial size; tiles are chosen per launch.
void choose_mrep_cp(int cin, int cout, int ks, int stride, int* mrep, int* cp);
// Choose spatial tiling for an output map.
void choose_tile(int ks, int stride, int Ho, int Wo, int* nrep, int* th, int* tw);

// Host: fold-free packing of f32 OIHW weights into the kernel's LDS image order.
// Returns bytes; fills `dst` (16-bit words) when non-null.
size_t pack_conv_weights(const float* w, int cout, int cin, int ks, int mt, int cp, int dtype,
                         uint16_t* dst, int* nchunks, int* ksteps_full);

int32_t conv_upload(const float* w, const float* bias, int cout, int cin, int ks, int stride,
                    int dtype, PackedConv* pc);
void conv_free(PackedConv* pc);
// cu_share > 0: the caller runs other layers beside this one (concurrent lanes of the captured forward); a small 3x3 layer
// then sizes its grid and tiles for that many CUs instead of the whole chip (same results: tiling never changes a pixel's sum)
int32_t conv_launch(const PackedConv& pc, const void* in, int N, int H, int W, const void* res,
                    int relu, int out_nchw_f32, void* out, hipStream_t stream, int cu_share = 0);
size_t conv_lds_bytes(const PackedConv& pc, int nrep, int th, int tw);
int plane_stride_for(int stride, int halo_h, int halo_w);
// software-pipelined persistent kernel (conv_pipe_kernel.h); nt = pixel tiles per work item
int32_t conv_launch_pipe(const PackedConv& pc, ConvLaunch& L, int nrep, int nt, int occ, hipStream_t stream);
size_t conv_pipe_lds_bytes(const PackedConv& pc, int plane_stride);
const void* conv_zero_page();   // lazily allocated 256 zero bytes on the current device
// fused BasicBlock (conv_block_kernel.h): out = relu(conv2(relu(conv1(x))) + x) for C -> C -> C 3x3 layers
bool block_fusable(const PackedConv& c1, const PackedConv& c2);
int32_t block_launch(const PackedConv& c1, const PackedConv& c2, const void* in, int N, int H, int W, void* out,
                     hipStream_t stream);
int conv_device_cus();
unsigned long long* conv_dbg_buffer(hipStream_t stream);   // development instrumentation
void conv_dbg_set_grid(int grid);
// PackedConv::mrep value of the 48-row Cout block of the producer/consumer kernel's 3 x 8 form (conv_m32p_kernel.h, M16 = 3): one and
// a half 32-row units have no integer; mt = 48
constexpr int kMrep48 = 15;
// 32x32x16-MFMA kernel (conv_m32_kernel.h): layer eligibility + variant, packing, launch
bool conv_m32_choose(int cin, int cout, int ks, int stride, int* mr, int* wm, int* cp);
size_t pack_conv_weights_m32(const float* w, int cout, int cin, int ks, int mt, int cp, int dtype,
                             uint16_t* dst, int* nchunks, int* ksteps_full);
int32_t conv_launch_m32(const PackedConv& pc, ConvLaunch& L, hipStream_t stream);   // SCPOSE_E_UNSUPPORTED-free: returns 1 if the shape has no good tiling (caller falls back)

// ---- stem: 3 -> 64 -> 64, two 3x3 stride-2 convolutions from f32 NCHW or u8 NHWC -------------
// fused stem (stem_fused.hip): conv1 + bn1 + relu + conv2 + bn2 + relu in one launch, both on MFMA
void stem_fused_pack(const float* w1, const float* b1, const float* w2, const float* b2, int dtype, std::vector<uint16_t>* pw1,
                     std::vector<uint16_t>* pw2, std::vector<float>* pb1, std::vector<float>* pb2);
int32_t stem_fused_launch(const void* in, int in_fmt, const void* w1, const void* w2, const float* b1, const float* b2,
                          const float* mean_std, int N, int H, int W, int dtype, void* out,
                          uint32_t* sched /*2 zero-initialised device words: dynamic tile queue (conv_device.h: tile_claim)*/, hipStream_t stream);

// fused layer1 Bottleneck (bottleneck.hip): conv1 1x1 Cin->64, conv2 3x3 64->64, conv3 1x1 64->256 + residual in one launch;
// Cin = 256: identity residual; Cin = 64: the first Bottleneck, its `downsample` projection (wds, bds) folded into conv3
bool bottleneck_fusable(int cin, int cmid, int cout);
void bottleneck_pack(const float* w1, const float* w2, const float* w3, const float* wds, const float* b1, const float* b2, const float* b3,
                     const float* bds, int cin, int dtype,
                     std::vector<uint16_t>* pw1, std::vector<uint16_t>* pw2, std::vector<uint16_t>* pw3, std::vector<float>* pb);
int32_t bottleneck_launch(const void* in, const void* w1, const void* w2, const void* w3, const float* bias, int N, int H, int W,
                          int cin, int dtype, void* out, uint32_t* sched /*11 zero-initialised device words: per-XCD tile queues [0..7], finished workgroups [8], device-wide queue of the first Bottleneck [9..10]*/,
                          hipStream_t stream);

// fuse row 0 + the first hop of every down path from branch 0 of a HighResolutionModule, one pass over branch 0 (fuse_down.hip)
struct FuseDownPacked {
  void* d_w = nullptr;     // conv_s2r_pack of the concatenated first-hop convolutions [2 c0 | c0 | c0][c0][3][3]
  float* d_b = nullptr;
  int c0 = 0, nb = 0, dtype = 0;
};
bool fuse_down_supported(int nb, int c0, int c1);
int32_t fuse_down_upload(const float* w, const float* bias, int nb, int c0, int dtype, FuseDownPacked* fd);
void fuse_down_free(FuseDownPacked* fd);
int32_t fuse_down_launch(const FuseDownPacked& fd, const void* x0, int N, int H, int W, const void* const* terms, void* y,
                         void* const* outs, hipStream_t stream);

// ---- pose_resnet: stem, transposed convolution, 1x1 stride-2 projection ----------------------
// ResNet stem (resnet_stem.hip): conv 7x7 s2 p3 3 -> 64 + BN + ReLU + max-pool 3x3 s2 p1 in one launch
void resnet_stem_pack(const float* w, int dtype, std::vector<uint16_t>* pw);
int32_t resnet_stem_launch(const void* in, int in_fmt, const void* w, const float* bias, const float* mean_std, int N, int H, int W,
                           int dtype, void* out, hipStream_t stream);
// gather convolution (conv_gather.hip): ConvTranspose2d k 4 / 3 / 2 stride 2 by output parity class, Conv2d 1x1 stride 2
struct GatherClass {
  int32_t ntaps, dy[4], dx[4];   // input offsets of the class's taps relative to si * (my, mx)
  int32_t py, px;                // the class's output position relative to so * (my, mx)
  long long w_off;               // first A fragment of the class (16-byte units)
};
struct GatherLaunch {
  const void* in; const void* w; const float* bias; const void* res; void* out;
  int32_t N, H, W, Ho, Wo, Hb, Wb;   // input map, output map, base grid
  int32_t cin, cout, nclass, si, so, relu;
  GatherClass cls[4];
};
struct GatherPacked {
  void* d_w = nullptr;
  float* d_bias = nullptr;
  int cin = 0, cout = 0, dtype = 0, nclass = 0, si = 1, so = 1, ks = 1;   // ks: the layer's kernel size (statistics only)
  GatherClass cls[4];
};
// w: folded f32 [cout][cin][k][k] (a ConvTranspose2d weight transposed to the Conv2d order, NOT flipped), bias [cout]
int32_t deconv_upload(const float* w, const float* bias, int cout, int cin, int k, int dtype, GatherPacked* gp);
int32_t conv1x1s2_upload(const float* w, const float* bias, int cout, int cin, int dtype, GatherPacked* gp);
void gather_free(GatherPacked* gp);
void gather_out_size(const GatherPacked& gp, int H, int W, int* Ho, int* Wo);
int32_t gather_launch(const GatherPacked& gp, const void* in, int N, int H, int W, const void* res, int relu, void* out,
                      hipStream_t stream);

// ---- elementwise ---------------------------------------------------------------------------
int32_t fuse_sum_launch(const void* const* terms, const int32_t* shifts, int nterms, int N, int C,
                        int H, int W, int dtype, void* out, hipStream_t stream);
int32_t crop_warp_launch(const uint8_t* frames, const int64_t* offsets, const int32_t* hw, const double* minv,
                         int N, int oh, int ow, int swap_rb, uint8_t* out, hipStream_t stream, const int32_t* roi = nullptr);
// events.hip: event stream -> event frames (v2e/convert_aedats.py: e2v.py's renderer + cv2.undistort)
int events_max_width();       // widest frame whose single row of int32 counters fits the LDS band
int32_t events_frame_bounds_launch(const int64_t* t, int64_t n, const double* starts, int F, int64_t* bounds, hipStream_t stream);
int32_t events_render_launch(const int32_t* x, const int32_t* y, const void* p, int p_bytes, const int64_t* bounds, int F,
                             int H, int W, int fs, int fold, const uint8_t* lut, const double* K, const double* dist,
                             uint8_t* frames, uint8_t* distorted, uint8_t* workspace, hipStream_t stream);
// events_exposure.hip: the frame bounds of the COUNT and AREA_COUNT exposure modes
size_t events_area_workspace_bytes(int64_t n, int64_t M, int D, int h, int w);
int32_t events_area_bounds_launch(const int32_t* x, const int32_t* y, int64_t n, int64_t M, int D, int h, int w, int64_t* bounds,
                                  int64_t capacity, int64_t* count_status, uint8_t* workspace, hipStream_t stream);
int32_t events_count_bounds_launch(int64_t N, int64_t F, int64_t* bounds, hipStream_t stream);
int32_t events_bounds_midpoints_launch(const int64_t* t, const int64_t* bounds, int64_t F, double* mids, hipStream_t stream);
// events_csv.hip: events.csv text -> (t, x, y, p)
size_t events_csv_workspace_bytes(int64_t n_bytes);
int32_t events_csv_parse_launch(const uint8_t* data, int64_t n_bytes, int ws_mode, int swap_xy, double t_div, int64_t* t, int32_t* x,
                                int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* ws, hipStream_t stream);
// events_write.hip: (t, x, y, p) -> event text / AEDAT-2.0 records
int events_text_tile_rows();
int events_text_scan_rows();
size_t events_text_workspace_bytes(int64_t n);
int32_t events_text_measure_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                   int64_t* count_status, uint8_t* ws, hipStream_t stream);
int32_t events_text_emit_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int sep, int swap_xy,
                                uint8_t* out, int64_t capacity, int64_t* count_status, uint8_t* ws, hipStream_t stream);
int32_t events_aedat2_pack_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int h, int w,
                                  uint8_t* out, int64_t* count_status, hipStream_t stream);
// events_aedat2_read.hip: AEDAT-2.0 records -> (t, x, y, p)
size_t events_aedat2_unpack_workspace_bytes(int64_t n);
int32_t events_aedat2_unpack_launch(const uint8_t* records, int64_t n, int h, int w, int layout, int flip_x, int flip_y, int unwrap,
                                    double t_div, int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                                    uint8_t* ws, hipStream_t stream);
// events_aedat3_read.hip: the polarity packets of an AEDAT-3.1 file -> (t, x, y, p)
size_t events_aedat3_workspace_bytes(int64_t n_packets);
int32_t events_aedat3_count_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* count_status, uint8_t* ws,
                                   hipStream_t stream);
int32_t events_aedat3_unpack_launch(const uint8_t* file, const int64_t* packets, int64_t n, int h, int w, int rebase, int64_t* t,
                                    int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* ws,
                                    hipStream_t stream);
// events_aedat4_read.hip: the event packets of an AEDAT-4.0 file -> (t, x, y, p)
size_t events_aedat4_workspace_bytes(int64_t n_packets);
int32_t events_aedat4_measure_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* total_status, uint8_t* ws,
                                     hipStream_t stream);
int32_t events_aedat4_decode_launch(const uint8_t* file, const int64_t* packets, int64_t n, uint8_t* staging, int64_t staging_bytes,
                                    int verify, uint8_t* ws, hipStream_t stream);
int32_t events_aedat4_count_launch(const uint8_t* src, const int64_t* packets, int64_t n, int staged, int64_t* count_status, uint8_t* ws,
                                   hipStream_t stream);
int32_t events_aedat4_unpack_launch(const uint8_t* src, int64_t n, int h, int w, int rebase, int64_t* t, int32_t* x, int32_t* y,
                                    int8_t* p, int64_t capacity, int64_t* count_status, uint8_t* ws, hipStream_t stream);
// events_aedat4_zstd.hip: the measure / decode pair for ZSTD payloads, on a workspace that starts with the reader's.  It fills
// the reader's per-packet slots (events_aedat4_slots) and closes its measure step with the reader's sizes step.
struct Aedat4Slots {
  int32_t* size;
  int64_t* off;
  int32_t* status;
};
Aedat4Slots events_aedat4_slots(int64_t n_packets, uint8_t* ws);
int32_t events_aedat4_sizes_launch(int64_t n, int64_t* total_status, uint8_t* ws, hipStream_t stream);
size_t events_aedat4_zstd_workspace_bytes(int64_t n_packets);
int32_t events_aedat4_zstd_measure_launch(const uint8_t* file, const int64_t* packets, int64_t n, int64_t* total_status, uint8_t* ws,
                                          hipStream_t stream);
int32_t events_aedat4_zstd_decode_launch(const uint8_t* file, const int64_t* packets, int64_t n, uint8_t* staging,
                                         int64_t staging_bytes, int verify, uint8_t* ws, hipStream_t stream);
// the limits of one packet that the reader holds its input to and the writer its output (events_aedat4_read.hip says why)
constexpr int kAedat4MaxDecoded = (1 << 23) - 16;
constexpr int kAedat4MaxCount = (1 << 23) - 1;
// events_aedat4_write.hip: (t, x, y, p) -> the event packets of an AEDAT-4.0 file; bytes -> LZ4 frames
struct Aedat4WriteSizes {
  size_t workspace_bytes, out_bytes;
};
Aedat4WriteSizes events_aedat4_pack_sizes(int64_t n, int64_t n_packets, int compression);
Aedat4WriteSizes events_aedat4_frame_sizes(int64_t n_bytes, int64_t n_packets);
int32_t events_aedat4_pack_launch(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, const int64_t* bounds,
                                  int64_t n_packets, int h, int w, int stream_id, int compression, uint8_t* out, int64_t capacity,
                                  int64_t* table, int64_t* total_status, uint8_t* ws, hipStream_t stream);
int32_t events_aedat4_frame_launch(const uint8_t* src, int64_t n_bytes, const int64_t* bounds, int64_t n_packets, uint8_t* out,
                                   int64_t capacity, int64_t* table, int64_t* total_status, uint8_t* ws, hipStream_t stream);
// jpeg_decode.hip: baseline JPEG files -> (N, H, W, 3) uint8 frames (jpeg_common.h: jpeg_blocks(h, w, mode), the blocks of one frame)
size_t jpeg_decode_workspace_bytes(int n, int h, int w, int mode, int max_subs);
int32_t jpeg_decode_launch(const uint8_t* desc, const int32_t* segs, int64_t n_rows, const uint8_t* data, int64_t n_bytes, int n, int h,
                           int w, int mode, int max_subs, int bgr, int max_rounds, uint8_t* out, uint8_t* y_out, int32_t* status,
                           uint8_t* ws, hipStream_t stream);
// the same files -> the crop_warp of each frame, (N, out_h, out_w, 3), without the frame.  roi_host: host int32 [n][4], each inside the frame
int32_t jpeg_decode_crop_launch(const uint8_t* desc, const int32_t* segs, int64_t n_rows, const uint8_t* data, int64_t n_bytes, int n, int h,
                                int w, int mode, int max_subs, int bgr, int max_rounds, const double* minv, const int32_t* roi_host,
                                int out_h, int out_w, uint8_t* crops, int32_t* status, uint8_t* ws, hipStream_t stream);

// jpeg_encode.hip: (N, H, W, 3) uint8 frames -> baseline JPEG byte streams; the overlay draw in front of it
size_t jpeg_encode_workspace_bytes(int n, int h, int w, int mode);
int64_t jpeg_encode_capacity_bytes(int n, int h, int w, int mode, int header_bytes);
// png_decode.hip: desc_host is host memory (n descriptors of SCPOSE_PNG_DESC_BYTES), uploaded into the workspace on `stream`
size_t png_decode_workspace_bytes(int n, int h, int w, int channels);
int32_t png_decode_launch(const uint8_t* desc_host, const uint8_t* data, int n, int h, int w, int channels, int bgr, uint8_t* out,
                          int32_t* status, uint8_t* ws, hipStream_t stream);
int32_t png_decode_crop_launch(const uint8_t* desc_host, const uint8_t* data, int n, int h, int w, int channels, int bgr, const double* minv,
                               const int32_t* roi_host, int out_h, int out_w, uint8_t* crops, int32_t* status, uint8_t* ws,
                               hipStream_t stream);
int32_t jpeg_encode_launch(const uint8_t* frames, int n, int h, int w, int mode, int quality, const uint32_t* huff, const uint8_t* header,
                           int header_bytes, uint8_t* out, int64_t capacity, int64_t* offsets, int32_t* status, uint8_t* ws,
                           hipStream_t stream);
int32_t overlay_draw_launch(uint8_t* frames, int n, int h, int w, const int32_t* bboxes, const double* points, int j, hipStream_t stream);
// resize_area.hip: uint8 frames -> area-resized frames or gray frames; the tables are host memory (w and h records of
// SCPOSE_RESIZE_AREA_REC_WORDS words, checked by the caller), uploaded into the workspace on `stream`
size_t resize_area_workspace_bytes(int h, int w);
int32_t resize_area_launch(const uint8_t* src, int F, int H, int W, int C, uint8_t* dst, int h, int w, int gray, int bgr, int box,
                           const int32_t* xtab_host, const int32_t* ytab_host, uint8_t* ws, hipStream_t stream);
// dvs_emulator.hip: intensity frames -> event stream (v2e/v2ecore/emulator.py: EventEmulator.generate_events)
size_t dvs_state_bytes(int h, int w);
size_t dvs_workspace_bytes(int h, int w, int frames, int max_iters);
int32_t dvs_init_launch(void* state, const uint8_t* frame0, double t0, int h, int w, const float* lut, double refractory_period_s,
                        hipStream_t stream);
int32_t dvs_emulate_launch(void* state, const uint8_t* frames, const double* t, int n_frames, const scpose_dvs_params& prm, float* t_s,
                           int64_t* t_us, int32_t* x, int32_t* y, int8_t* pol, int64_t capacity, int64_t* counts, uint8_t* ws,
                           hipStream_t stream);
int32_t head_gather_launch(const void* taps, const float* bias, const float* prev, int N, int J, int H, int W,
                           int K, int S, int dtype, float* out, hipStream_t stream);
int32_t heatmap_accumulate_launch(float* acc, const float* x, float div, size_t count, hipStream_t stream);
int32_t flip_merge_launch(const float* a, const float* b, const int32_t* perm, int N, int J, int H, int W, int shift,
                          float* out, hipStream_t stream);
int32_t nchw_to_blocked_launch(const float* src, int N, int C, int H, int W, int dtype, void* dst,
                               hipStream_t stream);
// Cd: channels of dst (the first Cd of the blocked tensor's C are copied); -1: all C
int32_t blocked_to_nchw_launch(const void* src, int N, int C, int H, int W, int dtype, float* dst,
                               hipStream_t stream, int Cd = -1);

// ---- decode / pnp --------------------------------------------------------------------------
// head_fused.hip: last fuse sum + final_layer (+ decode) in one pass (pose_hrnet.py:256-263, :458; lib/core/inference.py:18-79)
void head_fused_pack(const float* w, const float* b, int J, int C, int dtype, uint16_t* wfrag, float* bias);
size_t head_fused_part_bytes(int n);
bool head_fused_supported(int nterms, int C, int J, int N, int H, int W);
int32_t head_fused_launch(const void* const* terms, const int32_t* shifts, int nterms, int N, int C, int H, int W, int J,
                          int dtype, const void* wfrag, const float* bias, float* hm, float* part_v, int32_t* part_i,
                          const float* center, const float* scale, int post_process, float* preds, hipStream_t stream);
int32_t decode_launch(const float* hm, int N, int J, int H, int W, const float* center,
                      const float* scale, int post_process, float* preds_xyc, float* coords,
                      float* maxvals, hipStream_t stream);
int32_t pnp_launch(const float* kp_xyc, const double* landmarks, const double* K,
                   const double* dist, int N, int J, double conf_thr0, int min_pts, double thr_decay,
                   int thr_iters, int max_iters, double reproj_err, double confidence, double* rot,
                   double* tvec, double* rvec, int32_t* status, hipStream_t stream, double* rows = nullptr,
                   int refine_iters = 0, unsigned long long* inliers = nullptr);

// f32 -> 16-bit storage on the host (round to nearest even), matching the device casts.
uint16_t host_f32_to_16(float f, int dtype);
float host_16_to_f32(uint16_t v, int dtype);

}  // namespace scpose
