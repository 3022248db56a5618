// DVS emulator core on the device: time-stamped uint8 intensity frames -> an event stream in the columns events.hip takes.
//
// Restates EventEmulator._init / generate_events of the reference's v2e/v2ecore/emulator.py with lin_log, rescale_intensity_frame,
// low_pass_filter, subtract_leak_current and compute_event_map of emulator_utils.py, without shot noise and leak jitter (both draw
// random numbers per frame).  tests/dvs_emulator_restated.py is the executable statement of the semantics; this file equals it
// bit for bit.  This translation unit is compiled with -ffp-contract=off and correctly rounded division: every float32 step
// below is one IEEE operation, in the order of the reference's tensor expressions.
//
// Per frame, all on the stream, nothing read back:
//   update_kernel   per pixel: lin-log by table, low-pass, leak, ON / OFF counts (torch's fmod floor division), and the frame's
//                   num_iters as an integer atomicMax (order-independent)
//   count_kernel    per 64-pixel tile (one wavefront): walks the sub-iterations, refractory filter included, WITHOUT touching the
//                   state, and writes the tile's count of every group g = 2 * i + (0 ON, 1 OFF) into the group-major table
//                   table[g * tiles + tile].  Pixels are tiled in row-major order, so an exclusive scan of that table is the
//                   offset of the tile's first event of group g in the reference's unshuffled order
//   scan_*          scan_device.h's exclusive sum scan of the first 2 * num_iters * tiles entries.  That length is only known on
//                   the device: the launch covers 2 * max_iters * tiles entries and the workgroups past the length return at
//                   once.  The one-workgroup middle pass also advances the call's running event count and raises the status bits
//   scatter_kernel  the same walk again, now writing timestamp_mem and base; an event's rank inside its tile comes from the
//                   ballot of its group, so the output order is a fixed function of the input
// No floating-point atomic, no global atomic other than the integer maximum; two runs are bitwise equal.
#include "common.h"
#include "scan_device.h"

namespace scpose {

namespace {

constexpr int kThreads = 256;
static_assert(kThreads == kScanThreads, "the scan bodies of scan_device.h run in the workgroups of this file");
constexpr int kWave = 64;

struct DvsHeader {        // first 256 bytes of the state
  double t_prev;
  int32_t initialised;
  int32_t pad;
};

struct StateView {
  DvsHeader* hdr;
  float *base, *lp0, *lp1, *tmem;
  int32_t *on, *off;
};

// the state: a 256-byte header and six 256-byte aligned planes (ops.DvsEmulator.state() reads the first four)
inline size_t state_view(void* state, int h, int w, StateView* v) {
  const size_t hw = (size_t)h * w;
  Carve c{static_cast<uint8_t*>(state)};
  v->hdr = c.take<DvsHeader>(1);
  v->base = c.take<float>(hw);
  v->lp0 = c.take<float>(hw);
  v->lp1 = c.take<float>(hw);
  v->tmem = c.take<float>(hw);
  v->on = c.take<int32_t>(hw);
  v->off = c.take<int32_t>(hw);
  return c.bytes();
}

struct Workspace {
  int32_t* nit;        // [frames] num_iters of every frame (zeroed per call)
  int64_t* fbase;      // [frames + 1] events before every frame of this call
  int32_t* table;      // [2 * max_iters * tiles]
  int32_t* aggr;       // [scan blocks]
  size_t bytes;
};

inline Workspace workspace_view(uint8_t* ws, int h, int w, int frames, int max_iters) {
  const int64_t tiles = ((int64_t)h * w + kWave - 1) / kWave;
  const int64_t len = 2 * (int64_t)max_iters * tiles;
  Carve c{ws};
  Workspace v;
  v.nit = c.take<int32_t>(frames > 0 ? frames : 1);
  v.fbase = c.take<int64_t>(frames + 1);
  v.table = c.take<int32_t>(len);
  v.aggr = c.take<int32_t>((len + kScanTile - 1) / kScanTile);
  v.bytes = c.bytes();
  return v;
}

// what the kernels need of the parameters (pointers null: the scalar holds)
struct DevParams {
  int hw, w;
  float pos, neg;
  const float *pos_map, *neg_map, *noise_map;
  const float* lut;
  int cutoff, leak;
  double tau;
  float leak_rate, refr;
  int max_iters;
};

// the frame's time base: t_prev from the state for the first frame of a call, else the previous stamp
__device__ __forceinline__ double prev_time(const DvsHeader* hdr, const double* t, int f) { return f == 0 ? hdr->t_prev : t[f - 1]; }

// torch.div(a, b, rounding_mode="floor") for float32 (c10::div_floor_floating), b != 0
__device__ __forceinline__ float floor_div_f32(float a, float b) {
  const float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.f;
  if (div != 0.f) {
    float fl = floorf(div);
    if (div - fl > 0.5f) fl += 1.f;
    return fl;
  }
  return copysignf(0.f, a / b);
}

__global__ __launch_bounds__(kThreads) void init_kernel(DvsHeader* hdr, float* base, float* lp0, float* lp1, float* tmem,
                                                        const uint8_t* __restrict__ frame, const float* __restrict__ lut, int hw,
                                                        double t0, float refr) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
    hdr->t_prev = t0;
    hdr->initialised = 1;
    hdr->pad = 0;
  }
  if (i >= hw) return;
  const float v = lut[frame[i]];
  base[i] = v;
  lp0[i] = v;
  lp1[i] = v;
  tmem[i] = 0.f - refr;
}

__global__ __launch_bounds__(kThreads) void update_kernel(StateView s, DevParams p, const uint8_t* __restrict__ frame,
                                                          const double* __restrict__ t, int f, int32_t* __restrict__ nit,
                                                          int64_t* __restrict__ counts) {
  const double tp = prev_time(s.hdr, t, f), tf = t[f];
  if (!(tf > tp)) {                                        // the reference raises ValueError; every later kernel skips too
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[1] |= SCPOSE_DVS_TIME;
    return;
  }
  if (counts[1] & (SCPOSE_DVS_ITERS | SCPOSE_DVS_TIME)) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  int m = 0;
  if (i < p.hw) {
    const double dt = tf - tp;
    const int px = frame[i];
    const float log_new = p.lut[px];
    float lp0n, lp1n;
    if (p.cutoff) {
      const float inten01 = ((float)px + 20.f) / 275.f;
      float eps = inten01 * (float)(dt / p.tau);
      eps = eps > 1.f ? 1.f : eps;
      const float old0 = s.lp0[i];
      const float a = (1.f - eps) * old0;
      const float b = eps * log_new;
      lp0n = a + b;
      lp1n = old0;
    } else {
      lp0n = log_new;
      lp1n = log_new;
    }
    s.lp0[i] = lp0n;
    s.lp1[i] = lp1n;
    const float pth = p.pos_map ? p.pos_map[i] : p.pos;
    const float nth = p.neg_map ? p.neg_map[i] : p.neg;
    float base = s.base[i];
    if (p.leak) {
      const float rate = p.leak_rate * (p.noise_map ? p.noise_map[i] : 1.f);
      const float dl = ((float)dt * rate) * pth;
      base = base - dl;
      s.base[i] = base;
    }
    const float diff = lp1n - base;
    const int on = (int)floor_div_f32(fmaxf(diff, 0.f), pth);
    const int off = (int)floor_div_f32(fmaxf(-diff, 0.f), nth);
    s.on[i] = on;
    s.off[i] = off;
    m = on > off ? on : off;
  }
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const int v = __shfl_xor(m, o);
    m = v > m ? v : m;
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && m > 0) atomicMax(&nit[f], m);      // integer: order-independent
}

// the stamps of a frame: ts_step = reciprocal(n) * dt in float32, ts = linspace(t_prev + ts_step, t_frame, n) as torch's CPU
// kernel evaluates it (one rounding per element: the float64 product of two float32 values is exact)
struct Stamps {
  float start, end, step, ts_step;
  int n, half;
  __device__ __forceinline__ float at(int i) const {
    if (n == 1) return start;
    return i < half ? (float)((double)start + (double)step * (double)i) : (float)((double)end - (double)step * (double)(n - 1 - i));
  }
};

__device__ __forceinline__ Stamps make_stamps(double tp, double tf, int n) {
  Stamps st;
  st.n = n;
  st.half = n / 2;
  const float recip = 1.f / (float)n;
  st.ts_step = recip * (float)(tf - tp);
  st.start = (float)tp + st.ts_step;
  st.end = (float)tf;
  st.step = n > 1 ? (st.end - st.start) / (float)(n - 1) : 0.f;
  return st;
}

// one sub-iteration of one pixel (emulator.py:534-562): which polarities fire, and the refractory memory
__device__ __forceinline__ void sub_iteration(int i, float ts, int on, int off, bool valid, bool filt, float refr, float& tm, bool& pos,
                                              bool& neg) {
  pos = valid && on >= i + 1;
  neg = valid && off >= i + 1;
  if (filt) {
    const float ps = (pos ? ts : 0.f) - tm;            // cord * ts[i] - timestamp_mem: an inactive pixel evaluates 0 - mem
    const float ns = (neg ? ts : 0.f) - tm;
    pos = valid && ps > refr;
    neg = valid && ns > refr;
    if (pos || neg) tm = ts;
  }
}

__global__ __launch_bounds__(kThreads) void count_kernel(StateView s, DevParams p, const double* __restrict__ t, int f,
                                                         const int32_t* __restrict__ nit, int32_t* __restrict__ table, int tiles,
                                                         int64_t* __restrict__ counts) {
  const int n = nit[f];
  if (n == 0 || n > p.max_iters || (counts[1] & (SCPOSE_DVS_ITERS | SCPOSE_DVS_TIME))) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int tile = i / kWave, lane = threadIdx.x & (kWave - 1);
  if (tile >= tiles) return;                             // whole wavefronts only
  const bool valid = i < p.hw;
  const int on = valid ? s.on[i] : 0, off = valid ? s.off[i] : 0;
  float tm = valid ? s.tmem[i] : 0.f;
  const Stamps st = make_stamps(prev_time(s.hdr, t, f), t[f], n);
  const bool filt = p.refr > st.ts_step;
  for (int it = 0; it < n; ++it) {
    bool pos, neg;
    sub_iteration(it, st.at(it), on, off, valid, filt, p.refr, tm, pos, neg);
    const int cp = __popcll(__ballot(pos)), cn = __popcll(__ballot(neg));
    if (lane == 0) {
      table[(int64_t)(2 * it) * tiles + tile] = cp;
      table[(int64_t)(2 * it + 1) * tiles + tile] = cn;
    }
  }
}

// ---- exclusive int32 sum scan of table[0 .. 2 * nit[f] * tiles), in place.  Every workgroup reads the length on the device; one
// whose tile starts at or past it returns before any barrier, all of its threads alike
__device__ __forceinline__ int64_t scan_len(const int32_t* nit, int f, int tiles, int max_iters, const int64_t* counts) {
  const int n = nit[f];
  if (n > max_iters || (counts[1] & (SCPOSE_DVS_ITERS | SCPOSE_DVS_TIME))) return 0;
  return 2 * (int64_t)n * tiles;
}

__global__ __launch_bounds__(kThreads) void scan_reduce_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ nit,
                                                               int f, int tiles, int max_iters, const int64_t* __restrict__ counts,
                                                               int32_t* __restrict__ aggr) {
  __shared__ int32_t sm[kThreads];
  const int64_t len = scan_len(nit, f, tiles, max_iters, counts);
  if ((int64_t)blockIdx.x * kScanTile >= len) return;
  scan_tile_reduce<0, false>(table, len, aggr, sm);
}

// one workgroup: aggr[b] <- sum of aggr[0 .. b - 1]; then the call's running event count and the status bits
__global__ __launch_bounds__(kThreads) void scan_aggr_kernel(int32_t* __restrict__ aggr, const int32_t* __restrict__ nit, int f,
                                                             int tiles, int max_iters, int64_t capacity, int64_t* __restrict__ fbase,
                                                             int64_t* __restrict__ counts) {
  __shared__ int32_t sm[kThreads];
  const int64_t len = scan_len(nit, f, tiles, max_iters, counts);
  const int32_t events = scan_aggregates<0>(aggr, (len + kScanTile - 1) / kScanTile, sm);
  __syncthreads();                                         // every thread has read the status word before it changes
  if (threadIdx.x == 0) {
    const int64_t after = fbase[f] + events;
    fbase[f + 1] = after;
    int64_t status = counts[1];
    if (nit[f] > max_iters) status |= SCPOSE_DVS_ITERS;
    if (after > capacity) status |= SCPOSE_DVS_CAPACITY;
    counts[0] = after;
    counts[1] = status;
  }
}

__global__ __launch_bounds__(kThreads) void scan_apply_kernel(int32_t* table, const int32_t* __restrict__ nit, int f, int tiles,
                                                              int max_iters, const int64_t* __restrict__ counts,
                                                              const int32_t* __restrict__ aggr) {
  __shared__ int32_t sm[kThreads];
  const int64_t len = scan_len(nit, f, tiles, max_iters, counts);
  if ((int64_t)blockIdx.x * kScanTile >= len) return;
  scan_tile_apply<0, false, true>(table, table, len, aggr, sm);
}

struct OutColumns {
  float* t_s;
  int64_t* t;
  int32_t *x, *y;
  int8_t* p;
  int64_t capacity;
};

__global__ __launch_bounds__(kThreads) void scatter_kernel(StateView s, DevParams p, const double* __restrict__ t, int f,
                                                           const int32_t* __restrict__ nit, const int32_t* __restrict__ table,
                                                           int tiles, const int64_t* __restrict__ fbase, OutColumns out,
                                                           const int64_t* __restrict__ counts) {
  const int n = nit[f];
  if (n > p.max_iters || (counts[1] & (SCPOSE_DVS_ITERS | SCPOSE_DVS_TIME))) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int tile = i / kWave, lane = threadIdx.x & (kWave - 1);
  if (tile >= tiles) return;
  const bool valid = i < p.hw;
  const int on = valid ? s.on[i] : 0, off = valid ? s.off[i] : 0;
  float tm = valid ? s.tmem[i] : 0.f;
  int fin_on = 0, fin_off = 0;
  if (n > 0) {
    const Stamps st = make_stamps(prev_time(s.hdr, t, f), t[f], n);
    const bool filt = p.refr > st.ts_step;
    const unsigned long long below = (1ull << lane) - 1;
    const int64_t first = fbase[f];
    const int px = i % p.w, py = i / p.w;
    for (int it = 0; it < n; ++it) {
      bool pos, neg;
      const float ts = st.at(it);
      sub_iteration(it, ts, on, off, valid, filt, p.refr, tm, pos, neg);
      const unsigned long long bp = __ballot(pos), bn = __ballot(neg);
      fin_on += pos;
      fin_off += neg;
      if (pos || neg) {
        // the reference's h5 rule for the integer stamp: uint32(float32(ts) * 1e6), the product in float32, truncated
        const int64_t us = (int64_t)(uint32_t)(int64_t)(ts * 1e6f);
        if (pos) {
          const int64_t q = first + table[(int64_t)(2 * it) * tiles + tile] + __popcll(bp & below);
          if (q < out.capacity) { out.t_s[q] = ts; out.t[q] = us; out.x[q] = px; out.y[q] = py; out.p[q] = 1; }
        }
        if (neg) {
          const int64_t q = first + table[(int64_t)(2 * it + 1) * tiles + tile] + __popcll(bn & below);
          if (q < out.capacity) { out.t_s[q] = ts; out.t[q] = us; out.x[q] = px; out.y[q] = py; out.p[q] = 0; }
        }
      }
    }
  }
  if (valid) {
    const float pth = p.pos_map ? p.pos_map[i] : p.pos;
    const float nth = p.neg_map ? p.neg_map[i] : p.neg;
    float base = s.base[i];
    base = base + (float)fin_on * pth;
    base = base - (float)fin_off * nth;
    s.base[i] = base;
    s.tmem[i] = tm;
  }
}

// after the last frame of a call: the state's time base moves on (unless a frame was refused)
__global__ void finish_kernel(DvsHeader* hdr, const double* __restrict__ t, int frames, const int64_t* __restrict__ counts) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && !(counts[1] & (SCPOSE_DVS_ITERS | SCPOSE_DVS_TIME))) hdr->t_prev = t[frames - 1];
}

}  // namespace

size_t dvs_state_bytes(int h, int w) {
  StateView v;
  return state_view(nullptr, h, w, &v);
}

size_t dvs_workspace_bytes(int h, int w, int frames, int max_iters) { return workspace_view(nullptr, h, w, frames, max_iters).bytes; }

int32_t dvs_init_launch(void* state, const uint8_t* frame0, double t0, int h, int w, const float* lut, double refractory_period_s,
                        hipStream_t stream) {
  StateView s;
  state_view(state, h, w, &s);
  const int hw = h * w;
  hipLaunchKernelGGL(init_kernel, dim3((hw + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, s.hdr, s.base, s.lp0, s.lp1, s.tmem,
                     frame0, lut, hw, t0, (float)refractory_period_s);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

int32_t dvs_emulate_launch(void* state, const uint8_t* frames, const double* t, int n_frames, const scpose_dvs_params& prm, float* t_s,
                           int64_t* t_us, int32_t* x, int32_t* y, int8_t* pol, int64_t capacity, int64_t* counts, uint8_t* ws,
                           hipStream_t stream) {
  const int h = prm.h, w = prm.w, hw = h * w;
  StateView s;
  state_view(state, h, w, &s);
  const Workspace wk = workspace_view(ws, h, w, n_frames, prm.max_iters);
  DevParams p{};
  p.hw = hw; p.w = w;
  p.pos = prm.pos_thres; p.neg = prm.neg_thres;
  p.pos_map = prm.pos_thres_map; p.neg_map = prm.neg_thres_map; p.noise_map = prm.noise_rate_map;
  p.lut = prm.lin_log_table;
  p.cutoff = prm.cutoff_hz > 0.0;
  p.leak = prm.leak_rate_hz > 0.0;
  p.tau = p.cutoff ? 1.0 / (M_PI * 2 * prm.cutoff_hz) : 1.0;
  p.leak_rate = (float)prm.leak_rate_hz;
  p.refr = (float)prm.refractory_period_s;
  p.max_iters = prm.max_iters;
  const OutColumns out{t_s, t_us, x, y, pol, capacity};
  const int tiles = (hw + kWave - 1) / kWave;
  const int64_t len = 2 * (int64_t)prm.max_iters * tiles;
  const unsigned scan_blocks = (unsigned)((len + kScanTile - 1) / kScanTile);
  const unsigned px_blocks = (unsigned)(((int64_t)tiles * kWave + kThreads - 1) / kThreads);
  SCP_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), stream));
  SCP_CHECK_HIP(hipMemsetAsync(wk.nit, 0, (size_t)(n_frames > 0 ? n_frames : 1) * 4, stream));
  SCP_CHECK_HIP(hipMemsetAsync(wk.fbase, 0, sizeof(int64_t), stream));
  for (int f = 0; f < n_frames; ++f) {
    const uint8_t* frame = frames + (size_t)f * hw;
    hipLaunchKernelGGL(update_kernel, dim3(px_blocks), dim3(kThreads), 0, stream, s, p, frame, t, f, wk.nit, counts);
    hipLaunchKernelGGL(count_kernel, dim3(px_blocks), dim3(kThreads), 0, stream, s, p, t, f, wk.nit, wk.table, tiles, counts);
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(scan_blocks), dim3(kThreads), 0, stream, wk.table, wk.nit, f, tiles, prm.max_iters,
                       counts, wk.aggr);
    hipLaunchKernelGGL(scan_aggr_kernel, dim3(1), dim3(kThreads), 0, stream, wk.aggr, wk.nit, f, tiles, prm.max_iters, capacity,
                       wk.fbase, counts);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(scan_blocks), dim3(kThreads), 0, stream, wk.table, wk.nit, f, tiles, prm.max_iters,
                       counts, wk.aggr);
    hipLaunchKernelGGL(scatter_kernel, dim3(px_blocks), dim3(kThreads), 0, stream, s, p, t, f, wk.nit, wk.table, tiles, wk.fbase, out,
                       counts);
  }
  if (n_frames > 0) hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, stream, s.hdr, t, n_frames, counts);
  SCP_CHECK_HIP(hipGetLastError());
  return SCPOSE_OK;
}

}  // namespace scpose
