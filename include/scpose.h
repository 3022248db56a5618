/*
 * scpose.h -- C ABI of the MI355X (gfx950) HRNet -> heatmap decode -> EPnP/RANSAC library.
 *
 * The reference (mohsij/spacecraft-pose-estimation) has no FFI for this path; the path sits
 * behind Python call signatures.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference repo root).  INTEGRATION.md shows the ctypes
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns int32 status: 0 = ok, <0 = SCPOSE_E_*; the message of the last
 *     failure on the calling thread is returned by scpose_last_error().  Nothing throws.
 *   - OWNERSHIP: the host (PyTorch) allocates and owns every device buffer passed in
 *     (inputs, outputs, workspace).  The library owns only the opaque handle and the packed
 *     weights it uploads at create time (freed by scpose_hrnet_destroy).
 *   - STREAMS: every launch function takes a hipStream_t as void*; nothing synchronises
 *     internally and nothing allocates in a launch function, with one exception: the first
 *     launch of a kernel on a device opts that kernel into large LDS (hipFuncSetAttribute) and,
 *     for 64-bit-addressed tensors, allocates a 256-byte zero page -- both memoised PER DEVICE.
 *     Run one forward eagerly on a device before capturing launches into a hipGraph there
 *     (scpose_hrnet_graph_* below does so itself).
 *   - THREADING: a handle is bound to the device current at create time and is not
 *     thread-safe; distinct handles are independent.  The only process-wide state is the
 *     per-device memoisation above (idempotent, indexed by device id) and the thread-local
 *     error message.
 *   - ONE STREAM PER HANDLE AT A TIME: besides its read-only weights a handle owns a few words
 *     of mutable device state -- the dynamic tile queues of its persistent kernels (16 words
 *     per layer, self-resetting at the end of each launch).  All launches that use one handle
 *     -- eager forwards AND replays of graphs captured from it -- must therefore be ordered
 *     with respect to each other (same stream, or event dependencies); two forwards of one
 *     handle in flight at once would claim tiles from the same queue.  Every other buffer a
 *     forward writes lies in the caller's workspace.  For concurrent forwards create one
 *     handle per stream.
 *   - "blocked" activation layout used between layers: [N][C/8][H][W][8] 16-bit elements
 *     (bf16 or f16), C a multiple of 8.
 *   - NO CPU ENTRY POINTS: this library has no host implementation of any function below and no fallback -- every
 *     function needs a gfx950 device and fails with SCPOSE_E_HIP without one.  (SURVEY.md section 8b sketched
 *     `scpose_cpu_*` twins for the CPU baseline; they are deliberately not part of the ABI: the CPU restatement of
 *     the path is test infrastructure and lives under oracle/ -- hrnet_ref.py, decode_ref.py, pnp_ref.c, warp_ref.py --
 *     where only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it; tests/test_abi.py checks
 *     that nothing under the package, the CLIs or bench.py's measured path imports it.)
 */
#ifndef SCPOSE_H
#define SCPOSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCPOSE_ABI_VERSION 7

enum {
  SCPOSE_OK = 0,
  SCPOSE_E_INVALID = -1,   /* bad argument / unsupported shape */
  SCPOSE_E_MISSING = -2,   /* a required checkpoint tensor was not supplied */
  SCPOSE_E_HIP = -3,       /* a HIP runtime call failed */
  SCPOSE_E_WORKSPACE = -4, /* workspace too small */
  SCPOSE_E_NOMEM = -5
};

/* 16-bit storage / MFMA operand type of the network (accumulation is always fp32). */
enum { SCPOSE_DT_BF16 = 0, SCPOSE_DT_F16 = 1 };

/* output head = cfg.MODEL.NAME (landmark_regression/lib/models/):
 *   FINAL_LAYER  pose_hrnet.py:323-329   final_layer conv on branch 0, heat-maps H/4 x W/4
 *   CMS          hrnet_cms.py:353-419, :551-557   four ConvTranspose2d(k5,s4)+Conv2d heads summed coarse-to-fine
 *                with bilinear x2 upsampling, heat-maps H x W ("equal_to_image")
 *   CMS_384      hrnet_cms_384.py (same, k3 s2), heat-maps H/2 x W/2 ("4x") */
enum { SCPOSE_HEAD_FINAL_LAYER = 0, SCPOSE_HEAD_CMS = 1, SCPOSE_HEAD_CMS_384 = 2 };

/* input formats of scpose_hrnet_forward */
enum {
  SCPOSE_IN_F32_NCHW = 0,  /* normalised float32 N x 3 x H x W: what the reference module's
                              forward(x) receives (landmark_regression/tools/test.py:106-114) */
  SCPOSE_IN_U8_NHWC = 1    /* raw uint8 N x H x W x 3 RGB crop; ToTensor + Normalize(mean,std)
                              of tools/test.py:106-108 is fused into the stem kernel */
};

int32_t scpose_abi_version(void);
const char* scpose_last_error(void);
/* 0 for the shipped library (libscpose_hip.so: no instrumentation or ablation path compiled into any kernel), 1 for the
 * development build of the same sources (libscpose_hip_dev.so, -DSCPOSE_DEV_BUILD), which tools_dev/ loads with SCPOSE_DEV=1. */
int32_t scpose_is_dev_build(void);

/* ------------------------------------------------------------------------------------------
 * HRNet.  Replaces models.pose_hrnet.get_pose_net(cfg, is_train=False) + load_state_dict +
 * PoseHighResolutionNet.forward
 * (landmark_regression/lib/models/pose_hrnet.py:274-331, :425-460, :495-501;
 *  call sites landmark_regression/tools/test.py:84-98, lib/core/function.py:341).
 * ---------------------------------------------------------------------------------------- */
typedef struct scpose_hrnet_desc {
  int32_t num_joints;          /* cfg.MODEL.NUM_JOINTS */
  int32_t final_conv_kernel;   /* cfg.MODEL.EXTRA.FINAL_CONV_KERNEL (1 or 3) */
  int32_t num_stages;          /* always 3 (STAGE2..STAGE4) */
  int32_t num_modules[3];      /* EXTRA.STAGEk.NUM_MODULES */
  int32_t num_branches[3];     /* EXTRA.STAGEk.NUM_BRANCHES (2,3,4) */
  int32_t num_blocks[3][4];    /* EXTRA.STAGEk.NUM_BLOCKS (blocks per branch) */
  int32_t num_channels[3][4];  /* EXTRA.STAGEk.NUM_CHANNELS (the block's planes: a BOTTLENECK branch carries 4x as many channels) */
  int32_t dtype;               /* SCPOSE_DT_* */
  float mean[3], std[3];       /* Normalize() constants for SCPOSE_IN_U8_NHWC */
  int32_t head;                /* SCPOSE_HEAD_*: which member of the model family (cfg.MODEL.NAME) */
  int32_t block[3];            /* EXTRA.STAGEk.BLOCK (blocks_dict, pose_hrnet.py:266-269): 0 BASIC, 1 BOTTLENECK (expansion 4) */
} scpose_hrnet_desc;

typedef struct scpose_hrnet* scpose_hrnet_t;

/* names/ptrs/numels: the checkpoint's state_dict as HOST float32 arrays (conv weights OIHW),
 * keyed exactly as the reference module's state_dict ("conv1.weight", "bn1.running_var",
 * "stage3.2.fuse_layers.1.0.0.0.weight", "final_layer.bias", ...).  Unknown keys are ignored
 * (num_batches_tracked etc.); a missing required key fails with SCPOSE_E_MISSING unless
 * allow_missing != 0, in which case the tensor takes the reference constructor's default
 * (strict=False behaviour of tools/test.py:90: BN -> identity, conv -> zeros).
 * BatchNorm (eval, eps 1e-5) is folded into the conv weights/bias here and the result is
 * packed for the MFMA kernels and uploaded. */
int32_t scpose_hrnet_create(const scpose_hrnet_desc* desc, const char* const* names,
                            const float* const* ptrs, const int64_t* numels, int32_t count,
                            int32_t allow_missing, scpose_hrnet_t* out);
int32_t scpose_hrnet_destroy(scpose_hrnet_t h);

/* pose_resnet (landmark_regression/lib/models/pose_resnet.py, the SimpleBaseline network): ResNet trunk, NUM_DECONV_LAYERS
 * stride-2 ConvTranspose2d + BN + ReLU layers, a final 1x1 / 3x3 layer.  Returns the SAME handle type: every entry point
 * that takes a scpose_hrnet_t works on it unchanged (scpose_hrnet_tail_fused reports 0: the tail is not fused, and
 * scpose_hrnet_forward_decode runs forward + decode).  Heat-maps are H/32 * 2^L x W/32 * 2^L for L deconv layers.
 * State-dict keys are the reference module's: conv1.weight, bn1.*, layerK.B.convN / bnN / downsample.0 / downsample.1,
 * deconv_layers.{3i, 3i+1}.*, final_layer.*; allow_missing and unknown keys as for scpose_hrnet_create.  A deconv filter
 * count that is no multiple of 16 is carried at the next multiple (zero planes). */
typedef struct scpose_resnet_desc {
  int32_t num_joints;          /* cfg.MODEL.NUM_JOINTS */
  int32_t final_conv_kernel;   /* EXTRA.FINAL_CONV_KERNEL (1 or 3) */
  int32_t num_layers;          /* EXTRA.NUM_LAYERS: 18, 34, 50, 101, 152 */
  int32_t num_deconv_layers;   /* EXTRA.NUM_DECONV_LAYERS: 0..4 */
  int32_t deconv_filters[4];   /* EXTRA.NUM_DECONV_FILTERS */
  int32_t deconv_kernels[4];   /* EXTRA.NUM_DECONV_KERNELS: 4, 3 or 2 (padding / output_padding as _get_deconv_cfg) */
  int32_t deconv_with_bias;    /* EXTRA.DECONV_WITH_BIAS */
  int32_t dtype;               /* SCPOSE_DT_* */
  float mean[3], std[3];       /* Normalize() constants for SCPOSE_IN_U8_NHWC */
} scpose_resnet_desc;
int32_t scpose_resnet_create(const scpose_resnet_desc* desc, const char* const* names,
                             const float* const* ptrs, const int64_t* numels, int32_t count,
                             int32_t allow_missing, scpose_hrnet_t* out);

/* bytes of device workspace scpose_hrnet_forward needs for a batch of n frames of h x w. */
int32_t scpose_hrnet_workspace_bytes(scpose_hrnet_t h, int32_t n, int32_t height, int32_t width,
                                     size_t* bytes);
/* heat-map size scpose_hrnet_forward writes for an input of height x width: H/4 (pose_hrnet, the
 * cfg.MODEL.HEATMAP_SIZE of the shipped YAMLs), H (hrnet_cms) or H/2 (hrnet_cms_384). */
int32_t scpose_hrnet_heatmap_size(scpose_hrnet_t h, int32_t height, int32_t width, int32_t* out_h,
                                  int32_t* out_w);
/* number of kernel launches of one forward and total conv FLOPs (2*MAC) per frame. */
int32_t scpose_hrnet_stats(scpose_hrnet_t h, int32_t height, int32_t width, int32_t* launches,
                           double* flops_per_frame, double* act_bytes_per_frame);
/* the same two figures for the work the launches DO.  A NUM_CHANNELS entry that is no multiple of 16 is carried at
 * the next multiple (its added planes are zero: zero weights, zero bias), so a W18 / W30 / W40 / W44 network executes
 * more than scpose_hrnet_stats -- the algorithmic work at the widths the model describes -- reports.  Equal to
 * scpose_hrnet_stats for widths that are multiples of 16. */
int32_t scpose_hrnet_executed_stats(scpose_hrnet_t h, int32_t height, int32_t width,
                                    double* flops_per_frame, double* act_bytes_per_frame);

/* in: device pointer in in_fmt; heatmaps: device float32 N x J x H/4 x W/4 (scpose_hrnet_heatmap_size for the
 * hrnet_cms heads) (NCHW, raw scores,
 * exactly what the reference forward returns).  H and W must be multiples of 32. */
int32_t scpose_hrnet_forward(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n,
                             int32_t height, int32_t width, float* heatmaps, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Forward + decode in one call: the key points of validate() / the pose exporter without a heat-map round trip through HBM.
 * Replaces the pair model(input) -> get_final_preds(output, center, scale) of landmark_regression/lib/core/function.py:376-393
 * (lib/core/inference.py:18-79, lib/utils/transforms.py:49-110); arguments as scpose_hrnet_forward and scpose_decode.
 * For pose_hrnet with FINAL_CONV_KERNEL == 1 the last fuse sum, final_layer and the decode run as one pass over the
 * branch-0 tensor (head_fused.hip): `heatmaps` may then be NULL and nothing is written for them; when it is given it
 * receives exactly what scpose_hrnet_forward writes.  Other heads (3x3 final layer, hrnet_cms) need `heatmaps` and run
 * forward + scpose_decode back to back on `stream`.  preds_xyc is bit-identical to scpose_decode(scpose_hrnet_forward(...)). */
int32_t scpose_hrnet_tail_fused(scpose_hrnet_t h, int32_t n, int32_t height, int32_t width, int32_t* fused);   /* 1: heatmaps may be NULL */
int32_t scpose_hrnet_forward_decode(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n, int32_t height,
                                    int32_t width, const float* center, const float* scale, int32_t post_process,
                                    float* preds_xyc, float* heatmaps, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* Captured forward.  The launch list of one forward for a FIXED (input buffer, batch shape, heat-map buffer, workspace)
 * is recorded once into a hipGraph and replayed with one call: for small batches the host-side launch cost of the
 * ~280 kernels disappears, and with concurrent != 0 the ops that do not depend on each other -- the branches of a
 * HighResolutionModule (pose_hrnet.py:247-253), the rows of its fuse layer (:254-265), the transition convolutions
 * (:333-372) -- are recorded on parallel graph branches, so that the small-grid kernels of the low-resolution
 * branches fill the CUs the high-resolution ones leave idle.  concurrent == 2 puts only the fuse rows and the transition
 * convolutions side by side (many short HBM-bound launches) and runs the branches one after the other: the choice for
 * batches whose branch kernels each fill the chip (W48 384x384 batch 256: -0.3 ms; with concurrent == 1 the MFMA-bound
 * branch kernels contend and the forward gets slower).  Results are bit-identical to scpose_hrnet_forward.
 * The concurrent memory plan keeps a tensor alive until every op that may run beside its last reader has finished:
 * size the workspace with scpose_hrnet_graph_workspace_bytes (>= scpose_hrnet_workspace_bytes).
 * create runs one eager forward on an internal stream (it needs valid input in `in`) and synchronises it; launch
 * only enqueues.  The caller refills `in` and reads `heatmaps` in stream order around scpose_hrnet_graph_launch. */
typedef struct scpose_hrnet_graph* scpose_hrnet_graph_t;
int32_t scpose_hrnet_graph_workspace_bytes(scpose_hrnet_t h, int32_t n, int32_t height, int32_t width, size_t* bytes);
int32_t scpose_hrnet_graph_create(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n, int32_t height,
                                  int32_t width, float* heatmaps, void* workspace, size_t workspace_bytes,
                                  int32_t concurrent, scpose_hrnet_graph_t* out);
/* the captured form of scpose_hrnet_forward_decode (center / scale / preds_xyc / heatmaps are baked in like `in`) */
int32_t scpose_hrnet_graph_create_decode(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n, int32_t height,
                                         int32_t width, const float* center, const float* scale, int32_t post_process,
                                         float* preds_xyc, float* heatmaps, void* workspace, size_t workspace_bytes,
                                         int32_t concurrent, scpose_hrnet_graph_t* out);
int32_t scpose_hrnet_graph_launch(scpose_hrnet_graph_t g, void* stream);
int32_t scpose_hrnet_graph_nodes(scpose_hrnet_graph_t g, int32_t* nodes);   /* kernel + dependency nodes captured */
int32_t scpose_hrnet_graph_destroy(scpose_hrnet_graph_t g);

/* Unit-level parity hook: runs the forward up to and including the op that produces the named intermediate tensor
 * and writes it as float32 N x C x h x w (converted from the 16-bit blocked layout).  Names follow the forward of
 * pose_hrnet.py:425-460: "stem2" (:429-431; the stem's first tap: conv1's output never leaves the fused stem kernel), "layer1" (:432), "stage<S>.<M>.out0" = y_list[0]
 * after module M of stage S (:247-265).  Every other tensor an op writes is offered too, named by the reference module
 * path that produces it: "layer1.<b>", "transition<k>.<i>" and hops "transition<k>.<i>.<j>", block outputs
 * "stage<S>.<M>.branches.<B>.<K>" and, where a block runs as separate launches, its intermediates "<block>.conv1" (and
 * "<block>.conv2" of a Bottleneck), fuse up paths "stage<S>.<M>.fuse_layers.<i>.<j>" (before upsampling), down hops
 * "stage<S>.<M>.fuse_layers.<i>.<j>.<k>", every fuse row "stage<S>.<M>.out<i>", and the 16-bit tap map of each hrnet_cms
 * head "<head>.tapmap".  With out == NULL only *channels / *out_h / *out_w are filled (shape query). */
int32_t scpose_hrnet_tap_names(scpose_hrnet_t h, char* buf, int32_t cap);   /* comma-separated names this handle offers */
int32_t scpose_hrnet_forward_tap(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n, int32_t height,
                                 int32_t width, const char* tap, float* out, int32_t* channels, int32_t* out_h,
                                 int32_t* out_w, void* workspace, size_t workspace_bytes, void* stream);

/* Measurement hooks (bench.py): the same forward with a HIP event recorded on `stream` before
 * every launch and after the last one, then per-launch milliseconds, algorithmic FLOPs and
 * bytes per frame and a kernel signature {kind, 10*ksize+stride | nterms, Cin, Cout} with kind
 * 0 stem conv1 alone (two-layer stem), 1 convolution, 2 fuse sum, 3 fused BasicBlock, 4 head gather
 * (hrnet_cms), 5 fused stem (conv1 + conv2), 6 fused Bottleneck, 7 fused tail (last fuse sum + final_layer; the fuse op it absorbs
 * reports no work).  profile_read blocks on the last event.  Call with ms == NULL to get *count. */
int32_t scpose_hrnet_forward_profiled(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n,
                                      int32_t height, int32_t width, float* heatmaps,
                                      void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 6) the same hook for scpose_hrnet_forward_decode: the launch list of the key-point path (fused tail with the decode
 * inside, no heat-map written when `heatmaps` is NULL) -- what bench.py's timed steps replay -- with per-launch events */
int32_t scpose_hrnet_forward_decode_profiled(scpose_hrnet_t h, const void* in, int32_t in_fmt, int32_t n, int32_t height,
                                             int32_t width, const float* center, const float* scale, int32_t post_process,
                                             float* preds_xyc, float* heatmaps, void* workspace, size_t workspace_bytes,
                                             void* stream);
int32_t scpose_hrnet_profile_read(scpose_hrnet_t h, int32_t height, int32_t width, int32_t cap,
                                  float* ms, double* flops_per_frame, double* bytes_per_frame,
                                  int32_t* sig, int32_t* count);

/* ------------------------------------------------------------------------------------------
 * Heatmap decode.  Replaces get_max_preds + get_final_preds + transform_preds
 * (landmark_regression/lib/core/inference.py:18-79, lib/utils/transforms.py:49-110) and the
 * all_preds assembly of validate() (lib/core/function.py:389-393).
 *   heatmaps  device f32 N x J x H x W
 *   center    device f32 N x 2, scale device f32 N x 2 (meta['center'], meta['scale'])
 *   preds_xyc device f32 N x J x 3 = [x_img, y_img, maxval]
 * post_process = cfg.TEST.POST_PROCESS.  One wavefront per (n, j) map.
 * ---------------------------------------------------------------------------------------- */
int32_t scpose_decode(const float* heatmaps, int32_t n, int32_t j, int32_t h, int32_t w,
                      const float* center, const float* scale, int32_t post_process,
                      float* preds_xyc, void* stream);
/* get_max_preds alone: coords device f32 N x J x 2 (heatmap px), maxvals device f32 N x J. */
int32_t scpose_max_preds(const float* heatmaps, int32_t n, int32_t j, int32_t h, int32_t w,
                         float* coords, float* maxvals, void* stream);

/* Crop pre-processing.  Replaces, per sample, cv2.warpAffine(frame, get_affine_transform(c, s, 0,
 * IMAGE_SIZE), IMAGE_SIZE, flags=INTER_LINEAR) and the COLOR_RGB channel swap of
 * landmark_regression/lib/dataset/JointsDataset.py:134-150, :191-195.
 *   frames    device u8: the samples' full frames (H_i x W_i x 3, any sizes) packed back to back
 *   offsets   device i64 N: byte offset of sample i's frame inside `frames`
 *   frame_hw  device i32 N x 2: (H_i, W_i)
 *   minv      device f64 N x 6: row-major 2x3 INVERSE of the reference's `trans` (crop pixel -> frame pixel),
 *             inverted the way cv::warpAffine does it (OpenCV 3.4 imgwarp.cpp; utils/transforms.py:invert_affine_cv)
 *   crops     device u8 N x out_h x out_w x 3 = the SCPOSE_IN_U8_NHWC input of scpose_hrnet_forward
 * swap_rb != 0 exchanges channels 0 and 2 (BGR frame -> RGB crop).  Border value 0.  Arithmetic: OpenCV's
 * fixed-point uint8 path (coordinates quantised to 1/32 px, integer weights scaled by 2^15, (sum + 2^14) >> 15). */
int32_t scpose_crop_warp(const uint8_t* frames, const int64_t* offsets, const int32_t* frame_hw,
                         const double* minv, int32_t n, int32_t out_h, int32_t out_w, int32_t swap_rb,
                         uint8_t* crops, void* stream);
/* (ABI 7) The same warp when only a WINDOW of every frame is resident: windows = packed uint8 (roi_h x roi_w x 3) blocks at
 * offsets[i], roi_xywh = device i32 N x 4 [x0, y0, w, h] of window i inside its frame, frame_hw = the FULL frame's size (the
 * border rule is the frame's).  The caller guarantees that every tap the warp reads inside the frame lies inside the window
 * (dataset/JointsDataset.py computes it from the affine); taps outside a window read 0.  Same crops, bit for bit, for a
 * fraction of the host-to-device bytes (a 1920 x 1200 frame is 6.9 MB, the window of a 300 px target 0.5 MB). */
int32_t scpose_crop_warp_roi(const uint8_t* windows, const int64_t* offsets, const int32_t* frame_hw,
                             const int32_t* roi_xywh, const double* minv, int32_t n, int32_t out_h,
                             int32_t out_w, int32_t swap_rb, uint8_t* crops, void* stream);

/* Event stream -> event frames: stage 0 of the reference's event pipeline, v2e/convert_aedats.py = `e2v.py --dvs_exposure
 * duration 10000 --dvs_vid_full_scale 2` (v2e/v2ecore/renderer.py: render_events_to_frames, accumulate_event_frame;
 * v2ecore/v2e_utils.py: hist2d_numba_seq) followed by cv2.undistort of every frame.  Additive in ABI 7.
 * The stream is time-sorted and lives in device memory as separate columns: t (i64 ticks, |t| < 2^53), x, y (i32), p (i8 or
 * i32; ON is p == 1, anything else is OFF; not read when fold_polarity != 0).
 *
 * scpose_events_frame_bounds: frame k takes the events [searchsorted(t, starts[k], left), searchsorted(t, starts[k+1], right)),
 * the end clamped to n_events - 1 (the reference never draws the last event of a stream); an event exactly on a boundary is
 * counted in both neighbouring frames.
 *   starts   device f64 F + 1: the frame start times, accumulated on the host by repeated float64 addition as the reference
 *            does (event_render.py: frame_schedule)
 *   bounds   device i64 F x 2: [begin, end) of every frame's slice of the stream
 *
 * scpose_events_render: histogram (row = y, column = x, events outside the frame dropped) of every frame's slice, every
 * polarity counted +1 (fold_polarity != 0, what e2v.py does) or ON minus OFF; the sum is clipped to [-full_scale, full_scale]
 * AFTER summation and mapped through gray_lut (device u8, 2 * full_scale + 1 entries for c = -full_scale ... full_scale; the
 * reference's uint8(((c + fs) / float(2 * fs)) * 255), built on the host) to three equal channels.
 *   K, dist     device f64 3 x 3 row-major and [k1, k2, p1, p2, k3]: undistort every frame as cv2.undistort(img, K, dist) does
 *               (source position through the forward distortion model in float64, new camera matrix = K, quantised to 1/32 px,
 *               the fixed-point bilinear tap of scpose_crop_warp, border 0); both NULL: no undistortion
 *   frames      device u8 F x h x w x 3: the (undistorted) frames, back to back: the `frames` of scpose_crop_warp with
 *               offsets[k] = k * h * w * 3
 *   distorted   device u8 F x h x w x 3 or NULL: also keep the frames before undistortion
 *   workspace   caller-owned, scpose_events_workspace_bytes(F, h, w); only used when K is given
 * Frames may be rendered in chunks (bounds + 2 * k, any F): chunked output equals one call.  Integer counters in LDS, no
 * global atomic: the output is bitwise deterministic.  F == 0 is a no-op; full_scale 1..127; w <= 40896 (one row of counters
 * must fit the LDS), h, w <= 32767, h * w <= 2^24. */
int32_t scpose_events_workspace_bytes(int32_t n_frames, int32_t h, int32_t w, size_t* bytes);
int32_t scpose_events_frame_bounds(const int64_t* t, int64_t n_events, const double* starts, int32_t n_frames,
                                   int64_t* bounds, void* stream);
int32_t scpose_events_render(const int32_t* x, const int32_t* y, const void* p, int32_t p_itemsize, const int64_t* bounds,
                             int32_t n_frames, int32_t h, int32_t w, int32_t full_scale, int32_t fold_polarity,
                             const uint8_t* gray_lut, const double* K, const double* dist, uint8_t* frames,
                             uint8_t* distorted, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) The other two exposure modes of the reference's renderer (`e2v.py --dvs_exposure count N` and
 * `--dvs_exposure area_count M D`): they produce the bounds array scpose_events_render takes, whose histogram, clip and gray
 * table are unchanged.  n_events is the length of the stream; a frame is written only while its end is < n_events - 1.
 *
 * scpose_events_count_frames / _count_bounds: COUNT N (N >= 1), frame k = [kN, (k+1)N); F = (n_events - 2) / N frames
 * (0 below 2 events), known on the host.  _count_bounds writes the first n_frames <= F of them.
 *
 * scpose_events_area_bounds: AREA_COUNT M D (M >= 2, D >= 1).  Event i belongs to area (x // D, y // D) of the
 * (1 + w // D) x (1 + h // D) grid, floor division and Python's negative wraparound (x in [-nw * D, nw * D), y likewise).  A
 * frame starts at s with every area counter at zero and ends at the first e >= s whose area has received M events in [s, e];
 * it is [s, e) and e opens the next frame.  Computed as a suffix minimum over a stable sort of (area, index) and a log-depth
 * chain extraction (csrc/events_exposure.hip): no per-frame serial step, no global atomic, bitwise deterministic.
 *   x, y          device i32 n_events; n_events <= 2^31 - 1
 *   bounds        device i64 capacity x 2; capacity >= (n_events - 2) / (M - 1), the most frames a stream can hold
 *   count_status  device i64 [2] <- [F, status]: status 0 ok, 1 a coordinate off the area grid (the reference raises
 *                 IndexError there; F = 0 and nothing is written), 2 internal capacity error (F = 0)
 *   workspace     caller-owned, scpose_events_area_bounds_workspace_bytes(n_events, M, D, h, w)
 * The frame count is only known on the device: read count_status back before sizing the frames of scpose_events_render.
 *
 * scpose_events_bounds_midpoints: mids[k] = (t[begin_k] + t[end_k]) / 2 (an int64 sum, then float64): the reference's frame
 * time in both modes, whose '{:.0f}' is the frame's file stem.  t device i64, bounds device i64 n_frames x 2, mids device f64. */
int32_t scpose_events_count_frames(int64_t n_events, int64_t count, int64_t* n_frames);
int32_t scpose_events_count_bounds(int64_t n_events, int64_t count, int64_t n_frames, int64_t* bounds, void* stream);
int32_t scpose_events_area_bounds_workspace_bytes(int64_t n_events, int64_t area_count, int32_t area_dimension, int32_t h,
                                                  int32_t w, size_t* bytes);
int32_t scpose_events_area_bounds(const int32_t* x, const int32_t* y, int64_t n_events, int64_t area_count,
                                  int32_t area_dimension, int32_t h, int32_t w, int64_t* bounds, int64_t capacity,
                                  int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_bounds_midpoints(const int64_t* t, const int64_t* bounds, int64_t n_frames, double* mids, void* stream);

/* events.csv on the device (csrc/events_csv.hip): the file's bytes -> the four columns scpose_events_frame_bounds /
 * scpose_events_render take, rows in file order.  Replaces pd.read_csv(file, header=None, comment='#', delim_whitespace=...,
 * names=[t, x, y, p]) + .values.astype(np.int64) of v2e/e2v.py:116-138 on the part of that reader's grammar where a row depends
 * on its own line only; on that part the columns equal the reader's element for element.
 *   accepted     line ends '\n', '\r\n', '\r', a last line without one; empty lines, lines of spaces / tabs and lines that start
 *                with '#' are skipped; a '#' later in a line cuts it; exactly four fields per row, separated by ',' with spaces /
 *                tabs around fields ignored (delim_whitespace == 0) or by runs of spaces / tabs (!= 0); a field is
 *                [+-]? digits [. digits] or [+-]? . digits, its value the integer part (truncation toward zero, as the
 *                reader's float64 column cast to int64 gives); t fits int64, x and y int32, p int8
 *   unsupported  (status SCPOSE_CSV_UNSUPPORTED, n_rows = 0, column contents unspecified -- never a different answer): any other
 *                byte outside a comment (exponents, quotes, hex, nan, inf), an empty field, fewer or more than four fields, a
 *                value out of range, spaces / tabs followed by '#', a column that holds a '.' in one field and more than 15
 *                digit characters in one field (the reader's float64 column is exact only up to 15 digits), a line whose part
 *                before any '#' is 64 KiB or longer (one thread walks a line), and directly after
 *                a '\r' without '\n': a row that begins with a space / tab (comma mode), a line of only spaces / tabs
 *                (whitespace mode) -- the reader's tokenizer gives both a meaning of its own
 *   data         device u8 n_bytes, 16-byte aligned; offsets are 64-bit throughout, files above 2^31 bytes are untested
 *   swap_xy      != 0: the second field goes to y and the third to x
 *   t_divisor    0: none; 1e6 / 1e3: t <- (int64)((double)t / t_divisor), the reader's --microseconds_timestamp /
 *                --milliseconds_timestamp
 *   t, x, y, p   device i64 / i32 / i32 / i8, capacity rows each; (n_bytes + 1) / 8 rows always suffice (a row takes 8 bytes)
 *   count_status device i64 [2] <- [n_rows, status]: status 0 ok, SCPOSE_CSV_UNSUPPORTED, SCPOSE_CSV_CAPACITY (more rows than
 *                capacity: n_rows = 0).  The row count is only known on the device: read count_status back once.
 *   workspace    caller-owned, 16-byte aligned, scpose_events_csv_workspace_bytes(n_bytes)
 * No allocation, no synchronisation; two calls on the same bytes give bitwise equal outputs. */
enum { SCPOSE_CSV_UNSUPPORTED = 1, SCPOSE_CSV_CAPACITY = 2 };
int32_t scpose_events_csv_workspace_bytes(int64_t n_bytes, size_t* bytes);
int32_t scpose_events_csv_parse(const uint8_t* data, int64_t n_bytes, int32_t delim_whitespace, int32_t swap_xy, double t_divisor,
                                int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Event files from the device (csrc/events_write.hip): the four columns -> the bytes of a text / CSV file or of AEDAT-2.0
 * records, the way out that mirrors scpose_events_csv_parse.
 *
 * Text: a row is `t SEP a SEP b SEP p '\n'`, (a, b) = (x, y), or (y, x) with swap_xy != 0 (the reader's flag, so that
 * parse(format(cols, swap), swap) == cols); every value as C's "%d" prints it; `"%d %d %d %d\n" % row` of v2e/v2e.py:write_text
 * byte for byte.  The bytes lie inside the grammar scpose_events_csv_parse accepts.  Two calls, as scpose_events_count_frames +
 * scpose_events_render: measure, read [n_bytes, status] back once, size the output, emit.
 *   t, x, y, p   device i64 / i32 / i32 / i8, n rows each (n == 0: may be NULL)
 *   sep          ' ' (32) or ',' (44)
 *   measure      count_status device i64 [2] <- [n_bytes, 0]; n_bytes is 64-bit, a row takes 8 .. 50 bytes.  Leaves the tile
 *                offsets in the workspace, which emit reads: the same columns, n and workspace go to both calls
 *   emit         out device u8, 16-byte aligned, `capacity` bytes; count_status <- [n_bytes, status], status 0 or
 *                SCPOSE_TEXT_CAPACITY when capacity < n_bytes: nothing is stored at or past `capacity`, the bytes below it are
 *                the prefix of the text
 *   workspace    caller-owned, 16-byte aligned, scpose_events_text_workspace_bytes(n)
 *   tiling       tile_rows: rows per workgroup; scan_rows: rows per step of the offset scan (sizes at which tests look)
 *
 * AEDAT-2.0 (jAER): per event two big-endian 32-bit words, address = xf << 12 | yf << 22 | p << 11 computed in uint32 with
 * xf = w - 1 - x, yf = h - 1 - y, then (int32) t in microseconds: the records of the reference's v2ecore/output/aedat2_output.py
 * (AEDat2Output.appendEvents), which flips both axes for every size it takes.
 *   h, w         h 1 .. 1024 (the 10 bits above bit 22), w 1 .. 1280 (the reference's widest sensor; from x = 1024 on the x field
 *                shares bit 22 with y, in the reference's files as here)
 *   out          device u8, 8-byte aligned, 8 * n bytes
 *   count_status device i64 [3] <- [n, status, lead].  status bits: SCPOSE_AEDAT2_RANGE (some x outside [0, w), y outside [0, h)
 *                or p outside {0, 1}), SCPOSE_AEDAT2_TIME (some t outside [0, 2^31): the reference's cast is undefined there);
 *                with either set the records are unspecified.  lead: how many leading records start with the byte '#' (0x23:
 *                yf in 140 .. 143); the reference drops exactly those from the first non-empty write to a file, and so does
 *                the host writer (event_write.write_events_aedat2)
 * Argument errors (null pointers with n > 0, n < 0, another separator, h outside 1 .. 1024 or w outside 1 .. 1280, a workspace that is too small)
 * return -1 with a message before anything is launched.  No allocation, no synchronisation, no floating point; two calls on
 * the same columns give bitwise equal bytes. */
enum { SCPOSE_TEXT_CAPACITY = 1 };
enum { SCPOSE_AEDAT2_RANGE = 1, SCPOSE_AEDAT2_TIME = 2 };
int32_t scpose_events_text_tiling(int32_t* tile_rows, int32_t* scan_rows);
int32_t scpose_events_text_workspace_bytes(int64_t n, size_t* bytes);
int32_t scpose_events_text_measure(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                   int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_text_emit(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int32_t sep,
                                int32_t swap_xy, uint8_t* out, int64_t capacity, int64_t* count_status, void* workspace,
                                size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat2_pack(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n, int32_t h,
                                  int32_t w, uint8_t* out, int64_t* count_status, void* stream);

/* (ABI 7, additive) AEDAT-2.0 records on the device (csrc/events_aedat2_read.hip): the bytes after a file's '#' header -> the four
 * columns scpose_events_frame_bounds / scpose_events_render take, kept events in file order.  The inverse of
 * scpose_events_aedat2_pack, and a reader of jAER's DAVIS recordings.  A record is two big-endian uint32 words, (address, time stamp).
 *   records      device u8, 8-byte aligned, 8 * n_records bytes (n_records == 0: the data pointers may be NULL)
 *   layout       SCPOSE_AEDAT2_LAYOUT_DAVIS: jAER's DAVIS word.  Bit 31 set: an APS / IMU sample, dropped and counted in n_other.
 *                Bit 31 clear and bit 10 set: a special event, dropped and counted in n_special.  Otherwise a polarity event: p =
 *                bit 11, x field = bits 12-21, y field = bits 22-30.  h 1 .. 512, w 1 .. 1024.
 *                SCPOSE_AEDAT2_LAYOUT_V2E: what AEDat2Output of the reference and scpose_events_aedat2_pack write.  Every record is
 *                a polarity event; the y field is bits 22-31 (the writer's 692x520 sets bit 31 for its flipped y >= 512, which jAER
 *                itself would misread).  h 1 .. 1024, w 1 .. 1024: the 1280-wide size is refused, because from x = 1024 on the
 *                writer ORs bit 10 of x into bit 0 of y and the word cannot be inverted.
 *   flip_x/y     != 0: x = w - 1 - x field, y = h - 1 - y field, what both writers do (unpack(pack(cols)) == cols); 0: the field
 *   range        a polarity event whose x field is outside [0, w) or y field outside [0, h) sets status bit
 *                SCPOSE_AEDAT2_READ_RANGE; the columns are then unspecified -- never a different answer silently
 *   unwrap       with u_i the time stamp word of record i as uint32, over ALL records, dropped ones included:
 *                0: t = (int64)(int32)u.  != 0: t_i = u_i + 2^32 * wraps_i, wraps_i = #{ j in 1 .. i : u_{j-1} > u_j and
 *                u_{j-1} - u_j > 2^31 }.  A signed roll-over (0x7fffffff -> 0x80000000) is an increase and needs nothing, a full
 *                32-bit roll-over adds 2^32, a smaller step back is not a wrap.
 *   t_divisor    0: none; 1e3 / 1e6: t <- (int64)((double)t / t_divisor) afterwards, as scpose_events_csv_parse
 *   t, x, y, p   device i64 / i32 / i32 / i8, capacity rows each; n_records rows always suffice
 *   count_status device i64 [6] <- [n_events, status, n_other, n_special, n_wraps, n_backward].  n_wraps: the wraps of the whole
 *                stream (counted whatever unwrap says).  n_backward: kept events whose final t is below the previous kept event's:
 *                the renderer needs a sorted stream, the caller decides.  SCPOSE_AEDAT2_READ_CAPACITY: more kept events than
 *                capacity; nothing is stored at or past `capacity` and n_events = 0.  Read count_status back once.
 *   workspace    caller-owned, 16-byte aligned, scpose_events_aedat2_unpack_workspace_bytes(n_records) (never 0)
 * Argument errors (a null pointer with n_records > 0, a null count_status or workspace, n_records < 0, capacity < 0, an unknown
 * layout, h or w outside the layout's range -- "not supported" --, a divisor other than 0, 1e3, 1e6, a misaligned buffer, a workspace
 * that is too small) return -1 with a message before anything is launched.  Three launches, a tile of 4096 records per workgroup:
 * count, scan, scatter; 16 bytes read and at most 17 written per record.  No allocation, no synchronisation, no atomics on the
 * columns, no floating point except the divisor; two calls on the same bytes give bitwise equal outputs. */
enum { SCPOSE_AEDAT2_LAYOUT_DAVIS = 0, SCPOSE_AEDAT2_LAYOUT_V2E = 1 };
enum { SCPOSE_AEDAT2_READ_RANGE = 1, SCPOSE_AEDAT2_READ_CAPACITY = 2 };
int32_t scpose_events_aedat2_unpack_workspace_bytes(int64_t n_records, size_t* bytes);
int32_t scpose_events_aedat2_unpack(const uint8_t* records, int64_t n_records, int32_t h, int32_t w, int32_t layout,
                                    int32_t flip_x, int32_t flip_y, int32_t unwrap, double t_divisor,
                                    int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity,
                                    int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) The polarity packets of an AEDAT-3.1 recording on the device (csrc/events_aedat3_read.hip, which states the
 * format): the whole file and one descriptor per polarity packet -> the four columns, the valid events in file order.  The host
 * reads the text header and walks the 28-byte packet headers (event_read.parse_aedat3).  Two calls on one workspace, in this order,
 * and one small read-back between them:
 *   _count     one workgroup per packet counts the events whose valid bit is set.  count_status device i64 [6] <- [n_events, status,
 *              t of the first valid event, 0, 0, 0]; n_events = 0 unless status is 0.  Read back; allocate the columns.
 *   _unpack    the valid events -> t = (eventTSOverflow << 31) | ts (minus the first t when rebase != 0), x = data bits 17..31,
 *              y = data bits 2..16, p = data bit 1.  Adds to count_status [3] n_backward (events whose t is below their
 *              predecessor's) and [4] n_out_of_range (x >= w or y >= h; sets SCPOSE_AEDAT3_RANGE).  Writes nothing unless status
 *              was 0 and n_events <= capacity (else SCPOSE_AEDAT3_CAPACITY).  Read count_status back once more for the counters.
 *   file       device u8, the recording, no alignment asked; packets: device i64 [n_packets][3], (payload offset in file,
 *              eventNumber, eventTSOverflow) of each polarity packet, the payload's eventNumber * 8 bytes and the 28 header bytes
 *              before it inside the file -- the caller's duty, the kernels check every read against eventNumber * 8 only
 *   status     SCPOSE_AEDAT3_CORRUPT: an event (valid or not) with a negative ts, a descriptor with a payload offset below 4, an
 *              eventNumber outside 0 .. 2^23 - 1 (256 counts are summed in an int32) or an eventTSOverflow outside 0 .. 2^31 - 1.
 *              _VALID_MISMATCH: the valid bits of a packet do not add up to the eventValid its header states (the int32 4 bytes
 *              before the payload).  The kernels detect and never interpret.
 *   workspace  caller-owned, 16-byte aligned, scpose_events_aedat3_workspace_bytes(n_packets) (never 0), the SAME for both calls
 * Argument errors (null pointers, n_packets < 0 or above 2^31 - 1, h or w outside 1 .. 32768, a misaligned or short workspace)
 * return -1 with a message before anything is launched.  No allocation, no synchronisation, no atomics on the columns, integer
 * work only; two runs on the same bytes give bitwise equal outputs. */
enum { SCPOSE_AEDAT3_CORRUPT = 1, SCPOSE_AEDAT3_VALID_MISMATCH = 2, SCPOSE_AEDAT3_RANGE = 4, SCPOSE_AEDAT3_CAPACITY = 8 };
int32_t scpose_events_aedat3_workspace_bytes(int64_t n_packets, size_t* bytes);
int32_t scpose_events_aedat3_count(const uint8_t* file, const int64_t* packets, int64_t n_packets, int64_t* count_status,
                                   void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat3_unpack(const uint8_t* file, const int64_t* packets, int64_t n_packets, int32_t h, int32_t w, int32_t rebase,
                                    int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) The event packets of an AEDAT-4.0 recording on the device (csrc/events_aedat4_read.hip, which states the format):
 * the whole file and one descriptor per event packet -> the four columns, events in file order.  The host reads the IOHeader and
 * walks the packet headers (event_read.parse_aedat4).  Four calls on one workspace, in this order; _measure and _decode only when
 * the payloads are LZ4 frames (compression LZ4 / LZ4_HIGH), and two small read-backs size the buffers between them:
 *   _measure   one wavefront per packet walks the frame without copying; total_status device i64 [2] <- [staging bytes, status].
 *              Read back; allocate `staging` of that many bytes (a multiple of 16, 0 included).
 *   _decode    one wavefront per packet decodes its frame into its piece of `staging` (staging_bytes long: a packet whose piece
 *              does not lie inside it is not decoded and reported CORRUPT); verify != 0 checks the block and content
 *              checksums the frame carries.  What it finds joins the packets' status words, reported by _count.
 *   _count     staged != 0: `src` is the staging buffer of _decode; 0: `src` is the file and the payloads are raw flatbuffers.
 *              Walks each payload's flatbuffer down to the event vector's count.  count_status device i64 [6] <- [n_events, status,
 *              t of the first event, 0, 0, 0]; n_events = 0 unless status is 0.  Read back; allocate the columns.
 *   _unpack    src as given to _count.  The structs -> t (minus the first t when rebase != 0), x, y, p = (on != 0).  Adds to
 *              count_status [3] n_backward (events whose t is below their predecessor's) and [4] n_out_of_range (x outside [0, w)
 *              or y outside [0, h); sets SCPOSE_AEDAT4_RANGE).  Writes nothing unless status was 0 and n_events <= capacity
 *              (else SCPOSE_AEDAT4_CAPACITY).  Read count_status back once more for the counters.
 *   file       device u8, the recording; packets: device i64 [n_packets][2], (payload offset in file, payload size), each payload
 *              inside the file -- the caller's duty, the kernels check every read against the payload only
 *   status     SCPOSE_AEDAT4_CORRUPT: a frame with a wrong magic, version, reserved bit, block maximum or HC, a dictionary id, a
 *              block or sequence that overruns its input, an offset of 0 or before the start of the output (of the block, when
 *              blocks are independent), a block that decodes past its maximum, a content size that differs, a packet that decodes
 *              to more than 2^23 - 16 bytes (the sizes are rounded up to 16 and 256 of them summed in an int32).  _CHECKSUM: a block or content checksum differs.  _FLATBUFFER: no "EVTS" identifier, or a step of
 *              the walk leaves the payload, or 2^23 events or more in one packet.  The kernels detect and never interpret.
 *   workspace  caller-owned, 16-byte aligned, scpose_events_aedat4_workspace_bytes(n_packets) (never 0), the SAME for all four calls
 * Argument errors (null pointers, n_packets < 0 or above 2^31 - 1, h or w outside 1 .. 32767, a misaligned or short workspace)
 * return -1 with a message before anything is launched.  No allocation, no synchronisation, no atomics on the columns, integer
 * work only; two runs on the same bytes give bitwise equal outputs. */
enum { SCPOSE_AEDAT4_CORRUPT = 1, SCPOSE_AEDAT4_CHECKSUM = 2, SCPOSE_AEDAT4_FLATBUFFER = 4, SCPOSE_AEDAT4_RANGE = 8,
       SCPOSE_AEDAT4_CAPACITY = 16 };
int32_t scpose_events_aedat4_workspace_bytes(int64_t n_packets, size_t* bytes);
int32_t scpose_events_aedat4_measure(const uint8_t* file, const int64_t* packets, int64_t n_packets, int64_t* total_status,
                                     void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat4_decode(const uint8_t* file, const int64_t* packets, int64_t n_packets, uint8_t* staging,
                                    int64_t staging_bytes, int32_t verify, void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat4_count(const uint8_t* src, const int64_t* packets, int64_t n_packets, int32_t staged,
                                   int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat4_unpack(const uint8_t* src, int64_t n_packets, int32_t h, int32_t w, int32_t rebase, int64_t* t, int32_t* x,
                                    int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* (ABI 7, additive) ZSTD / ZSTD_HIGH payloads (csrc/events_aedat4_zstd.hip, which states the format: RFC 8878, no dictionary): the
 * Zstandard counterpart of _measure and _decode, with their argument lists, their total_status, their per-packet slots and their
 * limit of 2^23 - 16 decoded bytes per packet, so _count (staged != 0) and _unpack follow unchanged on the SAME workspace.
 *   workspace  scpose_events_aedat4_zstd_workspace_bytes(n_packets): the workspace of the four calls above, its slots in
 *              their places, then one 128 KiB slot per workgroup for a block's regenerated literals.
 *   _zstd_measure  walks frames and blocks without storing: Frame_Content_Size where a frame states it, else Raw and RLE sizes from
 *              the block headers and Compressed ones from the literals header plus the sum of the match lengths.
 *   _zstd_decode   decodes every payload into its piece of `staging`; verify != 0 checks the content checksum (the low 32 bits of
 *              XXH64) of the frames that carry one.
 *   status     SCPOSE_AEDAT4_CORRUPT: a magic that is neither a Zstandard nor a skippable frame's, no Zstandard frame at all, the
 *              reserved bit, a dictionary ID, block type 3, a size above min(window, 128 KiB), a block, table or bitstream that
 *              overruns its input or does not end where it must, an accuracy above its limit, probabilities or Huffman weights
 *              that do not add up to a power of two, Treeless or Repeat with nothing before it, an offset of 0, beyond the window
 *              or before the frame's output, literals that run out, a size that differs from Frame_Content_Size or from
 *              _zstd_measure.  SCPOSE_AEDAT4_CHECKSUM: a content checksum differs.
 * Argument errors as above, under the names events_aedat4_zstd_*.  No allocation, no synchronisation, integer work only; two
 * runs on the same bytes give bitwise equal outputs. */
int32_t scpose_events_aedat4_zstd_workspace_bytes(int64_t n_packets, size_t* bytes);
int32_t scpose_events_aedat4_zstd_measure(const uint8_t* file, const int64_t* packets, int64_t n_packets, int64_t* total_status,
                                          void* workspace, size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat4_zstd_decode(const uint8_t* file, const int64_t* packets, int64_t n_packets, uint8_t* staging,
                                         int64_t staging_bytes, int32_t verify, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) The event packets of an AEDAT-4.0 recording, written on the device (csrc/events_aedat4_write.hip, which states
 * what is written): the four columns and the packets' row boundaries -> the byte string `int32 streamID, int32 size, payload` of
 * every packet, one after the other, as it stands in the file between the IOHeader and the file data table.  The host writes the
 * rest (event_write.write_events_aedat4).
 *   compression  SCPOSE_AEDAT4_NONE: a payload is the packet's size-prefixed "EVTS" flatbuffer, 48 + 16 * count bytes.
 *                SCPOSE_AEDAT4_LZ4: one LZ4 frame of it -- independent blocks of 64 KiB, content checksum, no content size, no block
 *                checksums; a block that does not compress is stored.  Valid LZ4, not liblz4's bytes.
 *   bounds       device i64 [n_packets + 1], rows: packet k holds rows bounds[k] .. bounds[k + 1] - 1; bounds[0] = 0, bounds[n_packets]
 *                = n, never decreasing (checked on the device: SCPOSE_AEDAT4_WRITE_BOUNDS).  An empty packet is written as one.
 *   out          device u8, 8-byte aligned, `capacity` bytes; _pack_sizes gives the capacity that always suffices
 *   table        device i64 [n_packets][5] <- per packet: byte offset of its record in `out`, payload size, events, first and last t
 *   total_status device i64 [2] <- [bytes written, status].  Read back once.  With a status set NOTHING has been stored in `out`
 *                and bytes is unspecified.  SCPOSE_AEDAT4_WRITE_RANGE: some x outside [0, w), y outside [0, h) or p outside {0, 1}.
 *                _SIZE: a packet of more than 2^23 - 1 events or 2^23 - 16 flatbuffer bytes (what the reader takes).  _CAPACITY:
 *                `out` is too small.
 *   workspace    caller-owned, 16-byte aligned, _pack_sizes' workspace_bytes (never 0): under LZ4 the flatbuffers and one slot of
 *                the LZ4 bound per block
 * scpose_events_aedat4_frame makes the same records (streamID 0) of arbitrary bytes: `bounds` (bytes) cuts src into payloads.
 * Argument errors (null pointers, n < 0, n_packets < 0 or above 2^24, packets without events' bounds, h or w outside 1 .. 32767,
 * an unknown compression, a misaligned or short workspace) return -1 with a message before anything is launched.  No allocation,
 * no synchronisation, integer work only; two runs on the same columns give bitwise equal outputs. */
enum { SCPOSE_AEDAT4_NONE = 0, SCPOSE_AEDAT4_LZ4 = 1 };
enum { SCPOSE_AEDAT4_WRITE_RANGE = 1, SCPOSE_AEDAT4_WRITE_SIZE = 2, SCPOSE_AEDAT4_WRITE_BOUNDS = 4, SCPOSE_AEDAT4_WRITE_CAPACITY = 8 };
int32_t scpose_events_aedat4_pack_sizes(int64_t n, int64_t n_packets, int32_t compression, size_t* workspace_bytes, size_t* out_bytes);
int32_t scpose_events_aedat4_pack(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                  const int64_t* bounds, int64_t n_packets, int32_t h, int32_t w, int32_t stream_id, int32_t compression,
                                  uint8_t* out, int64_t capacity, int64_t* table, int64_t* total_status, void* workspace,
                                  size_t workspace_bytes, void* stream);
int32_t scpose_events_aedat4_frame_sizes(int64_t n_bytes, int64_t n_packets, size_t* workspace_bytes, size_t* out_bytes);
int32_t scpose_events_aedat4_frame(const uint8_t* src, int64_t n_bytes, const int64_t* bounds, int64_t n_packets, uint8_t* out,
                                   int64_t capacity, int64_t* table, int64_t* total_status, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* (ABI 7, additive) Baseline JPEG files on the device (csrc/jpeg_decode.hip): the bytes of N files of one geometry -> (N, H, W, 3)
 * uint8 frames, bit for bit what libjpeg's baseline decoder returns (Huffman decoding, jidctint.c's ISLOW inverse DCT, jdsample.c's
 * fancy h2v2 upsampling, jdcolor.c's YCbCr -> RGB).  Decoded: SOF0, 8 bits, one interleaved scan, one component (SCPOSE_JPEG_GRAY)
 * or YCbCr at 4:4:4 (SCPOSE_JPEG_444) or 4:2:0 (SCPOSE_JPEG_420), any tables, any restart interval, any width and height.  The
 * host walks the markers (jpeg_read.py: parse_jpeg refuses everything else by name) and packs, little endian:
 *   desc         device u8 [n][SCPOSE_JPEG_DESC_BYTES], 8-byte aligned.  Per image: int64 offset of the file in `data`; int32
 *                first row of the image in `segs`, number of restart segments, number of subsequences, restart interval in MCUs
 *                (the whole image when the file has none); zeros up to byte 64; uint16 [3][64] quantisation table of each
 *                component in natural order; from byte 448 six tables of 1424 bytes, component c's DC (2 c) and AC (2 c + 1):
 *                uint16 [512] indexed by the next 9 bits (code length << 8 | symbol, 0: the code is longer), int32 [18]
 *                libjpeg's maxcode, int32 [18] its valoffset, uint8 [256] huffval
 *   segs         device i32 [n_seg_rows][4]: per restart segment the first byte and the end of its raw bytes relative to the
 *                file, the index of its first subsequence inside the image, 0; after an image's segments one closing row whose
 *                third word is the image's number of subsequences.  A segment of L raw bytes has max(1, ceil(L /
 *                SCPOSE_JPEG_SUBSEQ_BYTES)) subsequences.  A row that points outside `data` is treated as an empty segment.
 *   data         device u8 [n_bytes]: the files, one after the other
 *   max_subs     the most subsequences of one image of the batch (an image that claims more gets SCPOSE_JPEG_CORRUPT)
 *   bgr          0: R, G, B order; != 0: B, G, R
 *   max_rounds   1 .. 250 launches of the relaxation that finds the entry state of every subsequence (see the .hip file); an
 *                image for which an entry still changed in the last launch gets SCPOSE_JPEG_NOT_CONVERGED
 *   out          device u8 [n][h][w][3], 4-byte aligned;  y_out  device u8 [n][h][w] <- the luminance plane, or NULL
 *   status       device i32 [n] <- SCPOSE_JPEG_NOT_CONVERGED | SCPOSE_JPEG_CORRUPT | rounds used << 8 (bits 8 .. 15).  CORRUPT:
 *                a restart segment holds more or fewer blocks than the header implies, a code that no table holds, a run past
 *                coefficient 63; next to NOT_CONVERGED the bit says nothing.  The pixels of an image with a status bit set are unspecified; nothing outside the outputs
 *                and the workspace is ever written.
 *   workspace    caller-owned, 256-byte aligned, scpose_jpeg_decode_workspace_bytes(n, h, w, mode, max_subs)
 * No allocation, no synchronisation, no floating point, no atomics but integer ORs into status; two calls on the same bytes give
 * bitwise equal outputs.  Argument errors return -1 with a message before anything is launched. */
enum { SCPOSE_JPEG_GRAY = 0, SCPOSE_JPEG_444 = 1, SCPOSE_JPEG_420 = 2 };
enum { SCPOSE_JPEG_NOT_CONVERGED = 1, SCPOSE_JPEG_CORRUPT = 2 };
#define SCPOSE_JPEG_SUBSEQ_BYTES 128
#define SCPOSE_JPEG_DESC_BYTES 9216
int32_t scpose_jpeg_decode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, size_t* bytes);
int32_t scpose_jpeg_decode(const uint8_t* desc, const int32_t* segs, int64_t n_seg_rows, const uint8_t* data, int64_t n_bytes,
                           int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, int32_t bgr, int32_t max_rounds,
                           uint8_t* out, uint8_t* y_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) Baseline JPEG files -> network crops on the device (csrc/jpeg_decode.hip): crops[i] is, bit for bit, what
 * scpose_crop_warp_roi returns for the window roi_xywh[i] of the frame scpose_jpeg_decode returns for file i -- without that frame.
 * The entropy decoding and the DC sums run on the whole frame (the stream has no entry points); the inverse DCT runs only for the
 * blocks that hold a sample a pixel of the window reads (at 4:2:0 one chroma sample more on each side, clamped at the plane's
 * edge: the reach of the fancy upsampling); every one of the four bilinear taps of a crop pixel is then computed from the sample
 * planes.  A tap outside the frame or outside the window counts as 0, as in scpose_crop_warp_roi.
 *   desc, segs, n_seg_rows, data, n_bytes, n, h, w, mode, max_subs, bgr, max_rounds, status, workspace
 *                as for scpose_jpeg_decode; the workspace is the same scpose_jpeg_decode_workspace_bytes(n, h, w, mode, max_subs)
 *   minv         device f64 [n][6], 8-byte aligned: the inverse affine (crop -> frame) of each image, what scpose_crop_warp_roi takes
 *   roi_xywh     HOST i32 [n][4]: [x0, y0, w, h], a window of the frame that holds every pixel the warp reads (w or h may be 0:
 *                the crop is all zeros).  Read before the call returns: each is checked to lie inside the frame -- it bounds
 *                every sample the crop kernel reads -- and travels to the kernels in their arguments, 128 images per launch
 *   out_h, out_w 1 .. 65535 each
 *   crops        device u8 [n][out_h][out_w][3] <- the crops, channels in the order `bgr` selects.  The crop of an image with a
 *                status bit set is unspecified.
 * No allocation, no synchronisation, no atomics but integer ORs into status; floating point only in the source position of a
 * crop pixel (contraction off, as in scpose_crop_warp); two calls on the same bytes give bitwise equal outputs.  Argument errors
 * return -1 with a message before anything is launched. */
int32_t scpose_jpeg_decode_crop(const uint8_t* desc, const int32_t* segs, int64_t n_seg_rows, const uint8_t* data, int64_t n_bytes,
                                int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, int32_t bgr, int32_t max_rounds,
                                const double* minv, const int32_t* roi_xywh, int32_t out_h, int32_t out_w, uint8_t* crops,
                                int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) PNG files on the device (csrc/png_decode.hip): the image data of N files of one geometry -> (N, H, W, 3) uint8
 * frames, bit for bit what PIL's Image.open(..).convert("RGB") returns.  Decoded: bit depth 8, not interlaced, colour types 0 (gray,
 * replicated into three channels), 2 (RGB), 3 (palette; an index the PLTE chunk does not define is 0, 0, 0), 4 and 6 (alpha dropped,
 * not blended); tRNS is ignored.  The host walks the chunks (png_read.py): the IDAT payloads of an image are joined into one zlib
 * stream, so no chunk boundary reaches the device, and everything else -- Adam7, other bit depths, APNG -- is refused there.
 * The device inflates (stored, fixed and dynamic blocks), sums the Adler-32, undoes the filters 0 .. 4 and expands.  It DETECTS a
 * damaged stream and never interprets one: an image whose status is not 0 is the host decoder's to judge.
 *   desc         HOST u8 [n][SCPOSE_PNG_DESC_BYTES].  Per image: int64 offset of its zlib stream in `data` (a multiple of 4); int64
 *                length of the stream (header bytes, blocks, Adler-32 and whatever follows it); int32 h, w, colour type, channels
 *                (they must be the call's h, w, channels); 8 x int32 0; then the palette, u8 [256][3], zero-padded.  Checked before
 *                anything is launched -- a stream that does not lie inside `data` is an argument error -- and uploaded into the
 *                workspace on `stream`: keep it unchanged until the stream has passed the call
 *   data         device u8 [n_bytes], 4-byte aligned: the streams
 *   n, h, w      images of the call and their size, h and w 1 .. 65535; n = 0: nothing to do
 *   channels     bytes per pixel of a scan line, 1 .. 4 (colour types 0 and 3: 1, 4: 2, 2: 3, 6: 4)
 *   bgr          0: R, G, B; else B, G, R
 *   out          device u8 [n][h][w][3] <- the frames.  The frame of an image with a status bit set is unspecified.
 *   status       device i32 [n] <- 0 or SCPOSE_PNG_CORRUPT (a reserved block type, LEN != ~NLEN, an over-subscribed or incomplete
 *                code set, a repeat code with nothing to repeat or running past HLIT + HDIST, no end-of-block code, bits that are
 *                no code, an invalid length or distance symbol, a distance before the first byte, input that ends before the final
 *                block, fewer bytes than h x (1 + w channels)) | SCPOSE_PNG_CHECKSUM (the Adler-32 of every byte the stream
 *                produced differs from the four bytes behind the final block; not checked when the stream ends inside them) |
 *                SCPOSE_PNG_FILTER (a filter byte above 4; not judged for an image that is CORRUPT, whose scan lines are
 *                incomplete).  More bytes than the image needs is no error: they are decoded and summed, not stored.
 *   workspace    caller-owned, 256-byte aligned, scpose_png_decode_workspace_bytes(n, h, w, channels)
 * No allocation, no synchronisation, no atomics, no floating point; two calls on the same bytes give bitwise equal outputs whatever
 * the workspace held.  No kernel writes outside its image's plane of the workspace, its frame and its status word.  Argument
 * errors return -1 with a message before anything is launched and need no device. */
enum { SCPOSE_PNG_CORRUPT = 1, SCPOSE_PNG_CHECKSUM = 2, SCPOSE_PNG_FILTER = 4 };
#define SCPOSE_PNG_DESC_BYTES 832
int32_t scpose_png_decode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t channels, size_t* bytes);
int32_t scpose_png_decode(const uint8_t* desc, const uint8_t* data, int64_t n_bytes, int32_t n, int32_t h, int32_t w, int32_t channels,
                          int32_t bgr, uint8_t* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) PNG files -> network crops on the device (csrc/png_decode.hip): crops[i] is, bit for bit, what
 * scpose_crop_warp_roi returns for the window roi_xywh[i] of the frame scpose_png_decode returns for file i -- without that frame.
 * The whole stream is inflated and summed (it has no entry points); the filters are undone only down to the window's last row;
 * every one of the four bilinear taps of a crop pixel is fetched from the scan lines through the same expansion.  A tap outside the
 * frame or outside the window counts as 0, as in scpose_crop_warp_roi.
 *   desc, data, n_bytes, n, h, w, channels, bgr, status, workspace   as for scpose_png_decode, the same workspace size
 *   minv         device f64 [n][6], 8-byte aligned: the inverse affine (crop -> frame) of each image, what scpose_crop_warp_roi takes
 *   roi_xywh     HOST i32 [n][4]: [x0, y0, w, h], a window of the frame that holds every pixel the warp reads.  Read before the
 *                call returns: each is checked to lie inside the frame and travels to the kernels in their arguments
 *   out_h, out_w 1 .. 65535 each
 *   crops        device u8 [n][out_h][out_w][3] <- the crops.  The crop of an image with a status bit set is unspecified.
 * Floating point only in the source position of a crop pixel (contraction off, as in scpose_crop_warp). */
int32_t scpose_png_decode_crop(const uint8_t* desc, const uint8_t* data, int64_t n_bytes, int32_t n, int32_t h, int32_t w,
                               int32_t channels, int32_t bgr, const double* minv, const int32_t* roi_xywh, int32_t out_h, int32_t out_w,
                               uint8_t* crops, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) Area resize for shrinking on the device (csrc/resize_area.hip): uint8 frames (F, H, W, C), C = 1 or 3, ->
 * (F, h, w, C), or with gray != 0 and C = 3 -> (F, h, w) by OpenCV's 8-bit rule (4899 R + 9617 G + 1868 B + 8192) >> 14 on the
 * rounded resized channels: what the DVS emulator takes.  The arithmetic is cv2.resize(.., interpolation=INTER_AREA) as
 * resize_area.py restates it; the host builds one table per axis there and the kernel only applies them.
 *   src          device u8 [F][H][W][C]
 *   F, H, W, C   F >= 0 (0: nothing to do); H, W 1 .. 65535; C 1 or 3; H W C < 2^31
 *   dst          device u8 [F][h][w][C], or [F][h][w] when gray != 0 or C = 1
 *   h, w         1 .. H and 1 .. W: no axis grows
 *   gray, bgr    gray != 0: reduce three channels to one; bgr != 0: plane 0 is B and plane 2 is R (else the reverse)
 *   rule         SCPOSE_RESIZE_AREA_WEIGHTED: h = ((0 + p0 a0) + p1 a1) + .. along a source row in tap order, v = b0 h0, + b1 h1, ..
 *                down the rows, every multiply and add one float32 rounding, then round-half-to-even saturated to 0 .. 255.
 *                SCPOSE_RESIZE_AREA_BOX: W = cx w and H = cy h; s = the integer sum of the cx x cy box; (s + 2) >> 2 for 2 x 2, else
 *                float32(s) * float32(1.0f / (cx cy)) rounded the same way; cx cy <= 2^23.  The weights of a box table are not read.
 *   xtab, ytab   HOST i32 [w] and [h] records of SCPOSE_RESIZE_AREA_REC_WORDS words: first source index, tap count (>= 1), then the
 *                float32 bits of the weight of the first tap, of every inner tap and of the last tap (a record with one tap uses the
 *                first, with two the first and the last).  Checked before anything is launched -- every tap must lie inside the
 *                source axis and `first` must not decrease; rule BOX: first = d c and count = c for every d -- and uploaded into the
 *                workspace on `stream`: keep them unchanged until the stream has passed the call
 *   workspace    caller-owned, 256-byte aligned, scpose_resize_area_workspace_bytes(h, w)
 * No allocation, no synchronisation, no atomics; reads nothing outside src[0 .. F H W C) and writes nothing outside dst.  A batch
 * is one launch: more than 2^31 - 1 blocks (strips of 8 x 256 output pixels) is an argument error, and so is every other bad
 * argument: -1 with a message before anything is launched, without a device. */
enum { SCPOSE_RESIZE_AREA_WEIGHTED = 0, SCPOSE_RESIZE_AREA_BOX = 1 };
#define SCPOSE_RESIZE_AREA_REC_WORDS 5
int32_t scpose_resize_area_workspace_bytes(int32_t h, int32_t w, size_t* bytes);
int32_t scpose_resize_area_u8(const uint8_t* src, int32_t F, int32_t H, int32_t W, int32_t C, uint8_t* dst, int32_t h, int32_t w,
                              int32_t gray, int32_t bgr, int32_t rule, const int32_t* xtab, const int32_t* ytab, void* workspace,
                              size_t workspace_bytes, void* stream);

/* (ABI 7, additive) Baseline JPEG encoder on the device (csrc/jpeg_encode.hip): (N, H, W, 3) uint8 RGB frames of one size ->
 * N baseline JPEG byte streams, byte for byte what libjpeg's baseline encoder writes with the standard Huffman tables (PIL's
 * save(quality=q, subsampling=..) with its other defaults): jccolor.c, jcsample.c's h2v2 downsampling, jfdctint.c's forward
 * DCT, jcdctmgr.c's quantiser, jchuff.c's coder, one interleaved scan, no restart interval.  mode: SCPOSE_JPEG_GRAY (one
 * component, Y of the three channels), SCPOSE_JPEG_444 or SCPOSE_JPEG_420.  quality 1 .. 100 scales the standard quantisation
 * tables as jcparam.c does.  The host (jpeg_write.py) supplies
 *   huff         device u32 [4][256], 4-byte aligned: DC luminance, AC luminance, DC chrominance, AC chrominance; per symbol
 *                code | length << 16
 *   header       device u8 [header_bytes] (1 .. 65535): the bytes from SOI up to and including SOS, copied in front of every stream
 *   out          device u8 [capacity]: the streams packed in image order; stream i is out[offsets[i] .. offsets[i + 1])
 *   offsets      device i64 [n + 1], 8-byte aligned; written for every image, whether it fits or not
 *   status       device i32 [n] <- 0, SCPOSE_JPEG_ENC_CAPACITY (offsets[i + 1] > capacity: not one byte of the image is
 *                written; every image behind it has the bit too) or SCPOSE_JPEG_ENC_TABLES (huff is not a Huffman code of at
 *                most 16 bits: the image's bits exceed 1728 per block)
 *   workspace    caller-owned, 256-byte aligned, scpose_jpeg_encode_workspace_bytes(n, h, w, mode)
 * scpose_jpeg_encode_capacity_bytes: n * (header_bytes + 432 * blocks + 2), a capacity no frame content exceeds (at most
 * 16 + 11 bits per coefficient, doubled by byte stuffing, EOI).  Nothing is ever written past out[capacity).  An image is limited
 * to 2^31 / 2800 blocks.  No allocation, no synchronisation, no floating point, integer atomics only; two calls on the same
 * frames give bitwise equal outputs.  Argument errors return -1 with a message before anything is launched. */
enum { SCPOSE_JPEG_ENC_CAPACITY = 1, SCPOSE_JPEG_ENC_TABLES = 2 };
int32_t scpose_jpeg_encode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, size_t* bytes);
int32_t scpose_jpeg_encode_capacity_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, int32_t header_bytes, int64_t* bytes);
int32_t scpose_jpeg_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t mode, int32_t quality, const uint32_t* huff,
                           const uint8_t* header, int32_t header_bytes, uint8_t* out, int64_t capacity, int64_t* offsets,
                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 7, additive) Pose overlay on the device (csrc/jpeg_encode.hip), in place on (N, H, W, 3) uint8 RGB frames: per frame the
 * outline of PIL's ImageDraw.rectangle([x, y, x + w, y + h], outline=(0, 255, 0), width=2), then for every finite point the disc
 * of ImageDraw.ellipse([int(px) - 5, int(py) - 5, int(px) + 5, int(py) + 5], fill=(0, 0, 255)), clipped to the frame.
 *   bboxes       device i32 [n][4]: x, y, w, h with w >= 1 and h >= 2 (PIL draws thinner boxes as lines; not reproduced)
 *   points       device f64 [n][j][2] (8-byte aligned; null when j = 0): a point with a NaN or an infinity is skipped, int()
 *                truncates toward zero */
int32_t scpose_overlay_draw(uint8_t* frames, int32_t n, int32_t h, int32_t w, const int32_t* bboxes, const double* points, int32_t j,
                            void* stream);

/* (ABI 7, additive) DVS emulator core on the device (csrc/dvs_emulator.hip): time-stamped grayscale uint8 frames -> an event
 * stream, in the columns scpose_events_frame_bounds / scpose_events_render take.  Restates EventEmulator._init / generate_events
 * of the reference's v2e/v2ecore/emulator.py (with lin_log, rescale_intensity_frame, low_pass_filter, subtract_leak_current,
 * compute_event_map of emulator_utils.py) bit for bit in float32; shot noise and leak jitter, which draw random numbers every
 * frame, are not part of it.  The per-pixel quantities the reference draws once (thresholds, noise-rate array) are inputs.
 *
 * The state (base_log_frame, lp_log_frame0 / 1, timestamp_mem, t_previous and two planes of scratch) lives in a caller-owned
 * device buffer of scpose_dvs_state_bytes(h, w) bytes, 256-byte aligned.  scpose_dvs_init is the reference's first frame: it
 * only initialises the state.  scpose_dvs_emulate then takes n_frames >= 0 further frames in order and appends their events;
 * a sequence fed in several calls gives bitwise the events of one call.  Per sub-iteration i of a frame the events are all ON
 * pixels in row-major order, then all OFF pixels in row-major order (the reference shuffles each such group, whose stamps are
 * equal).  No allocation, no synchronisation, no floating-point atomic; two runs are bitwise equal.
 *   params        h, w; pos_thres / neg_thres (> 0) used where the matching *_map (device f32 h x w, or null) is null;
 *                 noise_rate_map device f32 h x w or null (1 everywhere), used when leak_rate_hz > 0; cutoff_hz, leak_rate_hz,
 *                 refractory_period_s >= 0 (0: off); lin_log_table device f32 [256], the reference's lin_log of 0 ... 255
 *                 (float64 formula, rounded to 1e-8, then float32); max_iters in [1, 4096]: the most sub-iterations of one
 *                 frame the workspace is sized for, 2 * h * w * max_iters < 2^31
 *   frames        device u8 n_frames x h x w;  t  device f64 [n_frames], seconds, each later than the one before (and than
 *                 the state's), >= 0 and below 2^32 us for the integer column
 *   t_s,t,x,y,p   device f32 / i64 / i32 / i32 / i8, capacity rows each: the reference's float32 stamp, the same in
 *                 microseconds by its h5 rule uint32(float32(t_s) * 1e6), the pixel, and the polarity: ON (the reference's
 *                 +1) is 1, OFF (its -1) is 0
 *   count_status  device i64 [2] <- [n_events, status].  n_events is the number the frames produce even where it exceeds
 *                 capacity; rows at and past capacity are never written.  status is a set of bits:
 *                   SCPOSE_DVS_CAPACITY  n_events > capacity: the first `capacity` rows are valid, the state has advanced
 *                   SCPOSE_DVS_ITERS     a frame needs more than max_iters sub-iterations: that frame and all later ones were
 *                                        not emulated and the state is unusable until the next scpose_dvs_init
 *                   SCPOSE_DVS_TIME      a stamp does not increase (the reference raises ValueError): likewise
 *   workspace     caller-owned, 256-byte aligned, scpose_dvs_workspace_bytes(h, w, n_frames, max_iters) */
enum { SCPOSE_DVS_CAPACITY = 1, SCPOSE_DVS_ITERS = 2, SCPOSE_DVS_TIME = 4 };
typedef struct {
  int32_t h, w;
  float pos_thres, neg_thres;
  const float* pos_thres_map;
  const float* neg_thres_map;
  const float* noise_rate_map;
  const float* lin_log_table;
  double cutoff_hz, leak_rate_hz, refractory_period_s;
  int32_t max_iters;
} scpose_dvs_params;
int32_t scpose_dvs_state_bytes(int32_t h, int32_t w, size_t* bytes);
int32_t scpose_dvs_workspace_bytes(int32_t h, int32_t w, int32_t n_frames, int32_t max_iters, size_t* bytes);
int32_t scpose_dvs_init(void* state, const uint8_t* frame0, double t0, const scpose_dvs_params* params, void* stream);
int32_t scpose_dvs_emulate(void* state, const uint8_t* frames, const double* t, int32_t n_frames, const scpose_dvs_params* params,
                           float* t_s, int64_t* t_us, int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Flip test (cfg.TEST.FLIP_TEST, lib/core/function.py:347-366): out = (a + flip_back(b)) * 0.5 where b
 * is the forward of the x-flipped input; flip_back (lib/utils/transforms.py:15-29) mirrors b in x and
 * swaps the joints of each flip pair; shift != 0 applies the TEST.SHIFT_HEATMAP column shift (:361-363).
 *   a, b, out  device f32 N x J x H x W (out may alias a)
 *   perm       device i32 J: perm[j] = partner joint of j (j itself when unpaired) */
int32_t scpose_flip_merge(const float* a, const float* b, const int32_t* perm, int32_t n, int32_t j,
                          int32_t h, int32_t w, int32_t shift, float* out, void* stream);

/* Ensemble mean of validate_cv (landmark_regression/lib/core/function.py:530-536,
 * tools/test_cv_ensemble.py:84-98): acc = (acc + x) / div over count float32 values.  Call once per
 * additional model with div = 1, and with div = number of models for the last one. */
int32_t scpose_heatmap_accumulate(float* acc, const float* x, float div, int64_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched PnP.  Replaces, per frame, the confidence filter + cv2.solvePnPRansac(...,
 * flags=SOLVEPNP_EPNP, iterationsCount, reprojectionError) + cv2.Rodrigues of
 * pose_estimation/export_predicted_poses_real.py:186-203.  One wavefront per frame, fp64.
 *   kp_xyc     device f32 N x J x 3 (x, y, confidence) -- rows of pred.mat
 *   landmarks  device f64 J x 3, K device f64 3x3 row-major, dist device f64[5] (k1,k2,p1,p2,k3)
 *   conf_thr0 / min_pts / thr_decay / thr_iters: the threshold loop of :188-197
 *              (0.95, 15, 0.8, 100 in the reference)
 *   rot        device f64 N x 9 row-major rotation matrix (= cv2.Rodrigues(rvec)[0])
 *   tvec       device f64 N x 3
 *   rvec       device f64 N x 3 (may be NULL)
 *   status     device i32 N: >=0 number of RANSAC inliers; <0 failure code
 *              (-1: fewer than 4 usable points [the reference raises], -2: RANSAC found no model, -4: the final solve is not
 *              finite [cv2 would return NaN]); every failure writes the identity rotation and a zero translation.
 *              Exactly four usable points: as in OpenCV 3.4, no RANSAC -- the P3P kernel on the first three points, the
 *              fourth picks among its up to four poses (status 4, or -2 when P3P finds none); exactly five: one EPnP.
 * ---------------------------------------------------------------------------------------- */
int32_t scpose_pnp_epnp_ransac(const float* kp_xyc, const double* landmarks, const double* K,
                               const double* dist, int32_t n, int32_t j, double conf_thr0,
                               int32_t min_pts, double thr_decay, int32_t thr_iters,
                               int32_t max_iters, double reproj_err, double confidence,
                               double* rot, double* tvec, double* rvec, int32_t* status,
                               void* stream);
/* (ABI 7) Same solve, one output: rows = device f64 N x 13, row i = [R (9, row-major), t (3), (double)status] of frame i --
 * the record export_predicted_poses_real.py:224-226 builds per frame, laid out as the block a rank all-gathers (SURVEY.md
 * section 8e) and copies to the host, so a step needs no assembly launches between the solve and the collective. */
int32_t scpose_pnp_epnp_ransac_rows(const float* kp_xyc, const double* landmarks, const double* K,
                                    const double* dist, int32_t n, int32_t j, double conf_thr0,
                                    int32_t min_pts, double thr_decay, int32_t thr_iters,
                                    int32_t max_iters, double reproj_err, double confidence,
                                    double* rows, void* stream);
/* (ABI 7, additive) The same solve, then optionally a Levenberg-Marquardt refinement of every solved frame (status > 0) and the
 * final point set as a bit mask -- the `inliers` output of cv2.solvePnPRansac, which export_predicted_poses_real.py:199 unpacks
 * and ignores.  The refinement restates cv2.solvePnPRefineLM from OpenCV's documentation (unpinned against cv2): parameters
 * (rvec, tvec), residuals = projection (pinhole + k1,k2,p1,p2,k3) of the float32-rounded landmark minus the raw float32 image
 * point, over the final fit's points (the RANSAC inliers; all 5 points for n == 5; the 4 points of the P3P branch for n == 4);
 * step (J^T J + lambda diag(J^T J)) d = -J^T r, lambda_0 = 1e-3, / 10 on a cost decrease, * 10 (step rejected) otherwise;
 * stops after refine_iters iterations or once a step with |d| <= FLT_EPSILON |p| has been tried (TermCriteria(EPS + COUNT, 20,
 * FLT_EPSILON)).  The
 * refined cost is never above the starting one; a non-finite refined pose keeps the unrefined one; status is unchanged.
 * Each frame's result is bit-identical whatever the batch size and the frame's position in the batch.
 *   refine_iters  0..100; 0: no refinement -- R / t / rvec / status / rows bit-identical to scpose_pnp_epnp_ransac / _rows
 *   rot, tvec, rvec, status  the per-array outputs of scpose_pnp_epnp_ransac (rvec may be NULL), or all NULL when rows != NULL
 *   rows          device f64 N x 13 as in scpose_pnp_epnp_ransac_rows, or NULL; exactly one of the two output forms is given
 *   inliers       device u64 N or NULL: bit k set = landmark k (landmark order, not compacted order) is in the final point set;
 *                 popcount = status for status > 0, 0 for failed frames */
int32_t scpose_pnp_epnp_ransac_refine(const float* kp_xyc, const double* landmarks, const double* K,
                                      const double* dist, int32_t n, int32_t j, double conf_thr0,
                                      int32_t min_pts, double thr_decay, int32_t thr_iters,
                                      int32_t max_iters, double reproj_err, double confidence,
                                      int32_t refine_iters, double* rot, double* tvec, double* rvec,
                                      int32_t* status, double* rows, uint64_t* inliers, void* stream);

/* ------------------------------------------------------------------------------------------
 * Single-layer entry points (unit-level parity of the kernels the forward is made of).
 * ---------------------------------------------------------------------------------------- */
typedef struct scpose_conv* scpose_conv_t;
/* weight: host f32 OIHW (already BN-folded or plain), bias: host f32[cout] or NULL. */
int32_t scpose_conv_create(const float* weight, const float* bias, int32_t cout, int32_t cin,
                           int32_t ksize, int32_t stride, int32_t dtype, scpose_conv_t* out);
int32_t scpose_conv_destroy(scpose_conv_t c);
/* in/out/residual: blocked 16-bit device tensors; out_nchw_f32 != 0 writes float32 NCHW
 * (cout channels) instead.  y = [relu]( conv(x) + bias [+ residual] ). */
int32_t scpose_conv_forward(scpose_conv_t c, const void* in, int32_t n, int32_t h, int32_t w,
                            const void* residual, int32_t relu, int32_t out_nchw_f32, void* out,
                            void* stream);
/* Fused BasicBlock (pose_hrnet.py:41-57): out = relu(conv2(relu(conv1(x))) + x) in one kernel, for two 3x3 /
 * stride-1 / C -> C convolutions created with scpose_conv_create (C = 32 or 48).  in/out blocked C x h x w.
 * Returns SCPOSE_E_INVALID when the pair is not fusable (then run the two scpose_conv_forward calls). */
int32_t scpose_basic_block_forward(scpose_conv_t conv1, scpose_conv_t conv2, const void* in, int32_t n,
                                   int32_t h, int32_t w, void* out, void* stream);
/* out = relu(sum_t upsample_nearest(term_t, 2^shift_t)); all blocked, out is c x h x w. */
int32_t scpose_fuse_sum(const void* const* terms, const int32_t* shifts, int32_t nterms,
                        int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype, void* out,
                        void* stream);
/* The two pose_resnet layers of conv_gather.hip.  y = [relu]( layer(x) + bias [+ residual] ), blocked 16-bit in and out.
 * deconv: ConvTranspose2d(cin -> cout, k in {4, 3, 2}, stride 2, padding / output_padding of _get_deconv_cfg), out 2h x 2w;
 *         weight is host f32 in ConvTranspose2d's own order (cin, cout, k, k).
 * conv1x1s2: Conv2d(cin -> cout, 1x1, stride 2), out ceil(h/2) x ceil(w/2); weight host f32 (cout, cin).
 * cin, cout multiples of 16; bias host f32[cout] or NULL. */
typedef struct scpose_gather* scpose_gather_t;
int32_t scpose_deconv_create(const float* weight, const float* bias, int32_t cin, int32_t cout, int32_t ksize, int32_t dtype,
                             scpose_gather_t* out);
int32_t scpose_conv1x1s2_create(const float* weight, const float* bias, int32_t cout, int32_t cin, int32_t dtype,
                                scpose_gather_t* out);
int32_t scpose_gather_destroy(scpose_gather_t g);
int32_t scpose_gather_forward(scpose_gather_t g, const void* in, int32_t n, int32_t h, int32_t w, const void* residual,
                              int32_t relu, void* out, void* stream);
/* ResNet stem (resnet_stem.hip): relu(conv 7x7 s2 p3 (3 -> 64) + bias) -> max-pool 3x3 s2 p1, one launch.  weight: host f32
 * (64, 3, 7, 7), BN-folded or plain; bias: host f32[64]; mean_std: host f32[6] (SCPOSE_IN_U8_NHWC) or NULL; in: device,
 * uint8 NHWC or float32 NCHW; out: device, blocked 16-bit 64 x h/4 x w/4.  A unit-test entry point, not for a hot path: every call
 * packs and uploads the weights, synchronises the stream and frees them again (the network's own stem does none of that). */
int32_t scpose_resnet_stem_forward(const float* weight, const float* bias, const float* mean_std, const void* in, int32_t in_fmt,
                                   int32_t n, int32_t h, int32_t w, int32_t dtype, void* out, void* stream);
/* layout converters: float32 NCHW <-> blocked 16-bit (c multiple of 8). */
int32_t scpose_nchw_f32_to_blocked(const float* src, int32_t n, int32_t c, int32_t h, int32_t w,
                                   int32_t dtype, void* dst, void* stream);
int32_t scpose_blocked_to_nchw_f32(const void* src, int32_t n, int32_t c, int32_t h, int32_t w,
                                   int32_t dtype, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCPOSE_H */
