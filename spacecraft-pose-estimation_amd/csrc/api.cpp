// extern "C" surface (include/scpose.h) over the kernels: decode, PnP, single-layer entry points.
// The HRNet entry points live next to the plan in hrnet.cpp.
#include "jpeg_common.h"
#include <new>

using namespace scpose;

static bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// The caller's workspace: there, at least `need` bytes and, where the entry point asks for one, on an `align`-byte boundary.
static int32_t workspace_ok(const char* who, const void* workspace, size_t workspace_bytes, size_t need, int align = 0) {
  SCP_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %zu bytes needed (got %zu)", who, need,
              workspace ? workspace_bytes : (size_t)0);
  SCP_REQUIRE(!align || aligned(workspace, align), "%s: workspace must be %d-byte aligned", who, align);
  return SCPOSE_OK;
}

struct scpose_conv { PackedConv pc; };

extern "C" int32_t scpose_abi_version(void) { return SCPOSE_ABI_VERSION; }
extern "C" int32_t scpose_is_dev_build(void) { return scpose::kDevBuild ? 1 : 0; }
extern "C" const char* scpose_last_error(void) { return last_error(); }

extern "C" int32_t scpose_decode(const float* heatmaps, int32_t n, int32_t j, int32_t h, int32_t w,
                                 const float* center, const float* scale, int32_t post_process,
                                 float* preds_xyc, void* stream) {
  if (n == 0) return SCPOSE_OK;  /* empty batch: nothing to do, pointers may be null */
  SCP_REQUIRE(heatmaps && preds_xyc, "decode: null argument");
  return decode_launch(heatmaps, n, j, h, w, center, scale, post_process, preds_xyc, nullptr,
                       nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_crop_warp(const uint8_t* frames, const int64_t* offsets, const int32_t* frame_hw,
                                    const double* minv, int32_t n, int32_t out_h, int32_t out_w, int32_t swap_rb,
                                    uint8_t* crops, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(frames && offsets && frame_hw && minv && crops, "crop_warp: null argument");
  SCP_REQUIRE(out_h > 0 && out_w > 0, "crop_warp: bad output size %dx%d", out_h, out_w);
  return crop_warp_launch(frames, offsets, frame_hw, minv, n, out_h, out_w, swap_rb, crops,
                          static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_crop_warp_roi(const uint8_t* windows, const int64_t* offsets, const int32_t* frame_hw, const int32_t* roi_xywh,
                                        const double* minv, int32_t n, int32_t out_h, int32_t out_w, int32_t swap_rb,
                                        uint8_t* crops, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(windows && offsets && frame_hw && roi_xywh && minv && crops, "crop_warp_roi: null argument");
  SCP_REQUIRE(out_h > 0 && out_w > 0, "crop_warp_roi: bad output size %dx%d", out_h, out_w);
  return crop_warp_launch(windows, offsets, frame_hw, minv, n, out_h, out_w, swap_rb, crops,
                          static_cast<hipStream_t>(stream), roi_xywh);
}

static int32_t events_shape_ok(int32_t f, int32_t h, int32_t w) {
  SCP_REQUIRE(f >= 0, "events: F=%d", f);
  SCP_REQUIRE(h > 0 && w > 0 && h <= 32767 && w <= 32767 && w <= events_max_width() && (int64_t)h * w <= (1 << 24),
              "events: frame %dx%d (HxW) not supported: 1..32767 each, W <= %d, H*W <= 2^24", h, w, events_max_width());
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_workspace_bytes(int32_t n_frames, int32_t h, int32_t w, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_workspace_bytes: null argument");
  const int32_t rc = events_shape_ok(n_frames, h, w);
  if (rc != SCPOSE_OK) return rc;
  *bytes = (size_t)n_frames * h * w;      // the gray plane the undistortion pass samples
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_frame_bounds(const int64_t* t, int64_t n_events, const double* starts, int32_t n_frames,
                                              int64_t* bounds, void* stream) {
  SCP_REQUIRE(n_frames >= 0 && n_events >= 0, "events_frame_bounds: F=%d n_events=%lld", n_frames, (long long)n_events);
  if (n_frames == 0) return SCPOSE_OK;
  SCP_REQUIRE(starts && bounds && (t || n_events == 0), "events_frame_bounds: null argument");
  return events_frame_bounds_launch(t, n_events, starts, n_frames, bounds, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_render(const int32_t* x, const int32_t* y, const void* p, int32_t p_itemsize,
                                        const int64_t* bounds, int32_t n_frames, int32_t h, int32_t w, int32_t full_scale,
                                        int32_t fold_polarity, const uint8_t* gray_lut, const double* K, const double* dist,
                                        uint8_t* frames, uint8_t* distorted, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  // argument errors are reported before the F == 0 return, so that they can be checked without a device
  const int32_t rc = events_shape_ok(n_frames, h, w);
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(full_scale >= 1 && full_scale <= 127, "events_render: full_scale=%d (1..127)", full_scale);
  SCP_REQUIRE(fold_polarity || p_itemsize == 1 || p_itemsize == 4, "events_render: p_itemsize=%d (1: int8, 4: int32)", p_itemsize);
  SCP_REQUIRE((K == nullptr) == (dist == nullptr), "events_render: give K and dist together, or neither (no undistortion)");
  if (n_frames == 0) return SCPOSE_OK;
  SCP_REQUIRE(x && y && bounds && gray_lut && frames && (fold_polarity || p), "events_render: null argument");
  SCP_REQUIRE(!K || (workspace && workspace_bytes >= (size_t)n_frames * h * w),
              "events_render: undistortion needs a workspace of scpose_events_workspace_bytes() = %zu bytes (got %zu)",
              (size_t)n_frames * h * w, workspace ? workspace_bytes : (size_t)0);
  return events_render_launch(x, y, p, p_itemsize, bounds, n_frames, h, w, full_scale, fold_polarity, gray_lut, K, dist, frames,
                              distorted, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static const int64_t kMaxExposureEvents = 2147483647;      // indices are int32 inside the AREA_COUNT kernels

extern "C" int32_t scpose_events_count_frames(int64_t n_events, int64_t count, int64_t* n_frames) {
  SCP_REQUIRE(n_frames, "events_count_frames: null argument");
  SCP_REQUIRE(count >= 1, "events_count_frames: count=%lld: COUNT exposure needs at least 1 event per frame", (long long)count);
  SCP_REQUIRE(n_events >= 0, "events_count_frames: n_events=%lld", (long long)n_events);
  *n_frames = n_events >= 2 ? (n_events - 2) / count : 0;   // frame k is written while (k + 1) * count < n - 1
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_count_bounds(int64_t n_events, int64_t count, int64_t n_frames, int64_t* bounds, void* stream) {
  int64_t f = 0;
  const int32_t rc = scpose_events_count_frames(n_events, count, &f);
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(n_frames >= 0 && n_frames <= f, "events_count_bounds: n_frames=%lld, the stream holds %lld COUNT frames",
              (long long)n_frames, (long long)f);
  if (n_frames == 0) return SCPOSE_OK;
  SCP_REQUIRE(bounds, "events_count_bounds: null argument");
  return events_count_bounds_launch(count, n_frames, bounds, static_cast<hipStream_t>(stream));
}

static int32_t area_args_ok(int64_t n, int64_t M, int32_t D, int32_t h, int32_t w) {
  const int32_t rc = events_shape_ok(0, h, w);
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(n >= 0 && n <= kMaxExposureEvents, "events_area_bounds: n_events=%lld (0 .. 2^31 - 1)", (long long)n);
  SCP_REQUIRE(M >= 2, "events_area_bounds: area_count=%lld: an area must receive at least 2 events (the reference never ends "
              "a frame below that)", (long long)M);
  SCP_REQUIRE(D >= 1, "events_area_bounds: area_dimension=%d (>= 1)", D);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_area_bounds_workspace_bytes(int64_t n_events, int64_t area_count, int32_t area_dimension, int32_t h,
                                                            int32_t w, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_area_bounds_workspace_bytes: null argument");
  const int32_t rc = area_args_ok(n_events, area_count, area_dimension, h, w);
  if (rc != SCPOSE_OK) return rc;
  *bytes = events_area_workspace_bytes(n_events, area_count, area_dimension, h, w);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_area_bounds(const int32_t* x, const int32_t* y, int64_t n_events, int64_t area_count,
                                             int32_t area_dimension, int32_t h, int32_t w, int64_t* bounds, int64_t capacity,
                                             int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  const int32_t rc = area_args_ok(n_events, area_count, area_dimension, h, w);
  if (rc != SCPOSE_OK) return rc;
  const int64_t fcap = n_events >= 2 ? (n_events - 2) / (area_count - 1) : 0;
  SCP_REQUIRE(capacity >= fcap, "events_area_bounds: capacity=%lld < (n_events - 2) / (area_count - 1) = %lld",
              (long long)capacity, (long long)fcap);
  if (int32_t rc = workspace_ok("events_area_bounds", workspace, workspace_bytes,
                                events_area_workspace_bytes(n_events, area_count, area_dimension, h, w)))
    return rc;
  SCP_REQUIRE(count_status && (bounds || fcap == 0) && ((x && y) || n_events == 0), "events_area_bounds: null argument");
  return events_area_bounds_launch(x, y, n_events, area_count, area_dimension, h, w, bounds, capacity, count_status,
                                   static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_bounds_midpoints(const int64_t* t, const int64_t* bounds, int64_t n_frames, double* mids,
                                                  void* stream) {
  SCP_REQUIRE(n_frames >= 0, "events_bounds_midpoints: n_frames=%lld", (long long)n_frames);
  if (n_frames == 0) return SCPOSE_OK;
  SCP_REQUIRE(t && bounds && mids, "events_bounds_midpoints: null argument");
  return events_bounds_midpoints_launch(t, bounds, n_frames, mids, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_csv_workspace_bytes(int64_t n_bytes, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_csv_workspace_bytes: null argument");
  SCP_REQUIRE(n_bytes >= 0, "events_csv_workspace_bytes: n_bytes=%lld", (long long)n_bytes);
  *bytes = events_csv_workspace_bytes(n_bytes);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_csv_parse(const uint8_t* data, int64_t n_bytes, int32_t delim_whitespace, int32_t swap_xy,
                                           double t_divisor, int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity,
                                           int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(n_bytes >= 0 && capacity >= 0, "events_csv_parse: n_bytes=%lld capacity=%lld", (long long)n_bytes, (long long)capacity);
  SCP_REQUIRE(t_divisor >= 0.0 && t_divisor <= 1e300, "events_csv_parse: t_divisor=%g (0: none, else a positive divisor)", t_divisor);
  SCP_REQUIRE(count_status && (data || n_bytes == 0) && ((t && x && y && p) || capacity == 0), "events_csv_parse: null argument");
  SCP_REQUIRE(aligned(data, 16), "events_csv_parse: data must be 16-byte aligned");
  SCP_REQUIRE(aligned(workspace, 16), "events_csv_parse: workspace must be 16-byte aligned");      // reported before its size here
  if (int32_t rc = workspace_ok("events_csv_parse", workspace, workspace_bytes, events_csv_workspace_bytes(n_bytes))) return rc;
  return events_csv_parse_launch(data, n_bytes, delim_whitespace != 0, swap_xy != 0, t_divisor, t, x, y, p, capacity, count_status,
                                 static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static const int64_t kMaxWriteEvents = (int64_t)1 << 38;      // one workgroup per 256 events, the grid below 2^31

static int32_t text_args_ok(const char* who, const void* t, const void* x, const void* y, const void* p, int64_t n,
                            const int64_t* count_status, const void* workspace, size_t workspace_bytes) {
  SCP_REQUIRE(n >= 0 && n <= kMaxWriteEvents, "%s: n=%lld (0 .. 2^38)", who, (long long)n);
  SCP_REQUIRE(count_status && ((t && x && y && p) || n == 0), "%s: null argument", who);
  return workspace_ok(who, workspace, workspace_bytes, events_text_workspace_bytes(n), 16);
}

extern "C" int32_t scpose_events_text_tiling(int32_t* tile_rows, int32_t* scan_rows) {
  SCP_REQUIRE(tile_rows && scan_rows, "events_text_tiling: null argument");
  *tile_rows = events_text_tile_rows();
  *scan_rows = events_text_scan_rows();
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_text_workspace_bytes(int64_t n, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_text_workspace_bytes: null argument");
  SCP_REQUIRE(n >= 0 && n <= kMaxWriteEvents, "events_text_workspace_bytes: n=%lld (0 .. 2^38)", (long long)n);
  *bytes = events_text_workspace_bytes(n);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_text_measure(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                              int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  const int32_t rc = text_args_ok("events_text_measure", t, x, y, p, n, count_status, workspace, workspace_bytes);
  if (rc != SCPOSE_OK) return rc;
  return events_text_measure_launch(t, x, y, p, n, count_status, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_text_emit(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                           int32_t sep, int32_t swap_xy, uint8_t* out, int64_t capacity, int64_t* count_status,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(sep == ' ' || sep == ',', "events_text_emit: sep=%d: the separator is ' ' (32) or ',' (44)", sep);
  SCP_REQUIRE(capacity >= 0, "events_text_emit: capacity=%lld", (long long)capacity);
  const int32_t rc = text_args_ok("events_text_emit", t, x, y, p, n, count_status, workspace, workspace_bytes);
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(out || capacity == 0, "events_text_emit: null argument");
  SCP_REQUIRE(aligned(out, 16), "events_text_emit: out must be 16-byte aligned");
  return events_text_emit_launch(t, x, y, p, n, sep, swap_xy != 0, out, capacity, count_status, static_cast<uint8_t*>(workspace),
                                 static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_aedat2_pack(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                             int32_t h, int32_t w, uint8_t* out, int64_t* count_status, void* stream) {
  // y has the 10 bits above bit 22; x starts at bit 12, and the reference's widest sensor (1280) already reaches into bit 22
  SCP_REQUIRE(h >= 1 && h <= 1024 && w >= 1 && w <= 1280, "events_aedat2_pack: frame %dx%d (HxW) not supported: H 1 .. 1024, "
              "W 1 .. 1280", h, w);
  SCP_REQUIRE(n >= 0 && n <= kMaxWriteEvents, "events_aedat2_pack: n=%lld (0 .. 2^38)", (long long)n);
  SCP_REQUIRE(count_status && ((t && x && y && p && out) || n == 0), "events_aedat2_pack: null argument");
  SCP_REQUIRE(aligned(out, 8), "events_aedat2_pack: out must be 8-byte aligned");
  return events_aedat2_pack_launch(t, x, y, p, n, h, w, out, count_status, static_cast<hipStream_t>(stream));
}

static const int64_t kMaxReadRecords = (int64_t)1 << 38;      // 2 TiB of records; the tile index is negated in an int32

extern "C" int32_t scpose_events_aedat2_unpack_workspace_bytes(int64_t n_records, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_aedat2_unpack_workspace_bytes: null argument");
  SCP_REQUIRE(n_records >= 0 && n_records <= kMaxReadRecords, "events_aedat2_unpack_workspace_bytes: n_records=%lld (0 .. 2^38)",
              (long long)n_records);
  *bytes = events_aedat2_unpack_workspace_bytes(n_records);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat2_unpack(const uint8_t* records, int64_t n_records, int32_t h, int32_t w, int32_t layout,
                                               int32_t flip_x, int32_t flip_y, int32_t unwrap, double t_divisor, int64_t* t, int32_t* x,
                                               int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(layout == SCPOSE_AEDAT2_LAYOUT_DAVIS || layout == SCPOSE_AEDAT2_LAYOUT_V2E,
              "events_aedat2_unpack: layout=%d: the layouts are 0 (DAVIS) and 1 (V2E)", layout);
  // x has the 10 bits from bit 12; y the 9 bits from bit 22 below the DAVIS type bit, or all 10 as the V2E writer uses them
  const int32_t max_h = layout == SCPOSE_AEDAT2_LAYOUT_DAVIS ? 512 : 1024;
  SCP_REQUIRE(h >= 1 && h <= max_h && w >= 1 && w <= 1024,
              "events_aedat2_unpack: frame %dx%d (HxW) not supported under the %s layout: H 1 .. %d, W 1 .. 1024%s", h, w,
              layout == SCPOSE_AEDAT2_LAYOUT_DAVIS ? "DAVIS" : "V2E", max_h,
              w > 1024 && w <= 1280 ? " (the 1280x720 writer ORs bit 10 of x into bit 0 of y: the word cannot be inverted)" : "");
  SCP_REQUIRE(n_records >= 0 && n_records <= kMaxReadRecords, "events_aedat2_unpack: n_records=%lld (0 .. 2^38)", (long long)n_records);
  SCP_REQUIRE(capacity >= 0, "events_aedat2_unpack: capacity=%lld", (long long)capacity);
  SCP_REQUIRE(t_divisor == 0.0 || t_divisor == 1e3 || t_divisor == 1e6, "events_aedat2_unpack: t_divisor=%g (0: none, 1e3 or 1e6)",
              t_divisor);
  SCP_REQUIRE(count_status && (n_records == 0 || (records && ((t && x && y && p) || capacity == 0))),
              "events_aedat2_unpack: null argument");
  SCP_REQUIRE(aligned(records, 8), "events_aedat2_unpack: records must be 8-byte aligned");
  if (int32_t rc = workspace_ok("events_aedat2_unpack", workspace, workspace_bytes, events_aedat2_unpack_workspace_bytes(n_records), 16))
    return rc;
  return events_aedat2_unpack_launch(records, n_records, h, w, layout, flip_x != 0, flip_y != 0, unwrap != 0, t_divisor, t, x, y, p,
                                     capacity, count_status, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

// n_packets in range, the workspace, then the pointers: the file and the descriptors are needed when there are packets
static int32_t aedat3_args_ok(const char* who, int64_t n_packets, const void* file, const void* packets, const void* count_status,
                              const void* workspace, size_t workspace_bytes) {
  SCP_REQUIRE(n_packets >= 0 && n_packets <= 0x7fffffff, "%s: n_packets=%lld (0 .. 2^31 - 1)", who, (long long)n_packets);
  if (int32_t rc = workspace_ok(who, workspace, workspace_bytes, events_aedat3_workspace_bytes(n_packets), 16)) return rc;
  SCP_REQUIRE(count_status && (n_packets == 0 || (file && packets)), "%s: null argument", who);
  SCP_REQUIRE(aligned(packets, 8) && aligned(count_status, 8), "%s: packets and count_status must be 8-byte aligned", who);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat3_workspace_bytes(int64_t n_packets, size_t* bytes) {
  SCP_REQUIRE(bytes, "events_aedat3_workspace_bytes: null argument");
  SCP_REQUIRE(n_packets >= 0 && n_packets <= 0x7fffffff, "events_aedat3_workspace_bytes: n_packets=%lld (0 .. 2^31 - 1)",
              (long long)n_packets);
  *bytes = events_aedat3_workspace_bytes(n_packets);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat3_count(const uint8_t* file, const int64_t* packets, int64_t n_packets, int64_t* count_status,
                                              void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = aedat3_args_ok("events_aedat3_count", n_packets, file, packets, count_status, workspace, workspace_bytes)) return rc;
  return events_aedat3_count_launch(file, packets, n_packets, count_status, static_cast<uint8_t*>(workspace),
                                    static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_aedat3_unpack(const uint8_t* file, const int64_t* packets, int64_t n_packets, int32_t h, int32_t w,
                                               int32_t rebase, int64_t* t, int32_t* x, int32_t* y, int8_t* p, int64_t capacity,
                                               int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  // x and y are 15-bit fields
  SCP_REQUIRE(h >= 1 && h <= 32768 && w >= 1 && w <= 32768, "events_aedat3_unpack: sensor %dx%d (HxW) not supported: each 1 .. 32768",
              h, w);
  SCP_REQUIRE(capacity >= 0, "events_aedat3_unpack: capacity=%lld", (long long)capacity);
  SCP_REQUIRE((t && x && y && p) || capacity == 0, "events_aedat3_unpack: null argument");
  if (int32_t rc = aedat3_args_ok("events_aedat3_unpack", n_packets, file, packets, count_status, workspace, workspace_bytes)) return rc;
  return events_aedat3_unpack_launch(file, packets, n_packets, h, w, rebase != 0, t, x, y, p, capacity, count_status,
                                     static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

// n_packets in range, the workspace, then the pointers: `a` and `b` are needed when there are packets, `result` always.
// zstd: the call belongs to the ZSTD pair, whose workspace is the larger one.
static int32_t aedat4_args_ok(const char* who, int64_t n_packets, const void* a, const void* b, const void* result,
                              const void* workspace, size_t workspace_bytes, bool zstd = false) {
  SCP_REQUIRE(n_packets >= 0 && n_packets <= 0x7fffffff, "%s: n_packets=%lld (0 .. 2^31 - 1)", who, (long long)n_packets);
  const size_t need = zstd ? events_aedat4_zstd_workspace_bytes(n_packets) : events_aedat4_workspace_bytes(n_packets);
  if (int32_t rc = workspace_ok(who, workspace, workspace_bytes, need, 16)) return rc;
  SCP_REQUIRE(result && (n_packets == 0 || (a && b)), "%s: null argument", who);
  return SCPOSE_OK;
}

// The workspace query, MEASURE and DECODE exist once per payload codec (LZ4, ZSTD): one body each, and `who` and `zstd` say which
// entry point runs it.  DECODE's kernels store nothing past a packet's measured size and nothing outside staging_bytes.
static int32_t aedat4_workspace_query(const char* who, int64_t n_packets, size_t* bytes, bool zstd) {
  SCP_REQUIRE(bytes, "%s: null argument", who);
  SCP_REQUIRE(n_packets >= 0 && n_packets <= 0x7fffffff, "%s: n_packets=%lld (0 .. 2^31 - 1)", who, (long long)n_packets);
  *bytes = zstd ? events_aedat4_zstd_workspace_bytes(n_packets) : events_aedat4_workspace_bytes(n_packets);
  return SCPOSE_OK;
}

static int32_t aedat4_measure(const char* who, bool zstd, const uint8_t* file, const int64_t* packets, int64_t n_packets,
                              int64_t* total_status, void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = aedat4_args_ok(who, n_packets, file, packets, total_status, workspace, workspace_bytes, zstd)) return rc;
  return (zstd ? events_aedat4_zstd_measure_launch : events_aedat4_measure_launch)(
      file, packets, n_packets, total_status, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static int32_t aedat4_decode(const char* who, bool zstd, const uint8_t* file, const int64_t* packets, int64_t n_packets,
                             uint8_t* staging, int64_t staging_bytes, int32_t verify, void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = aedat4_args_ok(who, n_packets, file, packets, workspace, workspace, workspace_bytes, zstd)) return rc;
  SCP_REQUIRE(staging_bytes >= 0 && (staging || staging_bytes == 0), "%s: staging of %lld bytes%s", who, (long long)staging_bytes,
              staging ? "" : " is null");
  SCP_REQUIRE(aligned(staging, 16), "%s: staging must be 16-byte aligned", who);
  return (zstd ? events_aedat4_zstd_decode_launch : events_aedat4_decode_launch)(
      file, packets, n_packets, staging, staging_bytes, verify != 0, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_aedat4_workspace_bytes(int64_t n_packets, size_t* bytes) {
  return aedat4_workspace_query("events_aedat4_workspace_bytes", n_packets, bytes, false);
}
extern "C" int32_t scpose_events_aedat4_zstd_workspace_bytes(int64_t n_packets, size_t* bytes) {
  return aedat4_workspace_query("events_aedat4_zstd_workspace_bytes", n_packets, bytes, true);
}

extern "C" int32_t scpose_events_aedat4_measure(const uint8_t* file, const int64_t* packets, int64_t n_packets, int64_t* total_status,
                                                void* workspace, size_t workspace_bytes, void* stream) {
  return aedat4_measure("events_aedat4_measure", false, file, packets, n_packets, total_status, workspace, workspace_bytes, stream);
}
extern "C" int32_t scpose_events_aedat4_zstd_measure(const uint8_t* file, const int64_t* packets, int64_t n_packets,
                                                     int64_t* total_status, void* workspace, size_t workspace_bytes, void* stream) {
  return aedat4_measure("events_aedat4_zstd_measure", true, file, packets, n_packets, total_status, workspace, workspace_bytes, stream);
}

extern "C" int32_t scpose_events_aedat4_decode(const uint8_t* file, const int64_t* packets, int64_t n_packets, uint8_t* staging,
                                               int64_t staging_bytes, int32_t verify, void* workspace, size_t workspace_bytes,
                                               void* stream) {
  return aedat4_decode("events_aedat4_decode", false, file, packets, n_packets, staging, staging_bytes, verify, workspace,
                       workspace_bytes, stream);
}
extern "C" int32_t scpose_events_aedat4_zstd_decode(const uint8_t* file, const int64_t* packets, int64_t n_packets, uint8_t* staging,
                                                    int64_t staging_bytes, int32_t verify, void* workspace, size_t workspace_bytes,
                                                    void* stream) {
  return aedat4_decode("events_aedat4_zstd_decode", true, file, packets, n_packets, staging, staging_bytes, verify, workspace,
                       workspace_bytes, stream);
}

extern "C" int32_t scpose_events_aedat4_count(const uint8_t* src, const int64_t* packets, int64_t n_packets, int32_t staged,
                                              int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = aedat4_args_ok("events_aedat4_count", n_packets, src, staged ? static_cast<const void*>(src) : packets, count_status,
                                  workspace, workspace_bytes))
    return rc;
  return events_aedat4_count_launch(src, packets, n_packets, staged != 0, count_status, static_cast<uint8_t*>(workspace),
                                    static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_events_aedat4_unpack(const uint8_t* src, int64_t n_packets, int32_t h, int32_t w, int32_t rebase, int64_t* t,
                                               int32_t* x, int32_t* y, int8_t* p, int64_t capacity, int64_t* count_status,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, "events_aedat4_unpack: sensor %dx%d (HxW) not supported: each 1 .. 32767",
              h, w);
  SCP_REQUIRE(capacity >= 0, "events_aedat4_unpack: capacity=%lld", (long long)capacity);
  SCP_REQUIRE((t && x && y && p) || capacity == 0, "events_aedat4_unpack: null argument");
  if (int32_t rc = aedat4_args_ok("events_aedat4_unpack", n_packets, src, src, count_status, workspace, workspace_bytes))
    return rc;
  return events_aedat4_unpack_launch(src, n_packets, h, w, rebase != 0, t, x, y, p, capacity, count_status,
                                     static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static const int64_t kMaxWritePackets = (int64_t)1 << 24;     // one wavefront per packet and per block in one grid

static int32_t aedat4_pack_shape_ok(const char* who, int64_t n, int64_t n_packets, int32_t compression) {
  SCP_REQUIRE(n >= 0 && n <= kMaxWriteEvents, "%s: n=%lld (0 .. 2^38)", who, (long long)n);
  SCP_REQUIRE(n_packets >= 0 && n_packets <= kMaxWritePackets, "%s: n_packets=%lld (0 .. 2^24)", who, (long long)n_packets);
  SCP_REQUIRE(n == 0 || n_packets > 0, "%s: n=%lld events in no packet", who, (long long)n);
  SCP_REQUIRE(compression == SCPOSE_AEDAT4_NONE || compression == SCPOSE_AEDAT4_LZ4,
              "%s: compression=%d: the compressions are 0 (NONE) and 1 (LZ4)", who, compression);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat4_pack_sizes(int64_t n, int64_t n_packets, int32_t compression, size_t* workspace_bytes,
                                                   size_t* out_bytes) {
  SCP_REQUIRE(workspace_bytes && out_bytes, "events_aedat4_pack_sizes: null argument");
  if (int32_t rc = aedat4_pack_shape_ok("events_aedat4_pack_sizes", n, n_packets, compression)) return rc;
  const Aedat4WriteSizes s = events_aedat4_pack_sizes(n, n_packets, compression);
  *workspace_bytes = s.workspace_bytes;
  *out_bytes = s.out_bytes;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat4_pack(const int64_t* t, const int32_t* x, const int32_t* y, const int8_t* p, int64_t n,
                                             const int64_t* bounds, int64_t n_packets, int32_t h, int32_t w, int32_t stream_id,
                                             int32_t compression, uint8_t* out, int64_t capacity, int64_t* table, int64_t* total_status,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(h >= 1 && h <= 32767 && w >= 1 && w <= 32767, "events_aedat4_pack: sensor %dx%d (HxW) not supported: each 1 .. 32767",
              h, w);
  if (int32_t rc = aedat4_pack_shape_ok("events_aedat4_pack", n, n_packets, compression)) return rc;
  SCP_REQUIRE(capacity >= 0, "events_aedat4_pack: capacity=%lld", (long long)capacity);
  SCP_REQUIRE(total_status && ((t && x && y && p) || n == 0) && ((bounds && table) || n_packets == 0) && (out || capacity == 0),
              "events_aedat4_pack: null argument");
  SCP_REQUIRE(aligned(out, 8) && aligned(bounds, 8) && aligned(table, 8) && aligned(total_status, 8),
              "events_aedat4_pack: out, bounds, table and total_status must be 8-byte aligned");
  if (int32_t rc = workspace_ok("events_aedat4_pack", workspace, workspace_bytes,
                                events_aedat4_pack_sizes(n, n_packets, compression).workspace_bytes, 16))
    return rc;
  return events_aedat4_pack_launch(t, x, y, p, n, bounds, n_packets, h, w, stream_id, compression, out, capacity, table, total_status,
                                   static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static int32_t aedat4_frame_shape_ok(const char* who, int64_t n_bytes, int64_t n_packets) {
  SCP_REQUIRE(n_bytes >= 0 && n_bytes <= ((int64_t)1 << 42), "%s: n_bytes=%lld (0 .. 2^42)", who, (long long)n_bytes);
  SCP_REQUIRE(n_packets >= 0 && n_packets <= kMaxWritePackets, "%s: n_packets=%lld (0 .. 2^24)", who, (long long)n_packets);
  SCP_REQUIRE(n_bytes == 0 || n_packets > 0, "%s: n_bytes=%lld in no packet", who, (long long)n_bytes);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat4_frame_sizes(int64_t n_bytes, int64_t n_packets, size_t* workspace_bytes, size_t* out_bytes) {
  SCP_REQUIRE(workspace_bytes && out_bytes, "events_aedat4_frame_sizes: null argument");
  if (int32_t rc = aedat4_frame_shape_ok("events_aedat4_frame_sizes", n_bytes, n_packets)) return rc;
  const Aedat4WriteSizes s = events_aedat4_frame_sizes(n_bytes, n_packets);
  *workspace_bytes = s.workspace_bytes;
  *out_bytes = s.out_bytes;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_events_aedat4_frame(const uint8_t* src, int64_t n_bytes, const int64_t* bounds, int64_t n_packets, uint8_t* out,
                                              int64_t capacity, int64_t* table, int64_t* total_status, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  if (int32_t rc = aedat4_frame_shape_ok("events_aedat4_frame", n_bytes, n_packets)) return rc;
  SCP_REQUIRE(capacity >= 0, "events_aedat4_frame: capacity=%lld", (long long)capacity);
  SCP_REQUIRE(total_status && (src || n_bytes == 0) && ((bounds && table) || n_packets == 0) && (out || capacity == 0),
              "events_aedat4_frame: null argument");
  SCP_REQUIRE(aligned(bounds, 8) && aligned(table, 8) && aligned(total_status, 8),
              "events_aedat4_frame: bounds, table and total_status must be 8-byte aligned");
  if (int32_t rc = workspace_ok("events_aedat4_frame", workspace, workspace_bytes,
                                events_aedat4_frame_sizes(n_bytes, n_packets).workspace_bytes, 16))
    return rc;
  return events_aedat4_frame_launch(src, n_bytes, bounds, n_packets, out, capacity, table, total_status,
                                    static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

// what the decoder, the encoder and the overlay draw ask of a batch of frames
static int32_t frames_ok(const char* who, int32_t n, int32_t h, int32_t w) {
  SCP_REQUIRE(n >= 1 && n <= 65535, "%s: n=%d (1 .. 65535)", who, n);
  SCP_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: frame %dx%d (HxW), each 1 .. 65535", who, h, w);
  return SCPOSE_OK;
}

static int32_t jpeg_frame_ok(const char* who, int32_t n, int32_t h, int32_t w, int32_t mode) {
  SCP_REQUIRE(mode == SCPOSE_JPEG_GRAY || mode == SCPOSE_JPEG_444 || mode == SCPOSE_JPEG_420,
              "%s: mode=%d: the modes are 0 (gray), 1 (4:4:4) and 2 (4:2:0)", who, mode);
  return frames_ok(who, n, h, w);
}

static int32_t jpeg_check_shape(int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, const char* who) {
  if (int32_t rc = jpeg_frame_ok(who, n, h, w, mode)) return rc;
  SCP_REQUIRE(max_subs >= 1 && max_subs <= (1 << 24), "%s: max_subs=%d (1 .. 2^24)", who, max_subs);
  SCP_REQUIRE((int64_t)n * jpeg_blocks(h, w, mode) < ((int64_t)1 << 31) && (int64_t)n * max_subs < ((int64_t)1 << 31),
              "%s: n * blocks and n * max_subs must stay below 2^31: decode the batch in parts", who);
  return SCPOSE_OK;
}

// What both *_decode_crop entry points ask of the crops and of the windows; each one's own sentences fire between the two checks.
static int32_t crop_size_ok(const char* who, int32_t out_h, int32_t out_w) {
  SCP_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= 65535 && out_w <= 65535, "%s: bad output size %dx%d (each 1 .. 65535)", who, out_h, out_w);
  return SCPOSE_OK;
}
static int32_t crop_rois_ok(const char* who, int32_t n, int32_t h, int32_t w, const int32_t* roi_xywh) {
  for (int32_t i = 0; i < n; ++i) {      // roi_xywh is host memory: the window bounds everything the crop kernel reads
    const int32_t* r = roi_xywh + 4 * (size_t)i;
    SCP_REQUIRE(r[0] >= 0 && r[1] >= 0 && r[2] >= 0 && r[3] >= 0 && (int64_t)r[0] + r[2] <= w && (int64_t)r[1] + r[3] <= h,
                "%s: roi %d = [%d, %d, %d, %d] (x, y, w, h) is not inside the %dx%d (HxW) frame", who, i, r[0], r[1], r[2], r[3], h, w);
  }
  return SCPOSE_OK;
}

extern "C" int32_t scpose_jpeg_decode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, size_t* bytes) {
  SCP_REQUIRE(bytes, "jpeg_decode_workspace_bytes: null argument");
  if (int32_t rc = jpeg_check_shape(n, h, w, mode, max_subs, "jpeg_decode_workspace_bytes")) return rc;
  *bytes = jpeg_decode_workspace_bytes(n, h, w, mode, max_subs);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_jpeg_decode(const uint8_t* desc, const int32_t* segs, int64_t n_seg_rows, const uint8_t* data, int64_t n_bytes,
                                      int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, int32_t bgr, int32_t max_rounds,
                                      uint8_t* out, uint8_t* y_out, int32_t* status, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (int32_t rc = jpeg_check_shape(n, h, w, mode, max_subs, "jpeg_decode")) return rc;
  SCP_REQUIRE(max_rounds >= 1 && max_rounds <= 250, "jpeg_decode: max_rounds=%d (1 .. 250)", max_rounds);
  SCP_REQUIRE(n_seg_rows >= 2 * (int64_t)n && n_seg_rows < ((int64_t)1 << 31) && n_bytes >= 0, "jpeg_decode: n_seg_rows=%lld n_bytes=%lld",
              (long long)n_seg_rows, (long long)n_bytes);
  SCP_REQUIRE(desc && segs && (data || n_bytes == 0) && out && status, "jpeg_decode: null argument");
  SCP_REQUIRE(aligned(desc, 8) && aligned(segs, 4) && aligned(out, 4) && aligned(y_out, 4) && aligned(status, 4),
              "jpeg_decode: desc must be 8-byte aligned, segs, out, y_out and status 4-byte aligned");
  if (int32_t rc = workspace_ok("jpeg_decode", workspace, workspace_bytes, jpeg_decode_workspace_bytes(n, h, w, mode, max_subs), 256))
    return rc;
  return jpeg_decode_launch(desc, segs, n_seg_rows, data, n_bytes, n, h, w, mode, max_subs, bgr != 0, max_rounds, out, y_out, status,
                            static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_jpeg_decode_crop(const uint8_t* desc, const int32_t* segs, int64_t n_seg_rows, const uint8_t* data, int64_t n_bytes,
                                           int32_t n, int32_t h, int32_t w, int32_t mode, int32_t max_subs, int32_t bgr, int32_t max_rounds,
                                           const double* minv, const int32_t* roi_xywh, int32_t out_h, int32_t out_w, uint8_t* crops,
                                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = jpeg_check_shape(n, h, w, mode, max_subs, "jpeg_decode_crop")) return rc;
  SCP_REQUIRE(max_rounds >= 1 && max_rounds <= 250, "jpeg_decode_crop: max_rounds=%d (1 .. 250)", max_rounds);
  SCP_REQUIRE(n_seg_rows >= 2 * (int64_t)n && n_seg_rows < ((int64_t)1 << 31) && n_bytes >= 0, "jpeg_decode_crop: n_seg_rows=%lld n_bytes=%lld",
              (long long)n_seg_rows, (long long)n_bytes);
  if (int32_t rc = crop_size_ok("jpeg_decode_crop", out_h, out_w)) return rc;
  SCP_REQUIRE(desc && segs && (data || n_bytes == 0) && minv && roi_xywh && crops && status, "jpeg_decode_crop: null argument");
  SCP_REQUIRE(aligned(desc, 8) && aligned(minv, 8) && aligned(segs, 4) && aligned(status, 4),
              "jpeg_decode_crop: desc and minv must be 8-byte aligned, segs and status 4-byte aligned");
  if (int32_t rc = crop_rois_ok("jpeg_decode_crop", n, h, w, roi_xywh)) return rc;
  if (int32_t rc = workspace_ok("jpeg_decode_crop", workspace, workspace_bytes, jpeg_decode_workspace_bytes(n, h, w, mode, max_subs), 256))
    return rc;
  return jpeg_decode_crop_launch(desc, segs, n_seg_rows, data, n_bytes, n, h, w, mode, max_subs, bgr != 0, max_rounds, minv, roi_xywh, out_h,
                                 out_w, crops, status, static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static int32_t png_check_shape(const char* who, int32_t n, int32_t h, int32_t w, int32_t channels) {
  SCP_REQUIRE(n >= 0 && n <= 65535, "%s: n=%d (0 .. 65535)", who, n);      // an empty batch has a workspace size too
  if (int32_t rc = frames_ok(who, n ? n : 1, h, w)) return rc;
  SCP_REQUIRE(channels >= 1 && channels <= 4, "%s: channels=%d (1 .. 4)", who, channels);
  return SCPOSE_OK;
}

// the descriptors are host memory: every stream must lie inside `data` and every image must have the call's geometry
static int32_t png_check_desc(const char* who, const uint8_t* desc, int64_t n_bytes, int32_t n, int32_t h, int32_t w, int32_t channels) {
  for (int32_t i = 0; i < n; ++i) {
    int64_t q[2];
    int32_t v[4];
    memcpy(q, desc + (size_t)i * SCPOSE_PNG_DESC_BYTES, sizeof q);
    memcpy(v, desc + (size_t)i * SCPOSE_PNG_DESC_BYTES + 16, sizeof v);
    SCP_REQUIRE(q[0] >= 0 && q[1] >= 0 && (q[0] & 3) == 0 && q[0] <= n_bytes && q[1] <= n_bytes - q[0],
                "%s: descriptor %d: the stream [%lld, +%lld) does not lie inside the %lld bytes of data on a 4-byte boundary", who, i,
                (long long)q[0], (long long)q[1], (long long)n_bytes);
    SCP_REQUIRE(v[0] == h && v[1] == w && v[3] == channels, "%s: descriptor %d is of a %dx%d frame with %d channels, the call of %dx%d with %d",
                who, i, v[0], v[1], v[3], h, w, channels);
    SCP_REQUIRE(v[2] == 0 || v[2] == 2 || v[2] == 3 || v[2] == 4 || v[2] == 6, "%s: descriptor %d: colour type %d", who, i, v[2]);
  }
  return SCPOSE_OK;
}

extern "C" int32_t scpose_png_decode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t channels, size_t* bytes) {
  SCP_REQUIRE(bytes, "png_decode_workspace_bytes: null argument");
  if (int32_t rc = png_check_shape("png_decode_workspace_bytes", n, h, w, channels)) return rc;
  *bytes = png_decode_workspace_bytes(n, h, w, channels);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_png_decode(const uint8_t* desc, const uint8_t* data, int64_t n_bytes, int32_t n, int32_t h, int32_t w,
                                     int32_t channels, int32_t bgr, uint8_t* out, int32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (n == 0) return SCPOSE_OK;
  if (int32_t rc = png_check_shape("png_decode", n, h, w, channels)) return rc;
  SCP_REQUIRE(desc && (data || n_bytes == 0) && out && status && n_bytes >= 0, "png_decode: null argument");
  SCP_REQUIRE(aligned(data, 4) && aligned(status, 4), "png_decode: data and status must be 4-byte aligned");
  if (int32_t rc = png_check_desc("png_decode", desc, n_bytes, n, h, w, channels)) return rc;
  if (int32_t rc = workspace_ok("png_decode", workspace, workspace_bytes, png_decode_workspace_bytes(n, h, w, channels), 256)) return rc;
  return png_decode_launch(desc, data, n, h, w, channels, bgr != 0, out, status, static_cast<uint8_t*>(workspace),
                           static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_png_decode_crop(const uint8_t* desc, const uint8_t* data, int64_t n_bytes, int32_t n, int32_t h, int32_t w,
                                          int32_t channels, int32_t bgr, const double* minv, const int32_t* roi_xywh, int32_t out_h,
                                          int32_t out_w, uint8_t* crops, int32_t* status, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  if (n == 0) return SCPOSE_OK;
  if (int32_t rc = png_check_shape("png_decode_crop", n, h, w, channels)) return rc;
  if (int32_t rc = crop_size_ok("png_decode_crop", out_h, out_w)) return rc;
  SCP_REQUIRE(desc && (data || n_bytes == 0) && minv && roi_xywh && crops && status && n_bytes >= 0, "png_decode_crop: null argument");
  SCP_REQUIRE(aligned(data, 4) && aligned(status, 4) && aligned(minv, 8),
              "png_decode_crop: data and status must be 4-byte aligned, minv 8-byte aligned");
  if (int32_t rc = png_check_desc("png_decode_crop", desc, n_bytes, n, h, w, channels)) return rc;
  if (int32_t rc = crop_rois_ok("png_decode_crop", n, h, w, roi_xywh)) return rc;
  if (int32_t rc = workspace_ok("png_decode_crop", workspace, workspace_bytes, png_decode_workspace_bytes(n, h, w, channels), 256))
    return rc;
  return png_decode_crop_launch(desc, data, n, h, w, channels, bgr != 0, minv, roi_xywh, out_h, out_w, crops, status,
                                static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

static int32_t resize_area_check_tab(const char* axis, const int32_t* tab, int32_t n_out, int32_t n_in, bool box) {
  const int32_t c = n_in / n_out;
  int32_t prev = 0;
  for (int32_t d = 0; d < n_out; ++d) {
    const int32_t first = tab[(size_t)d * SCPOSE_RESIZE_AREA_REC_WORDS], count = tab[(size_t)d * SCPOSE_RESIZE_AREA_REC_WORDS + 1];
    SCP_REQUIRE(first >= prev && count >= 1 && first < n_in && count <= n_in - first,
                "resize_area: %s table, record %d: taps [%d, +%d) do not lie inside 0 .. %d in increasing order", axis, d, first, count, n_in);
    SCP_REQUIRE(!box || (first == d * c && count == c), "resize_area: %s table, record %d: a box table has taps [%d, +%d) there (got [%d, +%d))",
                axis, d, d * c, c, first, count);
    prev = first;
  }
  return SCPOSE_OK;
}

extern "C" int32_t scpose_resize_area_workspace_bytes(int32_t h, int32_t w, size_t* bytes) {
  SCP_REQUIRE(bytes, "resize_area_workspace_bytes: null argument");
  SCP_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "resize_area_workspace_bytes: output size %dx%d (HxW), 1 .. 65535 each", h, w);
  *bytes = resize_area_workspace_bytes(h, w);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_resize_area_u8(const uint8_t* src, int32_t F, int32_t H, int32_t W, int32_t C, uint8_t* dst, int32_t h, int32_t w,
                                         int32_t gray, int32_t bgr, int32_t rule, const int32_t* xtab, const int32_t* ytab, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  SCP_REQUIRE(F >= 0, "resize_area: F=%d", F);
  if (F == 0) return SCPOSE_OK;
  SCP_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "resize_area: frame %dx%d (HxW), 1 .. 65535 each", H, W);
  SCP_REQUIRE(C == 1 || C == 3, "resize_area: channels=%d (1 or 3)", C);
  SCP_REQUIRE((int64_t)H * W * C < ((int64_t)1 << 31), "resize_area: frame %dx%dx%d: one frame must stay below 2^31 bytes", H, W, C);
  SCP_REQUIRE(h >= 1 && w >= 1 && h <= H && w <= W, "resize_area: output size %dx%d (HxW) of a %dx%d frame: no axis may grow", h, w, H, W);
  SCP_REQUIRE(rule == SCPOSE_RESIZE_AREA_WEIGHTED || rule == SCPOSE_RESIZE_AREA_BOX, "resize_area: rule=%d", rule);
  const bool box = rule == SCPOSE_RESIZE_AREA_BOX;
  SCP_REQUIRE(!box || (H % h == 0 && W % w == 0 && (int64_t)(H / h) * (W / w) <= (1 << 23)),
              "resize_area: the box rule needs whole ratios with at most 2^23 pixels per box (%dx%d -> %dx%d)", H, W, h, w);
  SCP_REQUIRE(src && dst && xtab && ytab, "resize_area: null argument");
  if (int32_t rc = resize_area_check_tab("x", xtab, w, W, box)) return rc;
  if (int32_t rc = resize_area_check_tab("y", ytab, h, H, box)) return rc;
  if (int32_t rc = workspace_ok("resize_area", workspace, workspace_bytes, resize_area_workspace_bytes(h, w), 256)) return rc;
  return resize_area_launch(src, F, H, W, C, dst, h, w, gray != 0, bgr != 0, box, xtab, ytab, static_cast<uint8_t*>(workspace),
                            static_cast<hipStream_t>(stream));
}

static int32_t jpeg_encode_check_shape(int32_t n, int32_t h, int32_t w, int32_t mode, const char* who) {
  if (int32_t rc = jpeg_frame_ok(who, n, h, w, mode)) return rc;
  SCP_REQUIRE(jpeg_blocks(h, w, mode) * 2800 < ((int64_t)1 << 31),
              "%s: frame %dx%d (HxW): the bits of one image must stay below 2^31 (blocks * 2800)", who, h, w);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_jpeg_encode_workspace_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, size_t* bytes) {
  SCP_REQUIRE(bytes, "jpeg_encode_workspace_bytes: null argument");
  if (int32_t rc = jpeg_encode_check_shape(n, h, w, mode, "jpeg_encode_workspace_bytes")) return rc;
  *bytes = jpeg_encode_workspace_bytes(n, h, w, mode);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_jpeg_encode_capacity_bytes(int32_t n, int32_t h, int32_t w, int32_t mode, int32_t header_bytes, int64_t* bytes) {
  SCP_REQUIRE(bytes, "jpeg_encode_capacity_bytes: null argument");
  if (int32_t rc = jpeg_encode_check_shape(n, h, w, mode, "jpeg_encode_capacity_bytes")) return rc;
  SCP_REQUIRE(header_bytes >= 1 && header_bytes <= 65535, "jpeg_encode_capacity_bytes: header_bytes=%d (1 .. 65535)", header_bytes);
  *bytes = jpeg_encode_capacity_bytes(n, h, w, mode, header_bytes);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_jpeg_encode(const uint8_t* frames, int32_t n, int32_t h, int32_t w, int32_t mode, int32_t quality,
                                      const uint32_t* huff, const uint8_t* header, int32_t header_bytes, uint8_t* out, int64_t capacity,
                                      int64_t* offsets, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (int32_t rc = jpeg_encode_check_shape(n, h, w, mode, "jpeg_encode")) return rc;
  SCP_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality=%d (1 .. 100)", quality);
  SCP_REQUIRE(header_bytes >= 1 && header_bytes <= 65535, "jpeg_encode: header_bytes=%d (1 .. 65535)", header_bytes);
  SCP_REQUIRE(capacity >= 0, "jpeg_encode: capacity=%lld", (long long)capacity);
  SCP_REQUIRE(frames && huff && header && (out || capacity == 0) && offsets && status, "jpeg_encode: null argument");
  SCP_REQUIRE(aligned(huff, 4) && aligned(offsets, 8) && aligned(status, 4),
              "jpeg_encode: huff and status must be 4-byte aligned, offsets 8-byte aligned");
  if (int32_t rc = workspace_ok("jpeg_encode", workspace, workspace_bytes, jpeg_encode_workspace_bytes(n, h, w, mode), 256)) return rc;
  return jpeg_encode_launch(frames, n, h, w, mode, quality, huff, header, header_bytes, out, capacity, offsets, status,
                            static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_overlay_draw(uint8_t* frames, int32_t n, int32_t h, int32_t w, const int32_t* bboxes, const double* points,
                                       int32_t j, void* stream) {
  if (int32_t rc = frames_ok("overlay_draw", n, h, w)) return rc;
  SCP_REQUIRE(j >= 0 && j <= 65535, "overlay_draw: j=%d (0 .. 65535)", j);
  SCP_REQUIRE(frames && bboxes && (points || j == 0), "overlay_draw: null argument");
  SCP_REQUIRE(aligned(bboxes, 4) && aligned(points, 8),
              "overlay_draw: bboxes must be 4-byte aligned, points 8-byte aligned");
  return overlay_draw_launch(frames, n, h, w, bboxes, points, j, static_cast<hipStream_t>(stream));
}

static int32_t dvs_check_params(const scpose_dvs_params* p, const char* who) {
  SCP_REQUIRE(p, "%s: null params", who);
  SCP_REQUIRE(p->h > 0 && p->w > 0 && (int64_t)p->h * p->w <= (1 << 24), "%s: bad shape h=%d w=%d", who, p->h, p->w);
  SCP_REQUIRE((p->pos_thres_map || p->pos_thres > 0.f) && (p->neg_thres_map || p->neg_thres > 0.f),
              "%s: thresholds must be > 0 (pos_thres=%g neg_thres=%g)", who, (double)p->pos_thres, (double)p->neg_thres);
  SCP_REQUIRE(p->cutoff_hz >= 0.0 && p->leak_rate_hz >= 0.0 && p->refractory_period_s >= 0.0 && p->cutoff_hz <= 1e300 &&
                  p->leak_rate_hz <= 1e300 && p->refractory_period_s <= 1e300,
              "%s: cutoff_hz=%g leak_rate_hz=%g refractory_period_s=%g must be finite and >= 0", who, p->cutoff_hz, p->leak_rate_hz,
              p->refractory_period_s);
  SCP_REQUIRE(p->lin_log_table, "%s: null lin_log_table", who);
  SCP_REQUIRE(p->max_iters >= 1 && p->max_iters <= 4096 && 2 * (int64_t)p->h * p->w * p->max_iters < ((int64_t)1 << 31),
              "%s: max_iters=%d (1 ... 4096, and 2 * h * w * max_iters < 2^31)", who, p->max_iters);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_dvs_state_bytes(int32_t h, int32_t w, size_t* bytes) {
  SCP_REQUIRE(bytes, "dvs_state_bytes: null argument");
  SCP_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= (1 << 24), "dvs_state_bytes: bad shape h=%d w=%d", h, w);
  *bytes = dvs_state_bytes(h, w);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_dvs_workspace_bytes(int32_t h, int32_t w, int32_t n_frames, int32_t max_iters, size_t* bytes) {
  SCP_REQUIRE(bytes, "dvs_workspace_bytes: null argument");
  SCP_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= (1 << 24) && n_frames >= 0, "dvs_workspace_bytes: bad shape h=%d w=%d n_frames=%d", h,
              w, n_frames);
  SCP_REQUIRE(max_iters >= 1 && max_iters <= 4096 && 2 * (int64_t)h * w * max_iters < ((int64_t)1 << 31),
              "dvs_workspace_bytes: max_iters=%d (1 ... 4096, and 2 * h * w * max_iters < 2^31)", max_iters);
  *bytes = dvs_workspace_bytes(h, w, n_frames, max_iters);
  return SCPOSE_OK;
}

extern "C" int32_t scpose_dvs_init(void* state, const uint8_t* frame0, double t0, const scpose_dvs_params* params, void* stream) {
  const int32_t rc = dvs_check_params(params, "dvs_init");
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(state && frame0, "dvs_init: null argument");
  SCP_REQUIRE(aligned(state, 256), "dvs_init: state must be 256-byte aligned");
  SCP_REQUIRE(t0 == t0 && t0 >= -1e300 && t0 <= 1e300, "dvs_init: t0=%g", t0);
  return dvs_init_launch(state, frame0, t0, params->h, params->w, params->lin_log_table, params->refractory_period_s,
                         static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_dvs_emulate(void* state, const uint8_t* frames, const double* t, int32_t n_frames,
                                      const scpose_dvs_params* params, float* t_s, int64_t* t_us, int32_t* x, int32_t* y, int8_t* p,
                                      int64_t capacity, int64_t* count_status, void* workspace, size_t workspace_bytes, void* stream) {
  const int32_t rc = dvs_check_params(params, "dvs_emulate");
  if (rc != SCPOSE_OK) return rc;
  SCP_REQUIRE(n_frames >= 0 && capacity >= 0, "dvs_emulate: n_frames=%d capacity=%lld", n_frames, (long long)capacity);
  SCP_REQUIRE(state && count_status && ((frames && t) || n_frames == 0) && ((t_s && t_us && x && y && p) || capacity == 0),
              "dvs_emulate: null argument");
  SCP_REQUIRE(aligned(state, 256) && aligned(workspace, 256), "dvs_emulate: state and workspace must be 256-byte aligned");
  if (int32_t rc = workspace_ok("dvs_emulate", workspace, workspace_bytes,
                                dvs_workspace_bytes(params->h, params->w, n_frames, params->max_iters)))
    return rc;
  return dvs_emulate_launch(state, frames, t, n_frames, *params, t_s, t_us, x, y, p, capacity, count_status,
                            static_cast<uint8_t*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_flip_merge(const float* a, const float* b, const int32_t* perm, int32_t n, int32_t j,
                                     int32_t h, int32_t w, int32_t shift, float* out, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(a && b && perm && out, "flip_merge: null argument");
  SCP_REQUIRE(j > 0 && h > 0 && w > 0, "flip_merge: bad shape J=%d H=%d W=%d", j, h, w);
  return flip_merge_launch(a, b, perm, n, j, h, w, shift, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_heatmap_accumulate(float* acc, const float* x, float div, int64_t count, void* stream) {
  if (count == 0) return SCPOSE_OK;
  SCP_REQUIRE(acc && x && count > 0, "heatmap_accumulate: null argument");
  SCP_REQUIRE(div > 0.f, "heatmap_accumulate: div=%f", (double)div);
  return heatmap_accumulate_launch(acc, x, div, (size_t)count, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_max_preds(const float* heatmaps, int32_t n, int32_t j, int32_t h,
                                    int32_t w, float* coords, float* maxvals, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(heatmaps && coords && maxvals, "max_preds: null argument");
  return decode_launch(heatmaps, n, j, h, w, nullptr, nullptr, 0, nullptr, coords, maxvals,
                       static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_pnp_epnp_ransac(const float* kp_xyc, const double* landmarks,
                                          const double* K, const double* dist, int32_t n, int32_t j,
                                          double conf_thr0, int32_t min_pts, double thr_decay,
                                          int32_t thr_iters, int32_t max_iters, double reproj_err,
                                          double confidence, double* rot, double* tvec,
                                          double* rvec, int32_t* status, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(kp_xyc && landmarks && K && rot && tvec && status, "pnp: null argument");
  return pnp_launch(kp_xyc, landmarks, K, dist, n, j, conf_thr0, min_pts, thr_decay, thr_iters,
                    max_iters, reproj_err, confidence, rot, tvec, rvec, status,
                    static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_pnp_epnp_ransac_rows(const float* kp_xyc, const double* landmarks, const double* K,
                                               const double* dist, int32_t n, int32_t j, double conf_thr0,
                                               int32_t min_pts, double thr_decay, int32_t thr_iters,
                                               int32_t max_iters, double reproj_err, double confidence,
                                               double* rows, void* stream) {
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(kp_xyc && landmarks && K && rows, "pnp_rows: null argument");
  return pnp_launch(kp_xyc, landmarks, K, dist, n, j, conf_thr0, min_pts, thr_decay, thr_iters,
                    max_iters, reproj_err, confidence, nullptr, nullptr, nullptr, nullptr,
                    static_cast<hipStream_t>(stream), rows);
}

extern "C" int32_t scpose_pnp_epnp_ransac_refine(const float* kp_xyc, const double* landmarks, const double* K,
                                                 const double* dist, int32_t n, int32_t j, double conf_thr0,
                                                 int32_t min_pts, double thr_decay, int32_t thr_iters,
                                                 int32_t max_iters, double reproj_err, double confidence,
                                                 int32_t refine_iters, double* rot, double* tvec, double* rvec,
                                                 int32_t* status, double* rows, uint64_t* inliers, void* stream) {
  // argument errors are reported before the n == 0 return, so that they can be checked without a device
  SCP_REQUIRE(refine_iters >= 0 && refine_iters <= 100, "pnp_refine: refine_iters=%d (0..100)", refine_iters);
  const bool arrays = rot || tvec || rvec || status;
  SCP_REQUIRE(arrays != (rows != nullptr),
              "pnp_refine: give exactly one output form: rot/tvec/status[/rvec], or rows (with rot/tvec/rvec/status NULL)");
  SCP_REQUIRE(rows || (rot && tvec && status), "pnp_refine: rot, tvec and status are required in the per-array form");
  if (n == 0) return SCPOSE_OK;
  SCP_REQUIRE(kp_xyc && landmarks && K, "pnp_refine: null argument");
  return pnp_launch(kp_xyc, landmarks, K, dist, n, j, conf_thr0, min_pts, thr_decay, thr_iters, max_iters, reproj_err,
                    confidence, rot, tvec, rvec, status, static_cast<hipStream_t>(stream), rows, refine_iters,
                    reinterpret_cast<unsigned long long*>(inliers));
}

extern "C" int32_t scpose_conv_create(const float* weight, const float* bias, int32_t cout,
                                      int32_t cin, int32_t ksize, int32_t stride, int32_t dtype,
                                      scpose_conv_t* out) {
  SCP_REQUIRE(weight && out, "conv_create: null argument");
  scpose_conv* c = new (std::nothrow) scpose_conv();
  if (!c) { set_error("conv_create: out of host memory"); return SCPOSE_E_NOMEM; }
  const int32_t rc = conv_upload(weight, bias, cout, cin, ksize, stride, dtype, &c->pc);
  if (rc != SCPOSE_OK) { conv_free(&c->pc); delete c; return rc; }
  *out = c;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_conv_destroy(scpose_conv_t c) {
  if (!c) return SCPOSE_OK;
  conv_free(&c->pc);
  delete c;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_conv_forward(scpose_conv_t c, const void* in, int32_t n, int32_t h,
                                       int32_t w, const void* residual, int32_t relu,
                                       int32_t out_nchw_f32, void* out, void* stream) {
  SCP_REQUIRE(c && in && out, "conv_forward: null argument");
  return conv_launch(c->pc, in, n, h, w, residual, relu, out_nchw_f32, out,
                     static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_basic_block_forward(scpose_conv_t conv1, scpose_conv_t conv2, const void* in, int32_t n,
                                              int32_t h, int32_t w, void* out, void* stream) {
  SCP_REQUIRE(conv1 && conv2 && in && out, "basic_block_forward: null argument");
  SCP_REQUIRE(block_fusable(conv1->pc, conv2->pc), "basic_block_forward: not a fusable pair (3x3 stride-1 C->C->C, C = 32 or 48)");
  return block_launch(conv1->pc, conv2->pc, in, n, h, w, out, static_cast<hipStream_t>(stream));
}

struct scpose_gather { GatherPacked gp; };

extern "C" int32_t scpose_deconv_create(const float* weight, const float* bias, int32_t cin, int32_t cout, int32_t ksize,
                                        int32_t dtype, scpose_gather_t* out) {
  SCP_REQUIRE(weight && out, "deconv_create: null argument");
  SCP_REQUIRE(cin > 0 && cout > 0 && ksize >= 2 && ksize <= 4, "deconv_create: cin=%d cout=%d kernel=%d", cin, cout, ksize);
  const int kk = ksize * ksize;
  std::vector<float> w((size_t)cout * cin * kk), b(cout, 0.f);   // (cin, cout, k, k) -> (cout, cin, k, k)
  for (int ci = 0; ci < cin; ++ci)
    for (int co = 0; co < cout; ++co)
      for (int t = 0; t < kk; ++t) w[((size_t)co * cin + ci) * kk + t] = weight[((size_t)ci * cout + co) * kk + t];
  if (bias) b.assign(bias, bias + cout);
  scpose_gather* g = new (std::nothrow) scpose_gather();
  if (!g) { set_error("deconv_create: out of host memory"); return SCPOSE_E_NOMEM; }
  const int32_t rc = deconv_upload(w.data(), b.data(), cout, cin, ksize, dtype, &g->gp);
  if (rc != SCPOSE_OK) { gather_free(&g->gp); delete g; return rc; }
  *out = g;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_conv1x1s2_create(const float* weight, const float* bias, int32_t cout, int32_t cin, int32_t dtype,
                                           scpose_gather_t* out) {
  SCP_REQUIRE(weight && out, "conv1x1s2_create: null argument");
  SCP_REQUIRE(cin > 0 && cout > 0, "conv1x1s2_create: cin=%d cout=%d", cin, cout);
  std::vector<float> b(cout, 0.f);
  if (bias) b.assign(bias, bias + cout);
  scpose_gather* g = new (std::nothrow) scpose_gather();
  if (!g) { set_error("conv1x1s2_create: out of host memory"); return SCPOSE_E_NOMEM; }
  const int32_t rc = conv1x1s2_upload(weight, b.data(), cout, cin, dtype, &g->gp);
  if (rc != SCPOSE_OK) { gather_free(&g->gp); delete g; return rc; }
  *out = g;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_gather_destroy(scpose_gather_t g) {
  if (!g) return SCPOSE_OK;
  gather_free(&g->gp);
  delete g;
  return SCPOSE_OK;
}

extern "C" int32_t scpose_gather_forward(scpose_gather_t g, const void* in, int32_t n, int32_t h, int32_t w, const void* residual,
                                         int32_t relu, void* out, void* stream) {
  SCP_REQUIRE(g && in && out, "gather_forward: null argument");
  return gather_launch(g->gp, in, n, h, w, residual, relu, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_resnet_stem_forward(const float* weight, const float* bias, const float* mean_std, const void* in,
                                              int32_t in_fmt, int32_t n, int32_t h, int32_t w, int32_t dtype, void* out, void* stream) {
  SCP_REQUIRE(weight && bias && in && out, "resnet_stem_forward: null argument");
  SCP_REQUIRE(dtype == SCPOSE_DT_BF16 || dtype == SCPOSE_DT_F16, "resnet_stem_forward: dtype %d", dtype);
  SCP_REQUIRE(in_fmt != SCPOSE_IN_U8_NHWC || mean_std, "resnet_stem_forward: u8 input needs mean/std");
  std::vector<uint16_t> pw;
  resnet_stem_pack(weight, dtype, &pw);
  void* d_w = nullptr; float* d_b = nullptr; float* d_ms = nullptr;
  auto release = [&]() { if (d_w) (void)hipFree(d_w); if (d_b) (void)hipFree(d_b); if (d_ms) (void)hipFree(d_ms); };
  int32_t rc = SCPOSE_OK;
  if (hipMalloc(&d_w, pw.size() * 2) != hipSuccess || hipMalloc(&d_b, 64 * 4) != hipSuccess || hipMalloc(&d_ms, 6 * 4) != hipSuccess ||
      hipMemcpy(d_w, pw.data(), pw.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_b, bias, 64 * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (mean_std && hipMemcpy(d_ms, mean_std, 6 * 4, hipMemcpyHostToDevice) != hipSuccess)) {
    set_error("resnet_stem_forward: uploading the weights failed");
    rc = SCPOSE_E_HIP;
  }
  if (rc == SCPOSE_OK) rc = resnet_stem_launch(in, in_fmt, d_w, d_b, mean_std ? d_ms : nullptr, n, h, w, dtype, out, static_cast<hipStream_t>(stream));
  if (rc == SCPOSE_OK && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) {
    set_error("resnet_stem_forward: the launch failed");
    rc = SCPOSE_E_HIP;
  }
  release();
  return rc;
}

extern "C" int32_t scpose_fuse_sum(const void* const* terms, const int32_t* shifts, int32_t nterms,
                                   int32_t n, int32_t c, int32_t h, int32_t w, int32_t dtype,
                                   void* out, void* stream) {
  SCP_REQUIRE(terms && shifts && out, "fuse_sum: null argument");
  return fuse_sum_launch(terms, shifts, nterms, n, c, h, w, dtype, out,
                         static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_nchw_f32_to_blocked(const float* src, int32_t n, int32_t c, int32_t h,
                                              int32_t w, int32_t dtype, void* dst, void* stream) {
  SCP_REQUIRE(src && dst, "nchw_f32_to_blocked: null argument");
  return nchw_to_blocked_launch(src, n, c, h, w, dtype, dst, static_cast<hipStream_t>(stream));
}

extern "C" int32_t scpose_blocked_to_nchw_f32(const void* src, int32_t n, int32_t c, int32_t h,
                                              int32_t w, int32_t dtype, float* dst, void* stream) {
  SCP_REQUIRE(src && dst, "blocked_to_nchw_f32: null argument");
  return blocked_to_nchw_launch(src, n, c, h, w, dtype, dst, static_cast<hipStream_t>(stream));
}
