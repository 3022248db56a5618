"""ctypes binding of libscpose_hip.so (C ABI declared in include/scpose.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If the
shared object is missing or a symbol is absent, importing callers get a RuntimeError.
"""
import ctypes
import os
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libscpose_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
DEV_LIB_PATH = os.path.join(_HERE, "libscpose_hip_dev.so")   # same sources, -DSCPOSE_DEV_BUILD (csrc/Makefile: make dev)
if os.environ.get("SCPOSE_DEV") == "1":
    # developer scripts only (tools_dev/README.md): an explicit build for A/B runs, else the development build -- the
    # only one whose kernels contain the phase stamps and ablation switches -- when it has been built
    if os.environ.get("SCPOSE_LIB"):
        LIB_PATH = os.path.abspath(os.environ["SCPOSE_LIB"])
    elif os.path.exists(DEV_LIB_PATH):
        LIB_PATH = DEV_LIB_PATH

DT_BF16, DT_F16 = 0, 1
IN_F32_NCHW, IN_U8_NHWC = 0, 1
CSV_UNSUPPORTED, CSV_CAPACITY = 1, 2
DVS_CAPACITY, DVS_ITERS, DVS_TIME = 1, 2, 4
TEXT_CAPACITY = 1
AEDAT2_RANGE, AEDAT2_TIME = 1, 2
AEDAT2_LAYOUT_DAVIS, AEDAT2_LAYOUT_V2E = 0, 1
AEDAT2_READ_RANGE, AEDAT2_READ_CAPACITY = 1, 2
AEDAT3_CORRUPT, AEDAT3_VALID_MISMATCH, AEDAT3_RANGE, AEDAT3_CAPACITY = 1, 2, 4, 8
AEDAT4_CORRUPT, AEDAT4_CHECKSUM, AEDAT4_FLATBUFFER, AEDAT4_RANGE, AEDAT4_CAPACITY = 1, 2, 4, 8, 16
AEDAT4_NONE, AEDAT4_LZ4 = 0, 1
AEDAT4_WRITE_RANGE, AEDAT4_WRITE_SIZE, AEDAT4_WRITE_BOUNDS, AEDAT4_WRITE_CAPACITY = 1, 2, 4, 8
JPEG_GRAY, JPEG_444, JPEG_420 = 0, 1, 2
JPEG_NOT_CONVERGED, JPEG_CORRUPT = 1, 2
JPEG_SUBSEQ_BYTES, JPEG_DESC_BYTES = 128, 9216
JPEG_ENC_CAPACITY, JPEG_ENC_TABLES = 1, 2
PNG_CORRUPT, PNG_CHECKSUM, PNG_FILTER = 1, 2, 4
PNG_DESC_BYTES = 832
RESIZE_AREA_WEIGHTED, RESIZE_AREA_BOX = 0, 1
RESIZE_AREA_REC_WORDS = 5
ABI_VERSION = 7


class HrnetDesc(ctypes.Structure):
    _fields_ = [
        ("num_joints", c_int32),
        ("final_conv_kernel", c_int32),
        ("num_stages", c_int32),
        ("num_modules", c_int32 * 3),
        ("num_branches", c_int32 * 3),
        ("num_blocks", (c_int32 * 4) * 3),
        ("num_channels", (c_int32 * 4) * 3),
        ("dtype", c_int32),
        ("mean", c_float * 3),
        ("std", c_float * 3),
        ("head", c_int32),
        ("block", c_int32 * 3),
    ]


class ResnetDesc(ctypes.Structure):
    _fields_ = [
        ("num_joints", c_int32),
        ("final_conv_kernel", c_int32),
        ("num_layers", c_int32),
        ("num_deconv_layers", c_int32),
        ("deconv_filters", c_int32 * 4),
        ("deconv_kernels", c_int32 * 4),
        ("deconv_with_bias", c_int32),
        ("dtype", c_int32),
        ("mean", c_float * 3),
        ("std", c_float * 3),
    ]


class DvsParams(ctypes.Structure):
    _fields_ = [
        ("h", c_int32),
        ("w", c_int32),
        ("pos_thres", c_float),
        ("neg_thres", c_float),
        ("pos_thres_map", c_void_p),
        ("neg_thres_map", c_void_p),
        ("noise_rate_map", c_void_p),
        ("lin_log_table", c_void_p),
        ("cutoff_hz", c_double),
        ("leak_rate_hz", c_double),
        ("refractory_period_s", c_double),
        ("max_iters", c_int32),
    ]


# name -> (restype, argtypes); every symbol include/scpose.h declares
SYMBOLS = {
    "scpose_abi_version": (c_int32, []),
    "scpose_last_error": (c_char_p, []),
    "scpose_is_dev_build": (c_int32, []),
    "scpose_hrnet_create": (c_int32, [POINTER(HrnetDesc), POINTER(c_char_p), POINTER(c_void_p),
                                      POINTER(c_int64), c_int32, c_int32, POINTER(c_void_p)]),
    "scpose_resnet_create": (c_int32, [POINTER(ResnetDesc), POINTER(c_char_p), POINTER(c_void_p),
                                       POINTER(c_int64), c_int32, c_int32, POINTER(c_void_p)]),
    "scpose_hrnet_destroy": (c_int32, [c_void_p]),
    "scpose_hrnet_workspace_bytes": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_hrnet_heatmap_size": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)]),
    "scpose_hrnet_stats": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_int32), POINTER(c_double),
                                     POINTER(c_double)]),
    "scpose_hrnet_executed_stats": (c_int32, [c_void_p, c_int32, c_int32, POINTER(c_double), POINTER(c_double)]),
    "scpose_hrnet_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                       c_void_p, c_size_t, c_void_p]),
    "scpose_hrnet_tail_fused": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_int32)]),
    "scpose_hrnet_forward_decode": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_hrnet_graph_create_decode": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                                   c_void_p, c_void_p, c_void_p, c_size_t, c_int32, POINTER(c_void_p)]),
    "scpose_hrnet_graph_workspace_bytes": (c_int32, [c_void_p, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_hrnet_graph_create": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_size_t,
                                            c_int32, POINTER(c_void_p)]),
    "scpose_hrnet_graph_launch": (c_int32, [c_void_p, c_void_p]),
    "scpose_hrnet_graph_nodes": (c_int32, [c_void_p, POINTER(c_int32)]),
    "scpose_hrnet_graph_destroy": (c_int32, [c_void_p]),
    "scpose_hrnet_tap_names": (c_int32, [c_void_p, c_char_p, c_int32]),
    "scpose_hrnet_forward_tap": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_char_p, c_void_p,
                                           POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), c_void_p, c_size_t, c_void_p]),
    "scpose_hrnet_forward_profiled": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                                c_void_p, c_size_t, c_void_p]),
    "scpose_hrnet_forward_decode_profiled": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                                       c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_hrnet_profile_read": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_void_p, POINTER(c_int32)]),
    "scpose_decode": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32,
                                c_void_p, c_void_p]),
    "scpose_max_preds": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                   c_void_p]),
    "scpose_crop_warp": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                   c_void_p]),
    "scpose_crop_warp_roi": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                       c_void_p]),
    "scpose_events_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_events_frame_bounds": (c_int32, [c_void_p, c_int64, c_void_p, c_int32, c_void_p, c_void_p]),
    "scpose_events_render": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_count_frames": (c_int32, [c_int64, c_int64, POINTER(c_int64)]),
    "scpose_events_count_bounds": (c_int32, [c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "scpose_events_area_bounds_workspace_bytes": (c_int32, [c_int64, c_int64, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_events_area_bounds": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int64,
                                            c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_bounds_midpoints": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "scpose_events_csv_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_csv_parse": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_text_tiling": (c_int32, [POINTER(c_int32), POINTER(c_int32)]),
    "scpose_events_text_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_text_measure": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_text_emit": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int64,
                                          c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat2_pack": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p,
                                            c_void_p]),
    "scpose_events_aedat2_unpack_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_aedat2_unpack": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_double,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t,
                                              c_void_p]),
    "scpose_events_aedat3_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_aedat3_count": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat3_unpack": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_aedat4_measure": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_decode": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_count": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_unpack": (c_int32, [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_zstd_workspace_bytes": (c_int32, [c_int64, POINTER(c_size_t)]),
    "scpose_events_aedat4_zstd_measure": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_zstd_decode": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_size_t,
                                                   c_void_p]),
    "scpose_events_aedat4_pack_sizes": (c_int32, [c_int64, c_int64, c_int32, POINTER(c_size_t), POINTER(c_size_t)]),
    "scpose_events_aedat4_pack": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32,
                                            c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_events_aedat4_frame_sizes": (c_int32, [c_int64, c_int64, POINTER(c_size_t), POINTER(c_size_t)]),
    "scpose_events_aedat4_frame": (c_int32, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_size_t, c_void_p]),
    "scpose_jpeg_decode_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_jpeg_decode": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_jpeg_decode_crop": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                          c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_png_decode_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_png_decode": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                    c_size_t, c_void_p]),
    "scpose_png_decode_crop": (c_int32, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                         c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_resize_area_workspace_bytes": (c_int32, [c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_resize_area_u8": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_jpeg_encode_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_jpeg_encode_capacity_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int64)]),
    "scpose_jpeg_encode": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p,
                                     c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_overlay_draw": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p]),
    "scpose_dvs_state_bytes": (c_int32, [c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_dvs_workspace_bytes": (c_int32, [c_int32, c_int32, c_int32, c_int32, POINTER(c_size_t)]),
    "scpose_dvs_init": (c_int32, [c_void_p, c_void_p, c_double, POINTER(DvsParams), c_void_p]),
    "scpose_dvs_emulate": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, POINTER(DvsParams), c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "scpose_heatmap_accumulate": (c_int32, [c_void_p, c_void_p, c_float, c_int64, c_void_p]),
    "scpose_flip_merge": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                    c_void_p]),
    "scpose_pnp_epnp_ransac": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                         c_int32, c_double, c_int32, c_int32, c_double, c_double, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p]),
    "scpose_pnp_epnp_ransac_rows": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                              c_int32, c_double, c_int32, c_int32, c_double, c_double, c_void_p, c_void_p]),
    "scpose_pnp_epnp_ransac_refine": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_double,
                                                c_int32, c_double, c_int32, c_int32, c_double, c_double, c_int32,
                                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "scpose_conv_create": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                     POINTER(c_void_p)]),
    "scpose_conv_destroy": (c_int32, [c_void_p]),
    "scpose_conv_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32,
                                      c_int32, c_void_p, c_void_p]),
    "scpose_deconv_create": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "scpose_conv1x1s2_create": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, POINTER(c_void_p)]),
    "scpose_gather_destroy": (c_int32, [c_void_p]),
    "scpose_gather_forward": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    "scpose_resnet_stem_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p, c_void_p]),
    "scpose_basic_block_forward": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "scpose_fuse_sum": (c_int32, [POINTER(c_void_p), POINTER(c_int32), c_int32, c_int32, c_int32, c_int32,
                                  c_int32, c_int32, c_void_p, c_void_p]),
    "scpose_nchw_f32_to_blocked": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p, c_void_p]),
    "scpose_blocked_to_nchw_f32": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                                             c_void_p, c_void_p]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    """Load (once) and return the HIP library; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            "%s not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (or `make -C %s`). There is no CPU fallback." % (LIB_PATH, os.path.join(_HERE, "csrc")))
    # PyTorch-ROCm ships its own libamdhip64; load it FIRST so that this library binds to the
    # same HIP runtime (two runtimes in one process do not see each other's device state).
    import torch  # noqa: F401
    try:
        handle = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 missing
        raise NativeError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(handle, name)
        except AttributeError:
            raise NativeError("%s does not export %s (stale build?)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    if handle.scpose_abi_version() != ABI_VERSION:
        raise NativeError("ABI version mismatch: library %d, binding %d" % (handle.scpose_abi_version(), ABI_VERSION))
    _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().scpose_last_error()
        raise NativeError("%s failed (%d): %s" % (what or "scpose call", rc, msg.decode() if msg else "?"))
