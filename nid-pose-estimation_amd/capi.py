"""ctypes binding of the C-ABI (include/nid/nid_c.h) exported by libnid_hip.so.

This is plumbing for tests and bench.py; the product is the shared library.
Loading fails loudly when the HIP library has not been built -- there is no
CPU fallback of any kind.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NID_HIP_LIB") or os.path.join(_HERE, "libnid_hip.so")  # NID_HIP_LIB: experiment builds of the same C-ABI

NID_OK = 0
NID_SLOTS = 1024
NID_MAX_BATCH = 256
NID_REDUCED_LEN = 32
NID_CELL_OUT = 10
JACBOUND_CPU, JACBOUND_CUDA = 0, 1
XFORM_QUAT, XFORM_MATRIX = 0, 1
MATH_FAST, MATH_STRICT = 0, 1

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
c_fp = C.POINTER(C.c_float)


class NidConfig(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("cell_num", C.c_int32),
                ("bin_num", C.c_int32), ("bs_degree", C.c_int32), ("device", C.c_int32),
                ("cell_begin", C.c_int32), ("cell_end", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


# every symbol include/nid/nid_c.h declares (tests/test_abi.py checks the export table)
SYMBOLS = [
    "nid_abi_version", "nid_status_string", "nid_last_error", "nid_device_count", "nid_create", "nid_create_strided",
    "nid_destroy", "nid_set_options", "nid_set_math_mode", "nid_set_href_nan_markers", "nid_set_stream", "nid_set_block_threads", "nid_set_launch_shape",
    "nid_set_reference_depth", "nid_set_pair_u16", "nid_set_reference_points", "nid_backproject", "nid_backproject_release", "nid_get_points3d", "nid_set_target_u8",
    "nid_set_target_f64", "nid_set_reference_image_f64", "nid_compute_href",
    "nid_compute_href_matrix", "nid_set_href_state", "nid_plain_nid", "nid_evaluate", "nid_evaluate_matrix",
    "nid_normal_equations", "nid_launch", "nid_launch_batch", "nid_launch_chain", "nid_launch_batch_to", "nid_run_sequence", "nid_run_chain", "nid_set_loop_form", "nid_set_direct_results", "nid_set_resident", "nid_resident_pause", "nid_resident_stats", "nid_wait", "nid_slot_buffers", "nid_debug_read_device", "nid_launch_to",
    "nid_unpack_reduced", "nid_debug_enable_pixel_dump", "nid_debug_get_pixel_dump",
    "nid_debug_enable_stamps", "nid_debug_get_stamps", "nid_bspline4_host", "nid_bspline4_poly_host", "nid_log2_fast_host", "nid_div_small_host", "nid_last_kernel_ms", "nid_enable_timing", "nid_time_launches", "nid_time_kernel",
    "nid_contract_bytes", "nid_debug_repair_count", "nid_set_short_sequence_policy",
]

# include/nid/nid_multistart.h (a header of its own: the symbols above are nid_c.h's, pinned by tests/test_abi.py)
MULTISTART_SYMBOLS = ["nid_multistart_lm", "nid_lm_step_host", "nid_lm_step_device"]
MS_RUNNING, MS_ITERATIONS, MS_TRIALS_EXHAUSTED, MS_RHO_NOT_NEGATIVE, MS_NBAD = 0, 1, 2, 3, 4
MS_F_FIRST, MS_F_ACCEPT, MS_F_REJECT, MS_F_OUTER_END, MS_F_SOLVE_FAILED, MS_F_FINISHED = 1, 2, 4, 8, 16, 32


class MsState(C.Structure):
    """nid_ms_state: one LM chain (zero it, set pose7 / iterations / xform_mode: new_ms_state)."""
    _fields_ = [("pose7", C.c_double * 7), ("chi2", C.c_double), ("H", C.c_double * 21), ("b", C.c_double * 6),
                ("lambda_", C.c_double), ("ni", C.c_double), ("ini_chi2", C.c_double), ("x", C.c_double * 6),
                ("trial7", C.c_double * 7), ("trial_chi2", C.c_double), ("rho", C.c_double),
                ("rec_q", C.c_double * 7), ("rec_M", C.c_double * 12),
                ("iterations", C.c_int32), ("xform_mode", C.c_int32), ("started", C.c_int32), ("n_active", C.c_int32),
                ("n_bad", C.c_int32), ("trials", C.c_int32), ("outer_done", C.c_int32), ("trials_total", C.c_int32),
                ("solve_ok", C.c_int32), ("status", C.c_int32), ("flags", C.c_int32), ("rec_mode", C.c_int32)]


# nid_ms_result / nid_ms_trace as numpy records (tobytes() of two arrays compares every bit)
MS_RESULT_DTYPE = np.dtype([("pose7", "f8", 7), ("chi2", "f8"), ("lambda_", "f8"), ("n_active", "i4"),
                            ("outer_iterations", "i4"), ("trials", "i4"), ("status", "i4")])
MS_TRACE_DTYPE = np.dtype([("trial_chi2", "f8"), ("lambda_", "f8"), ("rho", "f8"), ("pose7", "f8", 7),
                           ("flags", "i4"), ("status", "i4")])
assert C.sizeof(MsState) == 624 and MS_RESULT_DTYPE.itemsize == 88 and MS_TRACE_DTYPE.itemsize == 88

# include/nid/nid_pyr.h (a header of its own, like nid_multistart.h)
PYR_SYMBOLS = ["nid_pyr_level_config", "nid_pyr_create", "nid_pyr_destroy", "nid_pyr_levels", "nid_pyr_level",
               "nid_pyr_set_pair_u16", "nid_pyr_get_level_inputs", "nid_pyr_multistart_lm"]
PYR_MAX_LEVELS = 8

# include/nid/nid_pyr_stream.h (a header of its own again: frame streams on the resident pyramid, pose helpers, a tracker)
STREAM_SYMBOLS = ["nid_pyr_set_target_u8", "nid_pyr_promote_target_u16",
                  "nid_track_pose_inverse", "nid_track_pose_compose", "nid_track_pose_perturb", "nid_track_pose_to_Twc16",
                  "nid_track_pose_from_Twc16",
                  "nid_track_create", "nid_track_destroy", "nid_track_pyramid", "nid_track_set_lm", "nid_track_set_twists",
                  "nid_track_set_pose", "nid_track_push_u16"]
TRACK_FIRST, TRACK_OK, TRACK_LOST = 0, 1, 2


class TrackResult(C.Structure):
    """nid_track_result"""
    _fields_ = [("pose7", C.c_double * 7), ("chi2", C.c_double), ("n_active", C.c_int32), ("best_origin", C.c_int32),
                ("status", C.c_int32), ("promoted", C.c_int32), ("frame", C.c_int32), ("rounds", C.c_int32 * PYR_MAX_LEVELS)]


assert C.sizeof(TrackResult) == 120

# include/nid/nid_keyframe.h (a header of its own once more: the depth-consistency check and the tracker's keyframe policy)
KEYFRAME_SYMBOLS = ["nid_pyr_set_target_depth_u16", "nid_pyr_promote_target", "nid_pyr_depth_check", "nid_depth_check_host",
                    "nid_track_policy_default", "nid_track_set_policy", "nid_track_last_check"]
TRACK_REJECTED = 3
# nid_depth_cell / nid_depth_counts as numpy records (tobytes() of two arrays compares every bit)
DEPTH_CELL_DTYPE = np.dtype([("n_ref", "i4"), ("n_inframe", "i4"), ("n_both", "i4"), ("n_consistent", "i4"), ("n_occluded", "i4"),
                             ("n_through", "i4"), ("sum_abs_um", "u8")])
DEPTH_COUNTS_DTYPE = np.dtype([("n_ref", "i8"), ("n_inframe", "i8"), ("n_both", "i8"), ("n_consistent", "i8"), ("n_occluded", "i8"),
                               ("n_through", "i8"), ("sum_abs_um", "u8"), ("reserved", "u8")])


class TrackPolicy(C.Structure):
    """nid_track_policy"""
    _fields_ = [("keyframe_mode", C.c_int32), ("max_age", C.c_int32), ("min_samples", C.c_int32), ("reserved", C.c_int32),
                ("min_overlap", C.c_double), ("min_consistent", C.c_double), ("tol_abs", C.c_double), ("tol_rel", C.c_double)]


assert DEPTH_CELL_DTYPE.itemsize == 32 and DEPTH_COUNTS_DTYPE.itemsize == 64 and C.sizeof(TrackPolicy) == 48

# include/nid/nid_refmask.h (a header of its own again: a per-pixel mask on the pyramid's reference, the tracker's use of it)
REFMASK_SYMBOLS = ["nid_pyr_set_reference_mask_u8", "nid_pyr_mask_occluded", "nid_pyr_clear_reference_mask",
                   "nid_pyr_get_reference_mask_u8", "nid_refmask_host", "nid_track_set_masking", "nid_track_last_mask"]
REFMASK_CALLER, REFMASK_OCCLUDED, REFMASK_THROUGH, REFMASK_DILATED = 1, 2, 4, 8
REFMASK_MAX_DILATE = 8
REFMASK_COUNTS_DTYPE = np.dtype([("n_valid", "i8"), ("n_caller", "i8"), ("n_occluded", "i8"), ("n_through", "i8"), ("n_dilated", "i8"),
                                 ("n_masked", "i8"), ("reserved", "i8", 2)])
assert REFMASK_COUNTS_DTYPE.itemsize == 64

# include/nid/nid_reffill.h (likewise: depth for the reference's holes from tracked frames, the tracker's use of it)
REFFILL_SYMBOLS = ["nid_pyr_fill_reference_depth", "nid_pyr_clear_reference_fill", "nid_pyr_get_reference_fill_u16", "nid_reffill_host",
                   "nid_track_set_filling", "nid_track_last_fill"]
REFFILL_MAX_GUARD = 2
REFFILL_COUNTS_DTYPE = np.dtype([("n_target_valid", "i8"), ("n_splat", "i8"), ("n_hit", "i8"), ("n_holes", "i8"), ("n_refused", "i8"),
                                 ("n_new", "i8"), ("n_filled", "i8"), ("reserved", "i8")])
assert REFFILL_COUNTS_DTYPE.itemsize == 64

# include/nid/nid_reffuse.h (likewise: the reference's valid depth refined from tracked frames, the tracker's use of it)
REFFUSE_SYMBOLS = ["nid_pyr_fuse_reference_depth", "nid_pyr_clear_reference_fusion", "nid_pyr_get_reference_fused_u16",
                   "nid_pyr_get_reference_fusion_obs_u8", "nid_reffuse_host", "nid_track_set_fusing", "nid_track_last_fusion"]
REFFUSE_MAX_OBS = 255
REFFUSE_COUNTS_DTYPE = np.dtype([("n_target_valid", "i8"), ("n_splat", "i8"), ("n_hit", "i8"), ("n_valid", "i8"), ("n_fused", "i8"),
                                 ("n_gated", "i8"), ("n_saturated", "i8"), ("n_changed", "i8")])
assert REFFUSE_COUNTS_DTYPE.itemsize == 64

# include/nid/nid_refgather.h (likewise: bilinear depth samples fused into the reference, the tracker's use of them)
REFGATHER_SYMBOLS = ["nid_pyr_fuse_reference_depth_bilinear", "nid_refgather_host", "nid_track_set_fusion_sampling", "nid_track_last_gather"]
REFFUSE_NEAREST, REFFUSE_BILINEAR = 0, 1
REFGATHER_COUNTS_DTYPE = np.dtype([("n_valid", "i8"), ("n_sampled", "i8"), ("n_outside", "i8"), ("n_tap_refused", "i8"), ("n_fused", "i8"),
                                   ("n_gated", "i8"), ("n_saturated", "i8"), ("n_changed", "i8")])
assert REFGATHER_COUNTS_DTYPE.itemsize == 64

_lib = None


class NidError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NidError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                       " (there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.nid_abi_version.restype = C.c_int
    lib.nid_status_string.restype = C.c_char_p
    lib.nid_status_string.argtypes = [C.c_int]
    lib.nid_last_error.restype = C.c_char_p
    lib.nid_last_error.argtypes = [vp]
    lib.nid_device_count.restype = C.c_int
    lib.nid_create.argtypes = [C.POINTER(NidConfig), C.POINTER(vp)]
    lib.nid_create_strided.argtypes = [C.POINTER(NidConfig), C.c_int32, C.POINTER(vp)]
    lib.nid_destroy.argtypes = [vp]
    lib.nid_set_options.argtypes = [vp, C.c_int, C.c_int]
    lib.nid_set_math_mode.argtypes = [vp, C.c_int]
    lib.nid_set_stream.argtypes = [vp, vp]
    lib.nid_set_block_threads.argtypes = [vp, C.c_int]
    lib.nid_set_launch_shape.argtypes = [vp, C.c_int, C.c_int]
    lib.nid_set_reference_depth.argtypes = [vp, c_dp, c_u8p, c_dp]
    lib.nid_set_pair_u16.argtypes = [vp, C.POINTER(C.c_uint16), C.c_double, c_u8p, c_u8p, c_dp, c_dp, c_dp, c_ip, c_dp]
    lib.nid_set_reference_points.argtypes = [vp, c_dp, c_u8p]
    lib.nid_get_points3d.argtypes = [vp, c_dp]
    lib.nid_backproject.argtypes = [c_dp, c_dp] + [C.c_double] * 4 + [C.c_int32] * 3 + [c_dp]
    lib.nid_set_target_u8.argtypes = [vp, c_u8p]
    lib.nid_set_target_f64.argtypes = [vp, c_dp]
    lib.nid_set_reference_image_f64.argtypes = [c_dp, C.c_int64, c_u8p]
    lib.nid_compute_href.argtypes = [vp, c_dp, c_ip, c_dp, c_dp, c_ip]
    lib.nid_compute_href_matrix.argtypes = [vp, c_dp, c_ip, c_dp, c_dp, c_ip]
    lib.nid_set_href_state.argtypes = [vp, c_ip, c_dp, c_dp, c_ip]
    lib.nid_evaluate.argtypes = [vp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp]
    lib.nid_evaluate_matrix.argtypes = [vp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp]
    lib.nid_normal_equations.argtypes = [vp, c_dp, C.c_int, C.c_double, c_dp, c_dp, c_dp, c_ip]
    lib.nid_launch.argtypes = [vp, C.c_int, c_dp, C.c_int, C.c_double]
    lib.nid_launch_batch.argtypes = [vp, C.c_int, C.c_int, c_dp, C.c_int, C.c_double]
    lib.nid_launch_batch_to.argtypes = [vp, C.c_int, C.c_int, c_dp, C.c_int, C.c_double, vp]
    lib.nid_launch_chain.argtypes = [vp, C.c_int, C.c_int, c_dp, C.c_int, C.c_double]
    lib.nid_run_sequence.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_int, C.c_double, c_dp]
    lib.nid_launch_to.argtypes = [vp, C.c_int, c_dp, C.c_int, C.c_double, vp]
    lib.nid_run_chain.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_double, c_dp, c_dp]
    lib.nid_wait.argtypes = [vp, C.c_int, c_dp, c_dp, c_dp, c_ip]
    lib.nid_slot_buffers.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(lib, "nid_debug_read_device"):  # (tools/build_variant.py builds of earlier trees lack the newest entry points)
        lib.nid_debug_read_device.argtypes = [vp, vp, C.POINTER(C.c_double), C.c_size_t]
    lib.nid_unpack_reduced.argtypes = [c_dp, c_dp, c_dp, c_dp, c_ip]
    lib.nid_debug_enable_pixel_dump.argtypes = [vp, C.c_int]
    lib.nid_debug_get_pixel_dump.argtypes = [vp, c_dp, c_dp, c_dp, c_ip, c_dp]
    lib.nid_debug_enable_stamps.argtypes = [vp, C.c_int]
    lib.nid_debug_get_stamps.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.nid_bspline4_host.restype = None
    lib.nid_bspline4_host.argtypes = [C.c_double, C.c_int, c_dp, c_dp]
    lib.nid_bspline4_poly_host.restype = None
    lib.nid_bspline4_poly_host.argtypes = [C.c_double, C.c_int, c_dp, c_dp]
    lib.nid_div_small_host.restype = C.c_double
    lib.nid_div_small_host.argtypes = [C.c_double, C.c_double]
    lib.nid_last_kernel_ms.argtypes = [vp, C.c_int, c_fp, c_fp]
    lib.nid_enable_timing.argtypes = [vp, C.c_int]
    lib.nid_set_loop_form.argtypes = [vp, C.c_int]
    lib.nid_set_direct_results.argtypes = [vp, C.c_int]
    lib.nid_set_resident.argtypes = [vp, C.c_int]
    if hasattr(lib, "nid_resident_pause"):
        lib.nid_resident_pause.argtypes = [vp]
    lib.nid_resident_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.nid_time_launches.argtypes = [vp, C.c_int, c_dp, C.c_int, C.c_double, C.c_int, c_fp]
    if hasattr(lib, "nid_time_kernel"):   # (an older experiment build, NID_HIP_LIB, may lack it)
        lib.nid_time_kernel.argtypes = [vp, C.c_int, c_dp, C.c_int, C.c_double, C.c_int, c_fp]
    if hasattr(lib, "nid_debug_repair_count"):   # (an older experiment build, NID_HIP_LIB, may lack the newest diagnostics)
        lib.nid_debug_repair_count.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    if hasattr(lib, "nid_set_short_sequence_policy"):
        lib.nid_set_short_sequence_policy.argtypes = [vp, C.c_int, C.c_int]
    lib.nid_contract_bytes.restype = C.c_int64
    lib.nid_contract_bytes.argtypes = [vp]
    if hasattr(lib, "nid_multistart_lm"):   # (an older experiment build, NID_HIP_LIB, lacks it: calling it is an error there)
        lib.nid_multistart_lm.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_double, C.c_int, vp, c_ip, vp, c_ip]
        lib.nid_lm_step_host.argtypes = [C.POINTER(MsState), c_dp]
    if hasattr(lib, "nid_lm_step_device"):   # (likewise)
        lib.nid_lm_step_device.argtypes = [vp, C.POINTER(MsState), c_dp, C.c_int, c_dp, c_ip, vp, C.POINTER(C.c_uint32)]
    if hasattr(lib, "nid_pyr_create"):   # (an older experiment build, NID_HIP_LIB, lacks it: calling it is an error there)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_level_config.argtypes = [C.POINTER(NidConfig), C.c_int, C.POINTER(NidConfig)]
        lib.nid_pyr_create.argtypes = [C.POINTER(NidConfig), C.c_int, C.POINTER(vp)]
        lib.nid_pyr_destroy.argtypes = [vp]
        lib.nid_pyr_levels.argtypes = [vp]
        lib.nid_pyr_level.restype = vp
        lib.nid_pyr_level.argtypes = [vp, C.c_int]
        lib.nid_pyr_set_pair_u16.argtypes = [vp, u16p, C.c_double, c_u8p, c_u8p, c_dp]
        lib.nid_pyr_get_level_inputs.argtypes = [vp, C.c_int, u16p, c_u8p, c_u8p]
        lib.nid_pyr_multistart_lm.argtypes = [vp, c_dp, C.c_int, c_dp, C.c_int, C.c_double, c_ip, vp, c_ip, c_ip, c_ip, c_dp]
    if hasattr(lib, "nid_track_create"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_set_target_u8.argtypes = [vp, c_u8p]
        lib.nid_pyr_promote_target_u16.argtypes = [vp, u16p, C.c_double, c_dp]
        lib.nid_track_pose_inverse.argtypes = [c_dp, c_dp]
        lib.nid_track_pose_compose.argtypes = [c_dp, c_dp, c_dp]
        lib.nid_track_pose_perturb.argtypes = [c_dp, c_dp, c_dp]
        lib.nid_track_pose_to_Twc16.argtypes = [c_dp, c_dp]
        lib.nid_track_pose_from_Twc16.argtypes = [c_dp, c_dp]
        lib.nid_track_create.argtypes = [C.POINTER(NidConfig), C.c_int, C.POINTER(vp)]
        lib.nid_track_destroy.argtypes = [vp]
        lib.nid_track_pyramid.restype = vp
        lib.nid_track_pyramid.argtypes = [vp]
        lib.nid_track_set_lm.argtypes = [vp, C.c_int, C.c_double, c_ip]
        lib.nid_track_set_twists.argtypes = [vp, c_dp, C.c_int]
        lib.nid_track_set_pose.argtypes = [vp, c_dp]
        lib.nid_track_push_u16.argtypes = [vp, u16p, C.c_double, c_u8p, c_dp, C.POINTER(TrackResult)]
    if hasattr(lib, "nid_pyr_depth_check"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_set_target_depth_u16.argtypes = [vp, u16p, C.c_double]
        lib.nid_pyr_promote_target.argtypes = [vp, c_dp]
        lib.nid_pyr_depth_check.argtypes = [vp, c_dp, C.c_int, C.c_double, C.c_double, vp, vp]
        lib.nid_depth_check_host.argtypes = [C.POINTER(NidConfig), c_dp, u16p, C.c_double, c_dp, C.c_double, C.c_double, vp, vp]
        lib.nid_track_policy_default.argtypes = [C.POINTER(TrackPolicy)]
        lib.nid_track_set_policy.argtypes = [vp, C.POINTER(TrackPolicy)]
        lib.nid_track_last_check.argtypes = [vp, vp, c_ip, c_ip]
    if hasattr(lib, "nid_pyr_mask_occluded"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_set_reference_mask_u8.argtypes = [vp, c_u8p]
        lib.nid_pyr_mask_occluded.argtypes = [vp, c_dp, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, vp]
        lib.nid_pyr_clear_reference_mask.argtypes = [vp]
        lib.nid_pyr_get_reference_mask_u8.argtypes = [vp, c_u8p]
        lib.nid_refmask_host.argtypes = [C.POINTER(NidConfig), u16p, C.c_double, c_dp, u16p, C.c_double, c_dp, C.c_double, C.c_double,
                                         C.c_int, C.c_int, C.c_int, c_u8p, vp]
        lib.nid_track_set_masking.argtypes = [vp, C.c_int, C.c_int]
        lib.nid_track_last_mask.argtypes = [vp, vp]
    if hasattr(lib, "nid_pyr_fill_reference_depth"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_fill_reference_depth.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        lib.nid_pyr_clear_reference_fill.argtypes = [vp]
        lib.nid_pyr_get_reference_fill_u16.argtypes = [vp, u16p]
        lib.nid_reffill_host.argtypes = [C.POINTER(NidConfig), u16p, C.c_double, c_dp, u16p, C.c_double, c_dp, C.c_int, C.c_int, C.c_int,
                                         C.c_int, u16p, vp]
        lib.nid_track_set_filling.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.nid_track_last_fill.argtypes = [vp, vp]
    if hasattr(lib, "nid_pyr_fuse_reference_depth"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_fuse_reference_depth.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_int, vp]
        lib.nid_pyr_clear_reference_fusion.argtypes = [vp]
        lib.nid_pyr_get_reference_fused_u16.argtypes = [vp, u16p]
        lib.nid_pyr_get_reference_fusion_obs_u8.argtypes = [vp, c_u8p]
        lib.nid_reffuse_host.argtypes = [C.POINTER(NidConfig), u16p, C.c_double, c_dp, u16p, C.c_double, c_dp, C.c_int, C.c_int, C.c_int,
                                         C.POINTER(C.c_uint32), c_u8p, u16p, vp]
        lib.nid_track_set_fusing.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.nid_track_last_fusion.argtypes = [vp, vp]
    if hasattr(lib, "nid_pyr_fuse_reference_depth_bilinear"):   # (likewise)
        u16p = C.POINTER(C.c_uint16)
        lib.nid_pyr_fuse_reference_depth_bilinear.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        lib.nid_refgather_host.argtypes = [C.POINTER(NidConfig), u16p, C.c_double, c_dp, u16p, C.c_double, c_dp, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.POINTER(C.c_uint32), c_u8p, u16p, vp]
        lib.nid_track_set_fusion_sampling.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        lib.nid_track_last_gather.argtypes = [vp, vp]
    _lib = lib
    return lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _dp(a):
    return a.ctypes.data_as(c_dp) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(c_ip) if a is not None else None


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


class Context:
    """One frame pair on one MI355X (or one cell shard of it)."""

    def __init__(self, rows, cols, cell_num, bin_num, fx, fy, cx, cy, device=0, cell_begin=0,
                 cell_end=0, jac_bound=JACBOUND_CPU, xform=XFORM_QUAT, cell_stride=1):
        self.lib = load()
        cfg = NidConfig(rows, cols, cell_num, bin_num, 3, device, cell_begin, cell_end, fx, fy, cx, cy)
        h = C.c_void_p()
        rc = self.lib.nid_create_strided(C.byref(cfg), int(cell_stride), C.byref(h))
        if rc != NID_OK:
            raise NidError(f"nid_create: {self.lib.nid_status_string(rc).decode()} ({rc})")
        self.h = h
        self.rows, self.cols, self.cell_num, self.bin_num = rows, cols, cell_num, bin_num
        self.ncell = cell_num * cell_num
        self.cell_begin = cell_begin
        self.cell_end = cell_end if cell_end else self.ncell
        self._check(self.lib.nid_set_options(self.h, jac_bound, xform), "nid_set_options")

    @classmethod
    def borrow(cls, multi, k):
        """Shard k of a Multi as a Context (not owned: closing it does nothing)."""
        self = cls.__new__(cls)
        self.lib = load()
        self.h = C.c_void_p(multi.lib.nid_multi_shard(multi.h, int(k)))
        if not self.h:
            raise NidError(f"nid_multi_shard({k}): no such shard")
        self._borrowed = True
        self._owner = multi   # keeps the Multi (and with it this shard) alive as long as the borrowed handle is
        self.rows, self.cols, self.cell_num, self.bin_num = multi.rows, multi.cols, multi.cell_num, multi.bin_num
        self.ncell = multi.ncell
        self.cell_begin, self.cell_end = 0, self.ncell
        return self

    def _check(self, rc, what):
        if rc != NID_OK:
            msg = self.lib.nid_last_error(self.h).decode() if self.h else ""
            raise NidError(f"{what}: {self.lib.nid_status_string(rc).decode()} ({rc}) {msg}")

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.nid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup --------------------------------------------------------------
    def set_reference_depth(self, depth_m, im0, T_wc0_colmajor16):
        d, im, T = _d(depth_m).reshape(-1), _u8(im0).reshape(-1), _d(T_wc0_colmajor16)
        assert d.size == self.rows * self.cols and im.size == d.size and T.size == 16
        self._check(self.lib.nid_set_reference_depth(self.h, _dp(d), im.ctypes.data_as(c_u8p), _dp(T)),
                    "nid_set_reference_depth")

    def set_pair_u16(self, depth_u16, depth_factor, im0, im1, T_wc0_colmajor16, pose0, matrix=False):
        """nid_set_pair_u16: the whole pair in the driver's formats + the reference stage at pose0 (pose7, or a
        column-major 4x4 with matrix=True); returns (bs_counter, Href)."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1)
        a, b, T, p = _u8(im0).reshape(-1), _u8(im1).reshape(-1), _d(T_wc0_colmajor16), _d(pose0)
        assert d.size == self.rows * self.cols and a.size == d.size and b.size == d.size and T.size == 16 and p.size == (16 if matrix else 7)
        cnt = np.zeros(self.ncell, dtype=np.int32)
        href = np.full(self.ncell, np.nan)
        self._check(self.lib.nid_set_pair_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor), a.ctypes.data_as(c_u8p),
                                              b.ctypes.data_as(c_u8p), _dp(T), None if matrix else _dp(p), _dp(p) if matrix else None,
                                              _ip(cnt), _dp(href)), "nid_set_pair_u16")
        return cnt, href

    def set_reference_points(self, points3d, im0):
        p, im = _d(points3d).reshape(-1), _u8(im0).reshape(-1)
        assert p.size == 3 * self.rows * self.cols and im.size == self.rows * self.cols
        self._check(self.lib.nid_set_reference_points(self.h, _dp(p), im.ctypes.data_as(c_u8p)),
                    "nid_set_reference_points")

    def get_points3d(self):
        out = np.empty(3 * self.rows * self.cols)
        self._check(self.lib.nid_get_points3d(self.h, _dp(out)), "nid_get_points3d")
        return out

    def set_target(self, im1):
        im = _u8(im1).reshape(-1)
        assert im.size == self.rows * self.cols
        self._check(self.lib.nid_set_target_u8(self.h, im.ctypes.data_as(c_u8p)), "nid_set_target_u8")

    def compute_href(self, pose7, dump=False):
        cnt = np.zeros(self.ncell, dtype=np.int32)
        href = np.full(self.ncell, np.nan)
        N = self.rows * self.cols
        bsv = np.zeros((N, 4)) if dump else None
        bsi = np.zeros(N, dtype=np.int32) if dump else None
        self._check(self.lib.nid_compute_href(self.h, _dp(_d(pose7)), _ip(cnt), _dp(href), _dp(bsv), _ip(bsi)),
                    "nid_compute_href")
        return (cnt, href, bsv, bsi) if dump else (cnt, href)

    def compute_href_matrix(self, pose16):
        cnt = np.zeros(self.ncell, dtype=np.int32)
        href = np.full(self.ncell, np.nan)
        self._check(self.lib.nid_compute_href_matrix(self.h, _dp(_d(pose16)), _ip(cnt), _dp(href), None, None), "nid_compute_href_matrix")
        return cnt, href

    # ---- per iteration --------------------------------------------------------
    def plain_nid(self, pose7, bins=8):
        """Plain-histogram NID per cell (NID_standard_property.cpp): dict of per-cell arrays + 'total'."""
        n = self.ncell
        out = {k: np.full(n, np.nan) for k in ("Href", "Hcur", "Hjoint", "nid", "mi")}
        n_in = np.zeros(n, dtype=np.int32)
        total = C.c_double(0)
        self.lib.nid_plain_nid.argtypes = [C.c_void_p, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, C.POINTER(C.c_double)]
        self._check(self.lib.nid_plain_nid(self.h, _dp(_d(pose7)), int(bins), _dp(out["Href"]), _dp(out["Hcur"]),
                                           _dp(out["Hjoint"]), _dp(out["nid"]), _dp(out["mi"]), _ip(n_in),
                                           C.byref(total)), "nid_plain_nid")
        out["n_in"] = n_in
        out["total"] = float(total.value)
        return out

    def evaluate(self, pose7, want_jac=True):
        Hc = np.full(self.ncell, np.nan)
        Hj = np.full(self.ncell, np.nan)
        err = np.full(self.ncell, np.nan)
        J = np.full((self.ncell, 6), np.nan) if want_jac else None
        self._check(self.lib.nid_evaluate(self.h, _dp(_d(pose7)), 1 if want_jac else 0, _dp(Hc), _dp(Hj),
                                          _dp(err), _dp(J)), "nid_evaluate")
        return Hc, Hj, err, J

    def evaluate_matrix(self, pose16, want_jac=True):
        Hc = np.full(self.ncell, np.nan)
        Hj = np.full(self.ncell, np.nan)
        err = np.full(self.ncell, np.nan)
        J = np.full((self.ncell, 6), np.nan) if want_jac else None
        self._check(self.lib.nid_evaluate_matrix(self.h, _dp(_d(pose16)), 1 if want_jac else 0, _dp(Hc),
                                                 _dp(Hj), _dp(err), _dp(J)), "nid_evaluate_matrix")
        return Hc, Hj, err, J

    def normal_equations(self, pose7, delta, want_jac=True):
        H = np.zeros(36)
        b = np.zeros(6)
        chi2 = C.c_double(0)
        na = C.c_int32(0)
        self._check(self.lib.nid_normal_equations(self.h, _dp(_d(pose7)), 1 if want_jac else 0, float(delta),
                                                  _dp(H), _dp(b), C.byref(chi2), C.byref(na)),
                    "nid_normal_equations")
        return H.reshape(6, 6), b, chi2.value, na.value

    def launch(self, slot, pose7, delta, want_jac=True, reduced_dev=None):
        p = _d(pose7)
        if reduced_dev is None:
            rc = self.lib.nid_launch(self.h, slot, _dp(p), 1 if want_jac else 0, float(delta))
        else:
            rc = self.lib.nid_launch_to(self.h, slot, _dp(p), 1 if want_jac else 0, float(delta),
                                        C.c_void_p(reduced_dev))
        self._check(rc, "nid_launch")

    def launch_batch(self, first_slot, poses7, delta, want_jac=True, reduced_dev=None):
        p = _d(np.asarray(poses7).reshape(-1, 7))
        if reduced_dev is None:
            rc = self.lib.nid_launch_batch(self.h, first_slot, p.shape[0], _dp(p), 1 if want_jac else 0, float(delta))
        else:
            rc = self.lib.nid_launch_batch_to(self.h, first_slot, p.shape[0], _dp(p), 1 if want_jac else 0,
                                              float(delta), C.c_void_p(reduced_dev))
        self._check(rc, "nid_launch_batch")

    def launch_chain(self, first_slot, poses7, n_jac, delta):
        """an LM rejection chain: the first n_jac poses with the Jacobian phase, the rest cost only, concurrently"""
        p = _d(np.asarray(poses7).reshape(-1, 7))
        self._check(self.lib.nid_launch_chain(self.h, first_slot, p.shape[0], _dp(p), int(n_jac), float(delta)),
                    "nid_launch_chain")

    def run_sequence(self, poses7, delta, batch=8, want_jac=True, collect=True):
        p = _d(np.asarray(poses7).reshape(-1, 7))
        out = np.zeros((p.shape[0], NID_REDUCED_LEN)) if collect else None
        self._check(self.lib.nid_run_sequence(self.h, _dp(p), p.shape[0], int(batch), 1 if want_jac else 0,
                                              float(delta), _dp(out)), "nid_run_sequence")
        return out

    def run_chain(self, poses7, delta, want_jac=True, collect=True):
        """A dependent chain: one pose per launch, each result awaited on the host before the next launch.
        Returns (reduced blocks or None, seconds)."""
        p = _d(np.asarray(poses7).reshape(-1, 7))
        out = np.zeros((p.shape[0], NID_REDUCED_LEN)) if collect else None
        sec = C.c_double(0)
        self._check(self.lib.nid_run_chain(self.h, _dp(p), p.shape[0], 1 if want_jac else 0, float(delta), _dp(out),
                                           C.byref(sec)), "nid_run_chain")
        return out, float(sec.value)

    def wait(self, slot):
        H = np.zeros(36)
        b = np.zeros(6)
        chi2 = C.c_double(0)
        na = C.c_int32(0)
        self._check(self.lib.nid_wait(self.h, slot, _dp(H), _dp(b), C.byref(chi2), C.byref(na)), "nid_wait")
        return H.reshape(6, 6), b, chi2.value, na.value

    def slot_buffers(self, slot):
        """(reduced_dev, cellout_dev): device addresses of the slot's blocks (nid_slot_buffers)"""
        r, c = C.c_void_p(0), C.c_void_p(0)
        self._check(self.lib.nid_slot_buffers(self.h, int(slot), C.byref(r), C.byref(c)), "nid_slot_buffers")
        return r.value, c.value

    def read_device(self, dev, shape):
        out = np.zeros(shape)
        self._check(self.lib.nid_debug_read_device(self.h, C.c_void_p(dev), _dp(out), out.nbytes), "nid_debug_read_device")
        return out

    def set_math_mode(self, mode):
        self._check(self.lib.nid_set_math_mode(self.h, int(mode)), "nid_set_math_mode")

    def set_options(self, jac_bound=JACBOUND_CPU, xform=XFORM_QUAT):
        self._check(self.lib.nid_set_options(self.h, int(jac_bound), int(xform)), "nid_set_options")

    def set_stream(self, stream_handle):
        self._check(self.lib.nid_set_stream(self.h, C.c_void_p(stream_handle)), "nid_set_stream")

    def set_block_threads(self, n):
        self._check(self.lib.nid_set_block_threads(self.h, int(n)), "nid_set_block_threads")

    def set_launch_shape(self, jac_threads=0, cost_threads=0):
        self._check(self.lib.nid_set_launch_shape(self.h, int(jac_threads), int(cost_threads)), "nid_set_launch_shape")

    def set_loop_form(self, on=True):
        self._check(self.lib.nid_set_loop_form(self.h, 1 if on else 0), "nid_set_loop_form")

    def set_direct_results(self, on=True):
        self._check(self.lib.nid_set_direct_results(self.h, int(on)), "nid_set_direct_results")

    def set_resident(self, on=True):
        """False / 0: off; True / 1: single-pose requests are answered by the resident kernel."""
        self._check(self.lib.nid_set_resident(self.h, int(on)), "nid_set_resident")

    def resident_pause(self):
        self._check(self.lib.nid_resident_pause(self.h), "nid_resident_pause")

    def resident_stats(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self.lib.nid_resident_stats(self.h, C.byref(a), C.byref(b), C.byref(c)), "nid_resident_stats")
        return dict(served=a.value, fallbacks=b.value, starts=c.value)

    def enable_timing(self, on=True):
        self._check(self.lib.nid_enable_timing(self.h, 1 if on else 0), "nid_enable_timing")

    def last_kernel_ms(self, slot):
        a, b = C.c_float(0), C.c_float(0)
        self._check(self.lib.nid_last_kernel_ms(self.h, slot, C.byref(a), C.byref(b)), "nid_last_kernel_ms")
        return a.value, b.value

    def time_launches(self, poses7, delta, repeats=10, want_jac=True):
        """ms per launch of `repeats` back-to-back launches of these poses (one HIP event pair)."""
        ps = np.ascontiguousarray(np.asarray(poses7, dtype=np.float64).reshape(-1, 7))
        ms = C.c_float(0)
        self._check(self.lib.nid_time_launches(self.h, ps.shape[0], _dp(ps), int(want_jac), float(delta), int(repeats),
                                               C.byref(ms)), "nid_time_launches")
        return float(ms.value)

    def time_kernel(self, poses7, delta, repeats=10, want_jac=True):
        """ms of the evaluation kernel ALONE per launch of these poses (events right around k_eval2, one launch at a time)."""
        ps = np.ascontiguousarray(np.asarray(poses7, dtype=np.float64).reshape(-1, 7))
        ms = C.c_float(0)
        self._check(self.lib.nid_time_kernel(self.h, ps.shape[0], _dp(ps), int(want_jac), float(delta), int(repeats),
                                             C.byref(ms)), "nid_time_kernel")
        return float(ms.value)

    def contract_bytes(self):
        return int(self.lib.nid_contract_bytes(self.h))

    def set_short_sequence_policy(self, poses_per_launch=0, streams=0):
        """How nid_launch_batch / nid_run_sequence split a short sequence (0, 0: the library's table)."""
        self._check(self.lib.nid_set_short_sequence_policy(self.h, int(poses_per_launch), int(streams)), "nid_set_short_sequence_policy")

    def multistart_lm(self, poses, iterations, delta, max_rounds=0, trace=False):
        """Many LM chains at once, stepped on the device (nid_multistart_lm).  Returns (results, best, rounds_done) or,
        with trace=True, (results, best, rounds_done, trace): results an MS_RESULT_DTYPE array [n], trace an
        MS_TRACE_DTYPE array [rounds_done, n]."""
        p = _d(np.asarray(poses).reshape(-1, 7))
        n = p.shape[0]
        cap = int(max_rounds) if max_rounds > 0 else 1 + 10 * int(iterations)
        res = np.zeros(max(n, 1), dtype=MS_RESULT_DTYPE)
        tr = np.zeros((cap, max(n, 1)), dtype=MS_TRACE_DTYPE) if trace else None
        best, rounds = C.c_int32(-2), C.c_int32(0)
        self._check(self.lib.nid_multistart_lm(self.h, _dp(p), n, int(iterations), float(delta), int(max_rounds),
                                               res.ctypes.data_as(C.c_void_p), C.byref(best),
                                               tr.ctypes.data_as(C.c_void_p) if trace else None, C.byref(rounds)),
                    "nid_multistart_lm")
        if trace:
            return res[:n], int(best.value), int(rounds.value), tr[:rounds.value, :n]
        return res[:n], int(best.value), int(rounds.value)

    def repair_count(self, reset=False):
        """(cell, pose) evaluations that ran the fold's repair pass (kLinFlagW in csrc/nid_kernels.hip.h)."""
        if not hasattr(self.lib, "nid_debug_repair_count"):
            return -1
        n = C.c_int64(0)
        self._check(self.lib.nid_debug_repair_count(self.h, C.byref(n), 1 if reset else 0), "nid_debug_repair_count")
        return int(n.value)

    # ---- debug ----------------------------------------------------------------
    def enable_pixel_dump(self, on=True):
        """True / 1: cost-phase dump (u, v, ic, jc, wc); 2: Jacobian-phase dump (gx, gy, pc, jc, dw in the same arrays)."""
        self._check(self.lib.nid_debug_enable_pixel_dump(self.h, int(on)), "nid_debug_enable_pixel_dump")

    def enable_stamps(self, on=True):
        self._check(self.lib.nid_debug_enable_stamps(self.h, 1 if on else 0), "nid_debug_enable_stamps")

    def stamps(self):
        n = self.cell_end - self.cell_begin
        out = np.zeros((n, 10), dtype=np.int64)
        self._check(self.lib.nid_debug_get_stamps(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))), "nid_debug_get_stamps")
        return out

    def pixel_dump(self):
        N = self.rows * self.cols
        u = np.zeros(N); v = np.zeros(N); ic = np.zeros(N)
        jc = np.zeros(N, dtype=np.int32); wc = np.zeros((N, 4))
        self._check(self.lib.nid_debug_get_pixel_dump(self.h, _dp(u), _dp(v), _dp(ic), _ip(jc), _dp(wc)),
                    "nid_debug_get_pixel_dump")
        return dict(u=u, v=v, ic=ic, jc=jc, wc=wc)


def unpack_reduced(r):
    lib = load()
    r = _d(r)
    H = np.zeros(36)
    b = np.zeros(6)
    chi2 = C.c_double(0)
    na = C.c_int32(0)
    lib.nid_unpack_reduced(_dp(r), _dp(H), _dp(b), C.byref(chi2), C.byref(na))
    return H.reshape(6, 6), b, chi2.value, na.value


def new_ms_state(pose7, iterations, xform=XFORM_QUAT):
    """A fresh chain for lm_step_host."""
    st = MsState()
    st.pose7[:] = [float(v) for v in pose7]
    st.iterations = int(iterations)
    st.xform_mode = int(xform)
    return st


def lm_step_host(state, reduced32):
    """One step of one LM chain on the host (nid_lm_step_host: the function k_lm_step runs, compiled for the host) with
    the reduced block of the pose the chain asked for.  True while the chain is running."""
    r = _d(reduced32)
    assert r.size == NID_REDUCED_LEN
    rc = load().nid_lm_step_host(C.byref(state), _dp(r))
    if rc < 0:
        raise NidError(f"nid_lm_step_host: {rc}")
    return bool(rc)


def lm_step_device(states, reduced32, ctx, rec19, rec_mode, trace=True):
    """One launch of k_lm_step over caller-given chains on ctx (nid_lm_step_device).  states: a ctypes array of MsState, stepped
    in place; reduced32 [n, 32]; rec19 [n, 19] float64 and rec_mode [n] int32: the pose records as handed to the kernel,
    replaced by what it left.  Returns (running word, trace): trace an MS_TRACE_DTYPE array [n], or None."""
    n = len(states)
    r = _d(reduced32)
    assert r.size == n * NID_REDUCED_LEN and rec19.dtype == np.float64 and rec19.size == n * 19 and rec19.flags.c_contiguous
    assert rec_mode.dtype == np.int32 and rec_mode.size == n and rec_mode.flags.c_contiguous
    tr = np.zeros(max(n, 1), dtype=MS_TRACE_DTYPE) if trace else None
    word = C.c_uint32(0)
    ctx._check(ctx.lib.nid_lm_step_device(ctx.h, states, _dp(r), n, _dp(rec19), _ip(rec_mode),
                                          tr.ctypes.data_as(C.c_void_p) if trace else None, C.byref(word)), "nid_lm_step_device")
    return int(word.value), (tr[:n] if trace else None)


def log2_fast_host(x):
    lib = load()
    lib.nid_log2_fast_host.restype = C.c_double
    lib.nid_log2_fast_host.argtypes = [C.c_double]
    return float(lib.nid_log2_fast_host(float(x)))


def bspline4_poly_host(u, bin_num):
    B = np.zeros(4)
    D = np.zeros(4)
    load().nid_bspline4_poly_host(float(u), int(bin_num), _dp(B), _dp(D))
    return B, D


def bspline4_host(u, bin_num):
    B = np.zeros(4)
    D = np.zeros(4)
    load().nid_bspline4_host(float(u), int(bin_num), _dp(B), _dp(D))
    return B, D


def from_pair(pair, bin_num, device=0, cell_begin=0, cell_end=0, jac_bound=JACBOUND_CPU, xform=XFORM_QUAT,
              math=MATH_FAST, cell_stride=1):
    """Context set up like the reference's main() (NID_pose_estimation.cpp:253-257):
    back-projection (on the device) + target image; the caller runs compute_href."""
    import importlib
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    ctx = Context(pair.rows, pair.cols, pair.cell, bin_num, pair.fx, pair.fy, pair.cx, pair.cy, device=device,
                  cell_begin=cell_begin, cell_end=cell_end, jac_bound=jac_bound, xform=xform, cell_stride=cell_stride)
    ctx.set_math_mode(math)
    ctx.set_reference_depth(pair.depth_m, pair.im0, synth.matrix_colmajor16(pair.T_wc0))
    ctx.set_target(pair.im1)
    return ctx


# ---------------------------------------------------------------------------------------------------------------
# include/nid/nid_pyr.h: a device-built resident pyramid, coarse-to-fine multi-start LM on it
def pyr_level_config(cfg0, level):
    """nid_pyr_level_config: the NidConfig of pyramid level `level` of cfg0 (pure arithmetic, no device)."""
    lib = load()
    out = NidConfig()
    rc = lib.nid_pyr_level_config(C.byref(cfg0) if cfg0 is not None else None, int(level), C.byref(out))
    if rc != NID_OK:
        raise NidError(f"nid_pyr_level_config(level {level}): {lib.nid_status_string(rc).decode()} ({rc})")
    return out


class Pyramid:
    """One frame pair on every level of a pyramid that is built and kept on the device (nid_pyr)."""

    def __init__(self, rows, cols, cell_num, bin_num, fx, fy, cx, cy, levels=3, device=0):
        self.lib = load()
        self.cfg0 = NidConfig(rows, cols, cell_num, bin_num, 3, device, 0, 0, fx, fy, cx, cy)
        h = C.c_void_p()
        rc = self.lib.nid_pyr_create(C.byref(self.cfg0), int(levels), C.byref(h))
        if rc != NID_OK:
            raise NidError(f"nid_pyr_create: {self.lib.nid_status_string(rc).decode()} ({rc})")
        self.h = h
        self.levels = int(self.lib.nid_pyr_levels(self.h))
        self.bin_num = bin_num

    @classmethod
    def create(cls, pair, bin_num, levels=3, device=0):
        return cls(pair.rows, pair.cols, pair.cell, bin_num, pair.fx, pair.fy, pair.cx, pair.cy, levels=levels, device=device)

    def _check(self, rc, what):
        if rc != NID_OK:
            c0 = self.lib.nid_pyr_level(self.h, 0) if self.h else None
            msg = self.lib.nid_last_error(c0).decode() if c0 else ""
            raise NidError(f"{what}: {self.lib.nid_status_string(rc).decode()} ({rc}) {msg}")

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):   # (a Tracker's pyramid is the tracker's)
                self.lib.nid_pyr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def level_config(self, level):
        return pyr_level_config(self.cfg0, level)

    def level(self, level):
        """Level `level`'s context as a Context (not owned: closing it does nothing; it keeps this Pyramid alive)."""
        c = self.level_config(level)
        ctx = Context.__new__(Context)
        ctx.lib = self.lib
        ctx.h = C.c_void_p(self.lib.nid_pyr_level(self.h, int(level)))
        if not ctx.h:
            raise NidError(f"nid_pyr_level({level}): no such level")
        ctx._borrowed = True
        ctx._owner = self
        ctx.rows, ctx.cols, ctx.cell_num, ctx.bin_num = c.rows, c.cols, c.cell_num, c.bin_num
        ctx.ncell = c.cell_num * c.cell_num
        ctx.cell_begin, ctx.cell_end = 0, ctx.ncell
        return ctx

    def set_pair_u16(self, depth_u16, depth_factor, im0, im1, T_wc0_colmajor16):
        """nid_pyr_set_pair_u16: level 0 up, every coarser level made on the device, every level set up; no reference stage."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1)
        a, b, T = _u8(im0).reshape(-1), _u8(im1).reshape(-1), _d(T_wc0_colmajor16)
        N = self.cfg0.rows * self.cfg0.cols
        assert d.size == N and a.size == N and b.size == N and T.size == 16
        self._check(self.lib.nid_pyr_set_pair_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor),
                                                  a.ctypes.data_as(c_u8p), b.ctypes.data_as(c_u8p), _dp(T)), "nid_pyr_set_pair_u16")

    def set_target(self, im1):
        """nid_pyr_set_target_u8: a new target on every level; the reference side, its reference stage included, stays."""
        b = _u8(im1).reshape(-1)
        assert b.size == self.cfg0.rows * self.cfg0.cols
        self._check(self.lib.nid_pyr_set_target_u8(self.h, b.ctypes.data_as(c_u8p)), "nid_pyr_set_target_u8")

    def promote_target(self, depth_u16, depth_factor, T_wc_colmajor16):
        """nid_pyr_promote_target_u16: the resident target becomes the reference, with its depth and camera-to-world matrix."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1)
        T = _d(T_wc_colmajor16)
        assert d.size == self.cfg0.rows * self.cfg0.cols and T.size == 16
        self._check(self.lib.nid_pyr_promote_target_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor), _dp(T)),
                    "nid_pyr_promote_target_u16")

    def set_target_depth(self, depth_u16, depth_factor=1.0 / 5000):
        """nid_pyr_set_target_depth_u16: the resident target's depth map, kept at level 0 (nid_keyframe.h)."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1)
        assert d.size == self.cfg0.rows * self.cfg0.cols
        self._check(self.lib.nid_pyr_set_target_depth_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor)),
                    "nid_pyr_set_target_depth_u16")

    def promote_resident_target(self, T_wc_colmajor16):
        """nid_pyr_promote_target: promote_target with the resident target depth, copied on the device."""
        T = _d(T_wc_colmajor16)
        assert T.size == 16
        self._check(self.lib.nid_pyr_promote_target(self.h, _dp(T)), "nid_pyr_promote_target")

    def depth_check(self, poses, tol_abs=0.01, tol_rel=0.02, cells=True):
        """nid_pyr_depth_check: (totals [n] DEPTH_COUNTS_DTYPE, cells [n, cells of level 0] DEPTH_CELL_DTYPE or None)."""
        p = _d(np.asarray(poses).reshape(-1, 7))
        n = p.shape[0]
        ncell = self.cfg0.cell_num * self.cfg0.cell_num
        tot = np.zeros(max(n, 1), dtype=DEPTH_COUNTS_DTYPE)
        cel = np.zeros((max(n, 1), ncell), dtype=DEPTH_CELL_DTYPE) if cells else None
        self._check(self.lib.nid_pyr_depth_check(self.h, _dp(p), n, float(tol_abs), float(tol_rel), tot.ctypes.data_as(C.c_void_p),
                                                 cel.ctypes.data_as(C.c_void_p) if cells else None), "nid_pyr_depth_check")
        return tot[:n], (cel[:n] if cells else None)

    def set_reference_mask(self, mask):
        """nid_pyr_set_reference_mask_u8: the caller's bit from mask != 0, the derived bits cleared, the reference rebuilt."""
        m = _u8(mask).reshape(-1)
        assert m.size == self.cfg0.rows * self.cfg0.cols
        self._check(self.lib.nid_pyr_set_reference_mask_u8(self.h, m.ctypes.data_as(c_u8p)), "nid_pyr_set_reference_mask_u8")

    def mask_occluded(self, pose7, tol_abs=0.01, tol_rel=0.02, classes=REFMASK_OCCLUDED | REFMASK_THROUGH, dilate=0, accumulate=False):
        """nid_pyr_mask_occluded: the counts as a REFMASK_COUNTS_DTYPE record."""
        q = _d(pose7)
        assert q.size == 7
        n = np.zeros(1, dtype=REFMASK_COUNTS_DTYPE)
        self._check(self.lib.nid_pyr_mask_occluded(self.h, _dp(q), float(tol_abs), float(tol_rel), int(classes), int(dilate), int(accumulate),
                                                   n.ctypes.data_as(C.c_void_p)), "nid_pyr_mask_occluded")
        return n[0]

    def clear_reference_mask(self):
        self._check(self.lib.nid_pyr_clear_reference_mask(self.h), "nid_pyr_clear_reference_mask")

    def get_reference_mask(self):
        """nid_pyr_get_reference_mask_u8: the plane (rows x cols of level 0) as the device holds it."""
        m = np.zeros((self.cfg0.rows, self.cfg0.cols), dtype=np.uint8)
        self._check(self.lib.nid_pyr_get_reference_mask_u8(self.h, m.ctypes.data_as(c_u8p)), "nid_pyr_get_reference_mask_u8")
        return m

    def fill_reference_depth(self, pose7, guard=1, guard_abs=50, guard_rel_1024=20, accumulate=False):
        """nid_pyr_fill_reference_depth: the counts as a REFFILL_COUNTS_DTYPE record."""
        q = _d(pose7)
        assert q.size == 7
        n = np.zeros(1, dtype=REFFILL_COUNTS_DTYPE)
        self._check(self.lib.nid_pyr_fill_reference_depth(self.h, _dp(q), int(guard), int(guard_abs), int(guard_rel_1024), int(accumulate),
                                                          n.ctypes.data_as(C.c_void_p)), "nid_pyr_fill_reference_depth")
        return n[0]

    def clear_reference_fill(self):
        self._check(self.lib.nid_pyr_clear_reference_fill(self.h), "nid_pyr_clear_reference_fill")

    def get_reference_fill(self):
        """nid_pyr_get_reference_fill_u16: the plane (rows x cols of level 0) as the device holds it."""
        f = np.zeros((self.cfg0.rows, self.cfg0.cols), dtype=np.uint16)
        self._check(self.lib.nid_pyr_get_reference_fill_u16(self.h, f.ctypes.data_as(C.POINTER(C.c_uint16))), "nid_pyr_get_reference_fill_u16")
        return f

    def fuse_reference_depth(self, pose7, gate_abs=50, gate_rel_1024=20, max_obs=255):
        """nid_pyr_fuse_reference_depth (nid_reffuse.h): the counts as a REFFUSE_COUNTS_DTYPE record."""
        q = _d(pose7)
        assert q.size == 7
        n = np.zeros(1, dtype=REFFUSE_COUNTS_DTYPE)
        self._check(self.lib.nid_pyr_fuse_reference_depth(self.h, _dp(q), int(gate_abs), int(gate_rel_1024), int(max_obs),
                                                          n.ctypes.data_as(C.c_void_p)), "nid_pyr_fuse_reference_depth")
        return n[0]

    def fuse_reference_depth_bilinear(self, pose7, gate_abs=50, gate_rel_1024=20, max_obs=255, tap_abs=50, tap_rel_1024=20):
        """nid_pyr_fuse_reference_depth_bilinear (nid_refgather.h): the counts as a REFGATHER_COUNTS_DTYPE record."""
        q = _d(pose7)
        assert q.size == 7
        n = np.zeros(1, dtype=REFGATHER_COUNTS_DTYPE)
        self._check(self.lib.nid_pyr_fuse_reference_depth_bilinear(self.h, _dp(q), int(gate_abs), int(gate_rel_1024), int(max_obs), int(tap_abs),
                                                                   int(tap_rel_1024), n.ctypes.data_as(C.c_void_p)),
                    "nid_pyr_fuse_reference_depth_bilinear")
        return n[0]

    def clear_reference_fusion(self):
        self._check(self.lib.nid_pyr_clear_reference_fusion(self.h), "nid_pyr_clear_reference_fusion")

    def get_reference_fused(self):
        """nid_pyr_get_reference_fused_u16: the FUSED plane (rows x cols of level 0) as the device holds it."""
        f = np.zeros((self.cfg0.rows, self.cfg0.cols), dtype=np.uint16)
        self._check(self.lib.nid_pyr_get_reference_fused_u16(self.h, f.ctypes.data_as(C.POINTER(C.c_uint16))), "nid_pyr_get_reference_fused_u16")
        return f

    def get_reference_fusion_obs(self):
        """nid_pyr_get_reference_fusion_obs_u8: the OBS plane likewise."""
        k = np.zeros((self.cfg0.rows, self.cfg0.cols), dtype=np.uint8)
        self._check(self.lib.nid_pyr_get_reference_fusion_obs_u8(self.h, k.ctypes.data_as(c_u8p)), "nid_pyr_get_reference_fusion_obs_u8")
        return k

    def get_level_inputs(self, level):
        """(depth_u16, im0, im1) of a level as the device holds them."""
        c = self.level_config(level)
        dep = np.zeros((c.rows, c.cols), dtype=np.uint16)
        a = np.zeros((c.rows, c.cols), dtype=np.uint8)
        b = np.zeros((c.rows, c.cols), dtype=np.uint8)
        self._check(self.lib.nid_pyr_get_level_inputs(self.h, int(level), dep.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                      a.ctypes.data_as(c_u8p), b.ctypes.data_as(c_u8p)), "nid_pyr_get_level_inputs")
        return dep, a, b

    def multistart_lm(self, poses, iterations, delta, pose_ref=None, keep=None):
        """nid_pyr_multistart_lm.  Returns (results [levels, n] MS_RESULT_DTYPE, origin [levels, n] int32, rounds [levels],
        best_origin, best_pose7), coarsest level first."""
        p = _d(np.asarray(poses).reshape(-1, 7))
        n = p.shape[0]
        L = self.levels
        res = np.zeros((L, max(n, 1)), dtype=MS_RESULT_DTYPE)
        origin = np.full((L, max(n, 1)), -1, dtype=np.int32)
        rounds = np.zeros(L, dtype=np.int32)
        best_pose = np.zeros(7)
        best = C.c_int32(-2)
        ref = _d(pose_ref) if pose_ref is not None else None
        kp = None
        if keep is not None:
            kp = np.ascontiguousarray(keep, dtype=np.int32)
            assert kp.size == L, "keep: one entry per level, keep[l] = chains that start on level l"
        self._check(self.lib.nid_pyr_multistart_lm(self.h, _dp(p), n, _dp(ref), int(iterations), float(delta), _ip(kp),
                                                   res.ctypes.data_as(C.c_void_p), _ip(origin), _ip(rounds), C.byref(best),
                                                   _dp(best_pose)), "nid_pyr_multistart_lm")
        return res[:, :n], origin[:, :n], rounds, int(best.value), best_pose


def pyramid_from_pair(pair, bin_num, levels=3, device=0, depth_factor=1.0 / 5000):
    """A Pyramid holding `pair` on every level (no reference stage: the caller runs compute_href per level)."""
    import importlib
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    pyr = Pyramid.create(pair, bin_num, levels=levels, device=device)
    pyr.set_pair_u16(pair.depth_u16, depth_factor, pair.im0, pair.im1, synth.matrix_colmajor16(pair.T_wc0))
    return pyr


# ---------------------------------------------------------------------------------------------------------------
# include/nid/nid_pyr_stream.h: the pose arithmetic of a sequence (no device) and the tracker
def _pose_call(name, out_len, *args):
    lib = load()
    a = [_d(x) for x in args]
    out = np.zeros(out_len)
    rc = getattr(lib, name)(*[_dp(x) for x in a], _dp(out))
    if rc != NID_OK:
        raise NidError(f"{name}: {lib.nid_status_string(rc).decode()} ({rc})")
    return out


def pose_inverse(pose7):
    return _pose_call("nid_track_pose_inverse", 7, pose7)


def pose_compose(a7, b7):
    """a o b (b applied first), renormalised, w >= 0"""
    return _pose_call("nid_track_pose_compose", 7, a7, b7)


def pose_perturb(pose7, twist6):
    """exp(twist) o pose, twist = (omega, upsilon): the LM chains' update"""
    return _pose_call("nid_track_pose_perturb", 7, pose7, twist6)


def pose_to_Twc16(pose7_cw):
    """world -> camera pose7 -> column-major camera -> world matrix (what set_pair_u16 / promote_target take)"""
    return _pose_call("nid_track_pose_to_Twc16", 16, pose7_cw)


def pose_from_Twc16(T_wc_colmajor16):
    return _pose_call("nid_track_pose_from_Twc16", 7, T_wc_colmajor16)


class Tracker:
    """A frame sequence on a resident pyramid of its own (nid_track): push() is the schedule of nid_pyr_stream.h."""

    def __init__(self, rows, cols, cell_num, bin_num, fx, fy, cx, cy, levels=3, device=0):
        self.lib = load()
        self.cfg0 = NidConfig(rows, cols, cell_num, bin_num, 3, device, 0, 0, fx, fy, cx, cy)
        h = C.c_void_p()
        rc = self.lib.nid_track_create(C.byref(self.cfg0), int(levels), C.byref(h))
        if rc != NID_OK:
            raise NidError(f"nid_track_create: {self.lib.nid_status_string(rc).decode()} ({rc})")
        self.h = h
        # the tracker's pyramid as a Pyramid (not owned: closing it does nothing; it keeps this Tracker alive)
        pyr = Pyramid.__new__(Pyramid)
        pyr.lib, pyr.cfg0, pyr.bin_num = self.lib, self.cfg0, bin_num
        pyr.h = C.c_void_p(self.lib.nid_track_pyramid(self.h))
        pyr.levels = int(self.lib.nid_pyr_levels(pyr.h))
        pyr._borrowed = True
        pyr._owner = self
        self.pyramid = pyr
        self.levels = pyr.levels

    @classmethod
    def create(cls, pair, bin_num, levels=3, device=0):
        return cls(pair.rows, pair.cols, pair.cell, bin_num, pair.fx, pair.fy, pair.cx, pair.cy, levels=levels, device=device)

    def _check(self, rc, what):
        if rc != NID_OK:
            c0 = self.lib.nid_pyr_level(self.pyramid.h, 0) if self.h else None
            msg = self.lib.nid_last_error(c0).decode() if c0 else ""
            raise NidError(f"{what}: {self.lib.nid_status_string(rc).decode()} ({rc}) {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.pyramid.h = None
            self.lib.nid_track_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lm(self, iterations, delta, keep=None):
        kp = None
        if keep is not None:
            kp = np.ascontiguousarray(keep, dtype=np.int32)
            assert kp.size == self.levels, "keep: one entry per level"
        self._check(self.lib.nid_track_set_lm(self.h, int(iterations), float(delta), _ip(kp)), "nid_track_set_lm")

    def set_twists(self, twists6):
        tw = _d(np.asarray(twists6, dtype=np.float64).reshape(-1, 6))
        self._check(self.lib.nid_track_set_twists(self.h, _dp(tw) if tw.shape[0] else None, tw.shape[0]), "nid_track_set_twists")

    def set_pose(self, pose7):
        p = _d(pose7)
        assert p.size == 7
        self._check(self.lib.nid_track_set_pose(self.h, _dp(p)), "nid_track_set_pose")

    def set_policy(self, policy):
        """nid_track_set_policy (a TrackPolicy, e.g. track_policy_default() with members changed)"""
        self._check(self.lib.nid_track_set_policy(self.h, C.byref(policy)), "nid_track_set_policy")

    def last_check(self):
        """nid_track_last_check: (chosen candidate's counts as a DEPTH_COUNTS_DTYPE record, poses checked, age)"""
        chosen = np.zeros(1, dtype=DEPTH_COUNTS_DTYPE)
        n, age = C.c_int32(-1), C.c_int32(-1)
        self._check(self.lib.nid_track_last_check(self.h, chosen.ctypes.data_as(C.c_void_p), C.byref(n), C.byref(age)), "nid_track_last_check")
        return chosen[0], int(n.value), int(age.value)

    def set_masking(self, classes, dilate=0):
        """nid_track_set_masking (nid_refmask.h): classes 0 is off"""
        self._check(self.lib.nid_track_set_masking(self.h, int(classes), int(dilate)), "nid_track_set_masking")

    def last_mask(self):
        """nid_track_last_mask: the counts of the last push's step 5e as a REFMASK_COUNTS_DTYPE record (zeros: it ran none)"""
        n = np.zeros(1, dtype=REFMASK_COUNTS_DTYPE)
        self._check(self.lib.nid_track_last_mask(self.h, n.ctypes.data_as(C.c_void_p)), "nid_track_last_mask")
        return n[0]

    def set_filling(self, on, guard=1, guard_abs=50, guard_rel_1024=20):
        """nid_track_set_filling (nid_reffill.h): off by default"""
        self._check(self.lib.nid_track_set_filling(self.h, int(on), int(guard), int(guard_abs), int(guard_rel_1024)), "nid_track_set_filling")

    def last_fill(self):
        """nid_track_last_fill: the counts of the last push's fill as a REFFILL_COUNTS_DTYPE record (zeros: it ran none)"""
        n = np.zeros(1, dtype=REFFILL_COUNTS_DTYPE)
        self._check(self.lib.nid_track_last_fill(self.h, n.ctypes.data_as(C.c_void_p)), "nid_track_last_fill")
        return n[0]

    def set_fusing(self, on, gate_abs=50, gate_rel_1024=20, max_obs=255):
        """nid_track_set_fusing (nid_reffuse.h): off by default"""
        self._check(self.lib.nid_track_set_fusing(self.h, int(on), int(gate_abs), int(gate_rel_1024), int(max_obs)), "nid_track_set_fusing")

    def last_fusion(self):
        """nid_track_last_fusion: the counts of the last push's fusion as a REFFUSE_COUNTS_DTYPE record (zeros: it ran none)"""
        n = np.zeros(1, dtype=REFFUSE_COUNTS_DTYPE)
        self._check(self.lib.nid_track_last_fusion(self.h, n.ctypes.data_as(C.c_void_p)), "nid_track_last_fusion")
        return n[0]

    def set_fusion_sampling(self, mode, tap_abs=50, tap_rel_1024=20):
        """nid_track_set_fusion_sampling (nid_refgather.h): REFFUSE_NEAREST by default"""
        self._check(self.lib.nid_track_set_fusion_sampling(self.h, int(mode), int(tap_abs), int(tap_rel_1024)), "nid_track_set_fusion_sampling")

    def last_gather(self):
        """nid_track_last_gather: the counts of the last push's gather as a REFGATHER_COUNTS_DTYPE record (zeros: it ran none)"""
        n = np.zeros(1, dtype=REFGATHER_COUNTS_DTYPE)
        self._check(self.lib.nid_track_last_gather(self.h, n.ctypes.data_as(C.c_void_p)), "nid_track_last_gather")
        return n[0]

    def push(self, im, depth_u16=None, depth_factor=1.0 / 5000, T_wc_first=None):
        """nid_track_push_u16: one frame.  Returns a dict of nid_track_result's members (pose7 and rounds as arrays)."""
        N = self.cfg0.rows * self.cfg0.cols
        a = _u8(im).reshape(-1)
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1) if depth_u16 is not None else None
        T = _d(T_wc_first) if T_wc_first is not None else None
        assert a.size == N and (d is None or d.size == N) and (T is None or T.size == 16)
        r = TrackResult()
        self._check(self.lib.nid_track_push_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)) if d is not None else None,
                                                float(depth_factor), a.ctypes.data_as(c_u8p), _dp(T), C.byref(r)), "nid_track_push_u16")
        return dict(pose7=np.array(r.pose7[:]), chi2=float(r.chi2), n_active=int(r.n_active), best_origin=int(r.best_origin),
                    status=int(r.status), promoted=int(r.promoted), frame=int(r.frame),
                    rounds=np.array(r.rounds[:self.levels], dtype=np.int32))


# ---------------------------------------------------------------------------------------------------------------
# include/nid/nid_keyframe.h: the host build of the depth-consistency check (no device) and the default policy
def track_policy_default():
    lib = load()
    pol = TrackPolicy()
    rc = lib.nid_track_policy_default(C.byref(pol))
    if rc != NID_OK:
        raise NidError(f"nid_track_policy_default: {rc}")
    return pol


def depth_check_host(cfg, points3d, depth1_u16, depth_factor, pose7, tol_abs=0.01, tol_rel=0.02):
    """nid_depth_check_host over nid_get_points3d's layout: (total as a DEPTH_COUNTS_DTYPE record, cells [cell_num^2]
    DEPTH_CELL_DTYPE) -- what k_depth_check computes, from the same text compiled for the host."""
    lib = load()
    pts = _d(points3d).reshape(-1)
    d = np.ascontiguousarray(depth1_u16, dtype=np.uint16).reshape(-1)
    q = _d(pose7)
    assert pts.size == 3 * cfg.rows * cfg.cols and d.size == cfg.rows * cfg.cols and q.size == 7
    tot = np.zeros(1, dtype=DEPTH_COUNTS_DTYPE)
    cel = np.zeros(cfg.cell_num * cfg.cell_num, dtype=DEPTH_CELL_DTYPE)
    rc = lib.nid_depth_check_host(C.byref(cfg), _dp(pts), d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor), _dp(q),
                                  float(tol_abs), float(tol_rel), tot.ctypes.data_as(C.c_void_p), cel.ctypes.data_as(C.c_void_p))
    if rc != NID_OK:
        raise NidError(f"nid_depth_check_host: {lib.nid_status_string(rc).decode()} ({rc})")
    return tot[0], cel


def refmask_host(cfg, depth0_u16, factor0, T_wc_colmajor16, depth1_u16, factor1, pose7, tol_abs=0.01, tol_rel=0.02,
                 classes=REFMASK_OCCLUDED | REFMASK_THROUGH, dilate=0, accumulate=False, mask=None):
    """nid_refmask_host (nid_refmask.h): one call of the rule on a copy of `mask` (None: zeros): (plane [rows, cols] u8,
    counts as a REFMASK_COUNTS_DTYPE record) -- what nid_pyr_mask_occluded computes, from the same text compiled for the host."""
    lib = load()
    N = cfg.rows * cfg.cols
    u16p = C.POINTER(C.c_uint16)
    d0 = np.ascontiguousarray(depth0_u16, dtype=np.uint16).reshape(-1)
    d1 = np.ascontiguousarray(depth1_u16, dtype=np.uint16).reshape(-1)
    T, q = _d(T_wc_colmajor16), _d(pose7)
    m = np.zeros(N, dtype=np.uint8) if mask is None else np.array(mask, dtype=np.uint8).reshape(-1)
    assert d0.size == N and d1.size == N and m.size == N and T.size == 16 and q.size == 7
    n = np.zeros(1, dtype=REFMASK_COUNTS_DTYPE)
    rc = lib.nid_refmask_host(C.byref(cfg), d0.ctypes.data_as(u16p), float(factor0), _dp(T), d1.ctypes.data_as(u16p), float(factor1), _dp(q),
                              float(tol_abs), float(tol_rel), int(classes), int(dilate), int(accumulate), m.ctypes.data_as(c_u8p),
                              n.ctypes.data_as(C.c_void_p))
    if rc != NID_OK:
        raise NidError(f"nid_refmask_host: {lib.nid_status_string(rc).decode()} ({rc})")
    return m.reshape(cfg.rows, cfg.cols), n[0]


def reffill_host(cfg, depth0_u16, factor0, T_wc_colmajor16, depth1_u16, factor1, pose7, guard=1, guard_abs=50, guard_rel_1024=20,
                 accumulate=False, fill=None):
    """nid_reffill_host (nid_reffill.h): one call of the rule on a copy of `fill` (None: zeros): (plane [rows, cols] u16,
    counts as a REFFILL_COUNTS_DTYPE record) -- what nid_pyr_fill_reference_depth computes, from the same text compiled for
    the host."""
    lib = load()
    N = cfg.rows * cfg.cols
    u16p = C.POINTER(C.c_uint16)
    d0 = np.ascontiguousarray(depth0_u16, dtype=np.uint16).reshape(-1)
    d1 = np.ascontiguousarray(depth1_u16, dtype=np.uint16).reshape(-1)
    T, q = _d(T_wc_colmajor16), _d(pose7)
    f = np.zeros(N, dtype=np.uint16) if fill is None else np.array(fill, dtype=np.uint16).reshape(-1)
    assert d0.size == N and d1.size == N and f.size == N and T.size == 16 and q.size == 7
    n = np.zeros(1, dtype=REFFILL_COUNTS_DTYPE)
    rc = lib.nid_reffill_host(C.byref(cfg), d0.ctypes.data_as(u16p), float(factor0), _dp(T), d1.ctypes.data_as(u16p), float(factor1), _dp(q),
                              int(guard), int(guard_abs), int(guard_rel_1024), int(accumulate), f.ctypes.data_as(u16p),
                              n.ctypes.data_as(C.c_void_p))
    if rc != NID_OK:
        raise NidError(f"nid_reffill_host: {lib.nid_status_string(rc).decode()} ({rc})")
    return f.reshape(cfg.rows, cfg.cols), n[0]


def reffuse_host(cfg, depth0_u16, factor0, T_wc_colmajor16, depth1_u16, factor1, pose7, gate_abs=50, gate_rel_1024=20, max_obs=255,
                 sums=None, obs=None):
    """nid_reffuse_host (nid_reffuse.h): one call of the rule on copies of `sums` and `obs` (None: zeros): (SUM plane
    [rows, cols] u32, OBS plane u8, FUSED plane u16, counts as a REFFUSE_COUNTS_DTYPE record) -- what
    nid_pyr_fuse_reference_depth computes, from the same text compiled for the host."""
    lib = load()
    N = cfg.rows * cfg.cols
    u16p = C.POINTER(C.c_uint16)
    d0 = np.ascontiguousarray(depth0_u16, dtype=np.uint16).reshape(-1)
    d1 = np.ascontiguousarray(depth1_u16, dtype=np.uint16).reshape(-1)
    T, q = _d(T_wc_colmajor16), _d(pose7)
    s = np.zeros(N, dtype=np.uint32) if sums is None else np.array(sums, dtype=np.uint32).reshape(-1)
    k = np.zeros(N, dtype=np.uint8) if obs is None else np.array(obs, dtype=np.uint8).reshape(-1)
    f = np.zeros(N, dtype=np.uint16)
    assert d0.size == N and d1.size == N and s.size == N and k.size == N and T.size == 16 and q.size == 7
    n = np.zeros(1, dtype=REFFUSE_COUNTS_DTYPE)
    rc = lib.nid_reffuse_host(C.byref(cfg), d0.ctypes.data_as(u16p), float(factor0), _dp(T), d1.ctypes.data_as(u16p), float(factor1), _dp(q),
                              int(gate_abs), int(gate_rel_1024), int(max_obs), s.ctypes.data_as(C.POINTER(C.c_uint32)), k.ctypes.data_as(c_u8p),
                              f.ctypes.data_as(u16p), n.ctypes.data_as(C.c_void_p))
    if rc != NID_OK:
        raise NidError(f"nid_reffuse_host: {lib.nid_status_string(rc).decode()} ({rc})")
    shape = (cfg.rows, cfg.cols)
    return s.reshape(shape), k.reshape(shape), f.reshape(shape), n[0]


def refgather_host(cfg, depth0_u16, factor0, T_wc_colmajor16, depth1_u16, factor1, pose7, gate_abs=50, gate_rel_1024=20, max_obs=255,
                   tap_abs=50, tap_rel_1024=20, sums=None, obs=None):
    """nid_refgather_host (nid_refgather.h): one call of the rule on copies of `sums` and `obs` (None: zeros): (SUM plane
    [rows, cols] u32, OBS plane u8, FUSED plane u16, counts as a REFGATHER_COUNTS_DTYPE record) -- what
    nid_pyr_fuse_reference_depth_bilinear computes, from the same text compiled for the host."""
    lib = load()
    N = cfg.rows * cfg.cols
    u16p = C.POINTER(C.c_uint16)
    d0 = np.ascontiguousarray(depth0_u16, dtype=np.uint16).reshape(-1)
    d1 = np.ascontiguousarray(depth1_u16, dtype=np.uint16).reshape(-1)
    T, q = _d(T_wc_colmajor16), _d(pose7)
    s = np.zeros(N, dtype=np.uint32) if sums is None else np.array(sums, dtype=np.uint32).reshape(-1)
    k = np.zeros(N, dtype=np.uint8) if obs is None else np.array(obs, dtype=np.uint8).reshape(-1)
    f = np.zeros(N, dtype=np.uint16)
    assert d0.size == N and d1.size == N and s.size == N and k.size == N and T.size == 16 and q.size == 7
    n = np.zeros(1, dtype=REFGATHER_COUNTS_DTYPE)
    rc = lib.nid_refgather_host(C.byref(cfg), d0.ctypes.data_as(u16p), float(factor0), _dp(T), d1.ctypes.data_as(u16p), float(factor1), _dp(q),
                                int(gate_abs), int(gate_rel_1024), int(max_obs), int(tap_abs), int(tap_rel_1024),
                                s.ctypes.data_as(C.POINTER(C.c_uint32)), k.ctypes.data_as(c_u8p), f.ctypes.data_as(u16p), n.ctypes.data_as(C.c_void_p))
    if rc != NID_OK:
        raise NidError(f"nid_refgather_host: {lib.nid_status_string(rc).decode()} ({rc})")
    shape = (cfg.rows, cfg.cols)
    return s.reshape(shape), k.reshape(shape), f.reshape(shape), n[0]


# ---------------------------------------------------------------------------------------------------------------
# include/nid/nid_multi.h: cell shards over several GPUs (one process, or one process per GPU), in C++
REDUCE_HOST, REDUCE_RCCL, REDUCE_HOOK = 0, 1, 2
PARTITION_CONTIGUOUS, PARTITION_INTERLEAVED = 0, 1
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, c_dp, C.c_int64, C.c_void_p)
RCCL_ID_BYTES = 128
MULTI_SYMBOLS = [
    "nid_multi_cell_range", "nid_multi_cell_partition", "nid_multi_resident_pause", "nid_multi_create", "nid_multi_create_rank", "nid_multi_create_partitioned", "nid_multi_destroy", "nid_multi_last_error",
    "nid_multi_shards", "nid_multi_shard", "nid_multi_world", "nid_multi_comm_unique_id", "nid_comm_create_rank",
    "nid_comm_create_local", "nid_comm_destroy", "nid_comm_ranks", "nid_multi_attach_comm", "nid_multi_comm_init",
    "nid_multi_comm_init_local", "nid_multi_comm_ranks", "nid_multi_time_exchange", "nid_multi_set_exchange_hook", "nid_multi_set_reduce_mode",
    "nid_multi_set_options",
    "nid_multi_set_math_mode", "nid_multi_set_href_nan_markers", "nid_multi_set_block_threads", "nid_multi_set_launch_shape", "nid_multi_set_resident", "nid_multi_set_reference_depth",
    "nid_multi_set_reference_points", "nid_multi_set_target_u8", "nid_multi_set_pair_u16", "nid_multi_compute_href",
    "nid_multi_compute_href_matrix", "nid_multi_set_href_state", "nid_multi_evaluate", "nid_multi_evaluate_matrix",
    "nid_multi_normal_equations", "nid_multi_launch_batch", "nid_multi_launch_chain", "nid_multi_wait", "nid_multi_run_sequence",
    "nid_multi_contract_bytes",
]


def _load_multi():
    lib = load()
    if getattr(lib, "_multi_ready", False):
        return lib
    vp = C.c_void_p
    lib.nid_multi_cell_range.argtypes = [C.c_int32] * 3 + [c_ip, c_ip]
    if hasattr(lib, "nid_multi_cell_partition"):
        lib.nid_multi_cell_partition.argtypes = [C.c_int32] * 4 + [c_ip, c_ip, c_ip]
    lib.nid_multi_create.argtypes = [C.POINTER(NidConfig), c_ip, C.c_int32, C.POINTER(vp)]
    lib.nid_multi_create_rank.argtypes = [C.POINTER(NidConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.nid_multi_create_partitioned.argtypes = [C.POINTER(NidConfig), c_ip, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    lib.nid_multi_destroy.argtypes = [vp]
    lib.nid_multi_last_error.restype = C.c_char_p
    lib.nid_multi_last_error.argtypes = [vp]
    lib.nid_multi_shards.argtypes = [vp]
    lib.nid_multi_shard.restype = vp
    lib.nid_multi_shard.argtypes = [vp, C.c_int32]
    lib.nid_multi_comm_unique_id.argtypes = [c_u8p]
    lib.nid_multi_comm_init.argtypes = [vp, c_u8p]
    lib.nid_multi_comm_init_local.argtypes = [vp]
    lib.nid_multi_comm_ranks.argtypes = [vp, c_ip]
    lib.nid_multi_time_exchange.argtypes = [vp, C.c_int, C.c_int, c_fp]
    lib.nid_multi_set_reduce_mode.argtypes = [vp, C.c_int]
    lib.nid_multi_set_exchange_hook.argtypes = [vp, EXCHANGE_FN, vp]
    lib.nid_multi_set_options.argtypes = [vp, C.c_int, C.c_int]
    lib.nid_multi_set_math_mode.argtypes = [vp, C.c_int]
    lib.nid_multi_set_block_threads.argtypes = [vp, C.c_int]
    lib.nid_multi_set_reference_depth.argtypes = [vp, c_dp, c_u8p, c_dp]
    lib.nid_multi_set_target_u8.argtypes = [vp, c_u8p]
    lib.nid_multi_set_pair_u16.argtypes = [vp, C.POINTER(C.c_uint16), C.c_double, c_u8p, c_u8p, c_dp, c_dp, c_dp, c_ip, c_dp]
    lib.nid_multi_compute_href.argtypes = [vp, c_dp, c_ip, c_dp, c_dp, c_ip]
    lib.nid_multi_set_href_state.argtypes = [vp, c_ip, c_dp, c_dp, c_ip]
    lib.nid_multi_evaluate.argtypes = [vp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_dp]
    lib.nid_multi_normal_equations.argtypes = [vp, c_dp, C.c_int, C.c_double, c_dp, c_dp, c_dp, c_ip]
    lib.nid_multi_launch_batch.argtypes = [vp, C.c_int, C.c_int, c_dp, C.c_int, C.c_double]
    lib.nid_multi_launch_chain.argtypes = [vp, C.c_int, C.c_int, c_dp, C.c_int, C.c_double]
    lib.nid_multi_wait.argtypes = [vp, C.c_int, c_dp, c_dp, c_dp, c_ip]
    lib.nid_multi_run_sequence.argtypes = [vp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_dp]
    lib.nid_multi_contract_bytes.restype = C.c_int64
    lib.nid_multi_contract_bytes.argtypes = [vp]
    lib._multi_ready = True
    return lib


def cell_range(k, n, ncell):
    lib = _load_multi()
    lo, hi = C.c_int32(0), C.c_int32(0)
    rc = lib.nid_multi_cell_range(k, n, ncell, C.byref(lo), C.byref(hi))
    if rc != NID_OK:
        raise NidError(f"nid_multi_cell_range({k}, {n}, {ncell}): {lib.nid_status_string(rc).decode()}")
    return lo.value, hi.value


def cell_set(k, n, ncell, partition=0):
    """The cell ids shard k of n owns under `partition` (PARTITION_CONTIGUOUS / PARTITION_INTERLEAVED): the library's
    own arithmetic (nid_multi_cell_partition), no device needed."""
    lib = _load_multi()
    b, e, st = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = lib.nid_multi_cell_partition(k, n, ncell, int(partition), C.byref(b), C.byref(e), C.byref(st))
    if rc != NID_OK:
        raise NidError(f"nid_multi_cell_partition({k}, {n}, {ncell}, {partition}): {lib.nid_status_string(rc).decode()}")
    return np.arange(b.value, e.value, st.value)


def rccl_unique_id():
    """ncclGetUniqueId through the library (rank 0 of a multi-process job; 128 bytes)."""
    lib = _load_multi()
    buf = (C.c_uint8 * RCCL_ID_BYTES)()
    rc = lib.nid_multi_comm_unique_id(buf)
    if rc != NID_OK:
        raise NidError(f"nid_multi_comm_unique_id: {lib.nid_status_string(rc).decode()} ({rc})")
    return bytes(buf)


class Multi:
    """One frame pair on the cell shards of several GPUs: `devices` = one shard per entry in this process, or
    rank/world = this process's shard of a one-process-per-GPU job (then comm_init(id) before evaluating)."""

    def __init__(self, rows, cols, cell_num, bin_num, fx, fy, cx, cy, devices=(0,), rank=None, world=None,
                 jac_bound=JACBOUND_CPU, xform=XFORM_QUAT, partition=None):
        self.lib = _load_multi()
        cfg = NidConfig(rows, cols, cell_num, bin_num, 3, 0, 0, 0, fx, fy, cx, cy)
        h = C.c_void_p()
        if partition is not None:
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self.lib.nid_multi_create_partitioned(C.byref(cfg), _ip(dv), dv.size, int(rank or 0), int(world or 1),
                                                       int(partition), C.byref(h))
        elif world is not None:
            rc = self.lib.nid_multi_create_rank(C.byref(cfg), int(devices[0]), int(rank), int(world), C.byref(h))
        else:
            dv = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self.lib.nid_multi_create(C.byref(cfg), _ip(dv), dv.size, C.byref(h))
        if rc != NID_OK:
            raise NidError(f"nid_multi_create: {self.lib.nid_status_string(rc).decode()} ({rc})")
        self.h = h
        self.rows, self.cols, self.cell_num, self.bin_num = rows, cols, cell_num, bin_num
        self.ncell = cell_num * cell_num
        self._check(self.lib.nid_multi_set_options(self.h, jac_bound, xform), "nid_multi_set_options")

    def _check(self, rc, what):
        if rc != NID_OK:
            msg = self.lib.nid_multi_last_error(self.h).decode() if self.h else ""
            raise NidError(f"{what}: {self.lib.nid_status_string(rc).decode()} ({rc}) {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.nid_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shards(self):
        return int(self.lib.nid_multi_shards(self.h))

    def comm_init(self, id_bytes):
        buf = (C.c_uint8 * RCCL_ID_BYTES).from_buffer_copy(id_bytes)
        self._check(self.lib.nid_multi_comm_init(self.h, buf), "nid_multi_comm_init")

    def comm_init_local(self):
        self._check(self.lib.nid_multi_comm_init_local(self.h), "nid_multi_comm_init_local")

    def time_exchange(self, blocks, repeats=20):
        ms = C.c_float(0)
        self._check(self.lib.nid_multi_time_exchange(self.h, int(blocks), int(repeats), C.byref(ms)), "nid_multi_time_exchange")
        return float(ms.value)

    def comm_ranks(self):
        n = C.c_int32(0)
        self._check(self.lib.nid_multi_comm_ranks(self.h, C.byref(n)), "nid_multi_comm_ranks")
        return n.value

    def set_exchange_hook(self, fn):
        """fn(array) must replace the float64 array by its sum over all processes, in place (e.g. a gloo all_reduce)."""
        def _cb(ptr, count, _user):
            try:
                fn(np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception:
                return 1
        self._hook = EXCHANGE_FN(_cb)       # keep the trampoline alive
        self._check(self.lib.nid_multi_set_exchange_hook(self.h, self._hook, None), "nid_multi_set_exchange_hook")

    def set_reduce_mode(self, mode):
        self._check(self.lib.nid_multi_set_reduce_mode(self.h, int(mode)), "nid_multi_set_reduce_mode")

    def set_math_mode(self, mode):
        self._check(self.lib.nid_multi_set_math_mode(self.h, int(mode)), "nid_multi_set_math_mode")

    def set_block_threads(self, n):
        self._check(self.lib.nid_multi_set_block_threads(self.h, int(n)), "nid_multi_set_block_threads")

    def set_reference_depth(self, depth_m, im0, T_wc0_colmajor16):
        d, im, T = _d(depth_m).reshape(-1), _u8(im0).reshape(-1), _d(T_wc0_colmajor16)
        self._check(self.lib.nid_multi_set_reference_depth(self.h, _dp(d), im.ctypes.data_as(c_u8p), _dp(T)),
                    "nid_multi_set_reference_depth")

    def set_target(self, im1):
        im = _u8(im1).reshape(-1)
        self._check(self.lib.nid_multi_set_target_u8(self.h, im.ctypes.data_as(c_u8p)), "nid_multi_set_target_u8")

    def set_pair_u16(self, depth_u16, depth_factor, im0, im1, T_wc0_colmajor16, pose0, matrix=False):
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16).reshape(-1)
        a, b, T, p = _u8(im0).reshape(-1), _u8(im1).reshape(-1), _d(T_wc0_colmajor16), _d(pose0)
        cnt = np.zeros(self.ncell, dtype=np.int32)
        href = np.full(self.ncell, np.nan)
        self._check(self.lib.nid_multi_set_pair_u16(self.h, d.ctypes.data_as(C.POINTER(C.c_uint16)), float(depth_factor), a.ctypes.data_as(c_u8p),
                                                    b.ctypes.data_as(c_u8p), _dp(T), None if matrix else _dp(p), _dp(p) if matrix else None,
                                                    _ip(cnt), _dp(href)), "nid_multi_set_pair_u16")
        return cnt, href

    def compute_href(self, pose7, dump=False):
        cnt = np.zeros(self.ncell, dtype=np.int32)
        href = np.full(self.ncell, np.nan)
        N = self.rows * self.cols
        bsv = np.zeros((N, 4)) if dump else None
        bsi = np.zeros(N, dtype=np.int32) if dump else None
        self._check(self.lib.nid_multi_compute_href(self.h, _dp(_d(pose7)), _ip(cnt), _dp(href), _dp(bsv), _ip(bsi)),
                    "nid_multi_compute_href")
        return (cnt, href, bsv, bsi) if dump else (cnt, href)

    def set_href_state(self, cnt, href, bsv, bsi):
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        bsi = np.ascontiguousarray(bsi, dtype=np.int32)
        self._check(self.lib.nid_multi_set_href_state(self.h, _ip(cnt), _dp(_d(href)), _dp(_d(bsv)), _ip(bsi)),
                    "nid_multi_set_href_state")

    def evaluate(self, pose7, want_jac=True):
        Hc = np.full(self.ncell, np.nan)
        Hj = np.full(self.ncell, np.nan)
        err = np.full(self.ncell, np.nan)
        J = np.full((self.ncell, 6), np.nan) if want_jac else None
        self._check(self.lib.nid_multi_evaluate(self.h, _dp(_d(pose7)), 1 if want_jac else 0, _dp(Hc), _dp(Hj),
                                                _dp(err), _dp(J)), "nid_multi_evaluate")
        return Hc, Hj, err, J

    def normal_equations(self, pose7, delta, want_jac=True):
        H = np.zeros(36)
        b = np.zeros(6)
        chi2 = C.c_double(0)
        na = C.c_int32(0)
        self._check(self.lib.nid_multi_normal_equations(self.h, _dp(_d(pose7)), 1 if want_jac else 0, float(delta),
                                                        _dp(H), _dp(b), C.byref(chi2), C.byref(na)),
                    "nid_multi_normal_equations")
        return H.reshape(6, 6), b, chi2.value, na.value

    def launch_chain(self, first_slot, poses7, n_jac, delta):
        p = _d(np.asarray(poses7).reshape(-1, 7))
        self._check(self.lib.nid_multi_launch_chain(self.h, first_slot, p.shape[0], _dp(p), int(n_jac), float(delta)),
                    "nid_multi_launch_chain")

    def launch_batch(self, first_slot, poses7, delta, want_jac=True):
        p = _d(np.asarray(poses7).reshape(-1, 7))
        self._check(self.lib.nid_multi_launch_batch(self.h, first_slot, p.shape[0], _dp(p), 1 if want_jac else 0,
                                                    float(delta)), "nid_multi_launch_batch")

    def wait(self, slot):
        H = np.zeros(36)
        b = np.zeros(6)
        chi2 = C.c_double(0)
        na = C.c_int32(0)
        self._check(self.lib.nid_multi_wait(self.h, slot, _dp(H), _dp(b), C.byref(chi2), C.byref(na)), "nid_multi_wait")
        return H.reshape(6, 6), b, chi2.value, na.value

    def run_sequence(self, poses7, delta, batch=64, group=1, want_jac=True, collect=True):
        p = _d(np.asarray(poses7).reshape(-1, 7))
        out = np.zeros((p.shape[0], NID_REDUCED_LEN)) if collect else None
        self._check(self.lib.nid_multi_run_sequence(self.h, _dp(p), p.shape[0], int(batch), int(group),
                                                    1 if want_jac else 0, float(delta), _dp(out)),
                    "nid_multi_run_sequence")
        return out

    def contract_bytes(self):
        return int(self.lib.nid_multi_contract_bytes(self.h))


def multi_from_pair(pair, bin_num, devices=(0,), rank=None, world=None, jac_bound=JACBOUND_CPU, xform=XFORM_QUAT,
                    math=MATH_FAST, partition=None):
    import importlib
    synth = importlib.import_module("nid-pose-estimation_amd.synth")
    m = Multi(pair.rows, pair.cols, pair.cell, bin_num, pair.fx, pair.fy, pair.cx, pair.cy, devices=devices,
              rank=rank, world=world, jac_bound=jac_bound, xform=xform, partition=partition)
    m.set_math_mode(math)
    m.set_reference_depth(pair.depth_m, pair.im0, synth.matrix_colmajor16(pair.T_wc0))
    m.set_target(pair.im1)
    return m
