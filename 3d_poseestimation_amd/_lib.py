"""ctypes binding of libposelift.so (include/poselift.h).

The library is the product: there is no CPU or eager-torch fallback.  If the shared
object is missing, or an entry point reports an error, this module raises.
"""
import ctypes
import os

import torch  # noqa: F401  (loads torch's bundled HIP runtime first so the library binds to it)

_HERE = os.path.dirname(os.path.abspath(__file__))
# POSELIFT_LIB: another build of the same library (same-box A/B of two builds, tools/ab_env.py)
LIB_PATH = os.environ.get("POSELIFT_LIB") or os.path.join(_HERE, "csrc", "libposelift.so")

PL_F32, PL_BF16, PL_BF16X6, PL_F16X3 = 0, 1, 2, 3


# int gather(void* user, float* buf, int64_t floats_per_rank, void* stream)   (poselift.h: PLGatherFn)
GATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


class PLSync(ctypes.Structure):
    _fields_ = [("world", ctypes.c_int32), ("rank", ctypes.c_int32), ("gather", GATHER_FN),
                ("user", ctypes.c_void_p)]


class PLL1Term(ctypes.Structure):
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("da", ctypes.c_void_p), ("db", ctypes.c_void_p)]


L1_MAX_TERMS = 8


class PLDesc(ctypes.Structure):
    _fields_ = [
        ("in_dim", ctypes.c_int32), ("hidden", ctypes.c_int32), ("out_dim", ctypes.c_int32),
        ("num_stage", ctypes.c_int32), ("bn", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("p_dropout", ctypes.c_float), ("bn_eps", ctypes.c_float), ("bn_momentum", ctypes.c_float),
        ("reserved", ctypes.c_int32),
        ("params", ctypes.c_void_p), ("bn_running", ctypes.c_void_p), ("bn_batches", ctypes.c_void_p),
        ("sync", ctypes.POINTER(PLSync)),
        ("step_dev", ctypes.c_void_p),
        ("wplanes", ctypes.c_void_p), ("wplanes_valid", ctypes.c_int32), ("reserved2", ctypes.c_int32),
    ]


ADAMW_MAX_SEGS = 8


class PLAdamWSeg(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("numel", ctypes.c_int64), ("h", ctypes.c_void_p), ("l", ctypes.c_void_p)]


class PLAdamWPlanes(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int32), ("kind", ctypes.c_int32), ("scale", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("seg", PLAdamWSeg * ADAMW_MAX_SEGS)]


class PLEma(ctypes.Structure):
    _fields_ = [("e", ctypes.c_void_p), ("decay", ctypes.c_float), ("warmup", ctypes.c_int32), ("t0", ctypes.c_int64)]


class PLAdamWStep(ctypes.Structure):
    _fields_ = [("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("lr", ctypes.c_float), ("lr_dev", ctypes.c_void_p),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("t", ctypes.c_int64), ("t_dev", ctypes.c_void_p), ("ema", ctypes.POINTER(PLEma))]


CRIT_MSE, CRIT_L1, CRIT_SMOOTH_L1, CRIT_MPJPE = 0, 1, 2, 3


class PLCriterion(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("group", ctypes.c_int32), ("beta", ctypes.c_float), ("weights", ctypes.c_void_p)]


CRIT_HAS_SKELETON = 0x100
RHO_L1, RHO_MSE = 0, 1
SKELETON_MAX_JOINTS, SKELETON_MAX_BONES, SKELETON_MAX_PAIRS = 32, 31, 16


class PLSkeleton(ctypes.Structure):
    _fields_ = [("joints", ctypes.c_int32), ("bones", ctypes.c_int32), ("pairs", ctypes.c_int32), ("rho", ctypes.c_int32),
                ("bone_child", ctypes.c_void_p), ("bone_parent", ctypes.c_void_p), ("pair_a", ctypes.c_void_p),
                ("pair_b", ctypes.c_void_p), ("term_weights", ctypes.c_void_p), ("sub", ctypes.c_void_p), ("div", ctypes.c_void_p)]


class PLSkeletonCriterion(PLCriterion):
    """PLCriterion base; then the skeleton (poselift.h): byref() of one goes wherever a PLCriterion* does"""
    _fields_ = [("skeleton", ctypes.POINTER(PLSkeleton))]


CRIT_HAS_ROW_WEIGHTS = 0x200


class PLRowWeightsCriterion(PLSkeletonCriterion):
    """PLSkeletonCriterion sc; then row_weights (poselift.h): byref() of one goes wherever a PLCriterion* does"""
    _fields_ = [("row_weights", ctypes.c_void_p)]


class PLClipRecord(ctypes.Structure):
    _fields_ = [("norm", ctypes.c_float), ("coef", ctypes.c_float), ("finite", ctypes.c_uint32), ("skip", ctypes.c_uint32),
                ("skipped", ctypes.c_uint64)]


class PLGradRange(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_int64), ("hi", ctypes.c_int64)]


GRAD_NORM_MAX_RANGES = 1024


class PLPlanesEpilogue(ctypes.Structure):
    _fields_ = [("bias", ctypes.c_void_p), ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("resid", ctypes.c_void_p),
                ("relu", ctypes.c_int32), ("reserved", ctypes.c_int32), ("y_planes", ctypes.c_void_p)]


class PLPoseAug(ctypes.Structure):
    _fields_ = [("p_flip", ctypes.c_float), ("flip_offset", ctypes.c_float), ("max_rot", ctypes.c_float),
                ("scale_range", ctypes.c_float), ("max_shift", ctypes.c_float), ("jitter_sigma", ctypes.c_float),
                ("cx", ctypes.c_float), ("cy", ctypes.c_float), ("seed", ctypes.c_uint64)]


FRAME_U8, FRAME_F32 = 0, 1


class PLFrameWarp(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("src_dtype", ctypes.c_int32), ("C", ctypes.c_int32), ("N", ctypes.c_int64),
                ("Hs", ctypes.c_int64), ("Ws", ctypes.c_int64), ("src_idx", ctypes.c_void_p), ("row_id", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("out", ctypes.c_void_p), ("Ho", ctypes.c_int64), ("Wo", ctypes.c_int64),
                ("scale", ctypes.c_float), ("fill", ctypes.c_float), ("aug", ctypes.POINTER(PLPoseAug)),
                ("epoch", ctypes.c_uint64)]


CROP_BBOX, CROP_ROOT = 0, 1


class PLPoseCrop(ctypes.Structure):
    _fields_ = [("margin", ctypes.c_float), ("centre", ctypes.c_int32), ("min_side", ctypes.c_float),
                ("reserved", ctypes.c_int32), ("Hs", ctypes.c_int64), ("Ws", ctypes.c_int64)]


_c = ctypes
_P = ctypes.c_void_p
_D = ctypes.POINTER(PLDesc)
# name -> (restype, argtypes); one entry per declaration in include/poselift.h
SIGNATURES = {
    "pl_version": (_c.c_int, []),
    "pl_last_error": (_c.c_char_p, []),
    "pl_num_hidden": (_c.c_int64, [_D]),
    "pl_param_tensors": (_c.c_int64, [_D]),
    "pl_param_offset": (_c.c_int64, [_D, _c.c_int64]),
    "pl_param_numel": (_c.c_int64, [_D, _c.c_int64]),
    "pl_param_arena_floats": (_c.c_int64, [_D]),
    "pl_workspace_bytes": (_c.c_size_t, [_D, _c.c_int64]),
    "pl_workspace_view": (_c.c_int, [_D, _c.c_int64, _c.c_int, _c.c_int64,
                                     _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t)]),
    "pl_workspace_bitmap_format": (_c.c_int, [_D, _c.c_int64, _c.c_int64]),
    "pl_lifter_fwd_eval": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _P]),
    "pl_lifter_fwd_train": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _c.c_uint64,
                                       _c.c_uint64, _P, _P]),
    "pl_lifter_bwd": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _P, _P, _P]),
    "pl_lifter_fwd_eval_saved": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _P]),
    "pl_lifter_bwd_eval": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _P, _P, _P]),
    "pl_lifter_bwd_layers": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _P, _P, _c.c_int, _c.c_int, _P]),
    "pl_lifter_train_fwd_bwd": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _c.c_uint64, _c.c_uint64,
                                           _P, _P, _P, _c.c_int, _c.c_int, _P]),
    "pl_lifter_step_carries_adamw": (_c.c_int, [_D, _c.c_int64]),
    "pl_lifter_bwd_slab_rides": (_c.c_int, [_D, _c.c_int64, _c.c_int, _c.c_int]),
    "pl_lifter_train_step": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _c.c_uint64, _c.c_uint64,
                                        _P, _P, _P, _c.POINTER(PLAdamWStep), _P]),
    "pl_lifter_train_fwd_bwd_crit": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _c.c_uint64, _c.c_uint64,
                                                _c.POINTER(PLCriterion), _P, _P, _P, _c.c_int, _c.c_int, _P]),
    "pl_lifter_train_step_crit": (_c.c_int, [_D, _P, _P, _c.c_int64, _P, _c.c_size_t, _c.c_uint64, _c.c_uint64,
                                             _c.POINTER(PLCriterion), _P, _P, _P, _c.POINTER(PLAdamWStep), _P]),
    "pl_pose_loss_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.POINTER(PLCriterion)]),
    "pl_pose_loss_fwd_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.POINTER(PLCriterion), _c.c_float, _P, _P, _P, _P]),
    "pl_bone_lengths": (_c.c_int, [_P, _c.c_int64, _c.c_int32, _c.POINTER(PLSkeleton), _P, _P]),
    "pl_skeleton_terms_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int32, _c.POINTER(PLSkeleton), _c.c_float, _P, _P, _P]),
    "pl_skeleton_abi_bytes": (_c.c_size_t, [_c.c_int]),
    "pl_criterion_abi_bytes": (_c.c_size_t, [_c.c_int]),
    "pl_mse_scratch_bytes": (_c.c_size_t, [_c.c_int64]),
    "pl_mse_fwd_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_float, _P, _P, _P, _P]),
    "pl_l1_scratch_bytes": (_c.c_size_t, [_c.c_int]),
    "pl_l1_terms_fwd_bwd": (_c.c_int, [_c.POINTER(PLL1Term), _c.c_int, _c.c_float, _P, _P, _P]),
    "pl_mpjpe_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    "pl_mpjpe_accum": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_pose_errors": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_pose_errors_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_pose_errors_t": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_mpjpe_accum_t": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_pose_metrics_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int, _c.c_int]),
    "pl_pose_metrics_accum": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int, _P, _c.c_int, _P, _P, _P, _P, _P]),
    "pl_pose_errors_w": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P, _P]),
    "pl_pose_errors_w_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_pose_metrics_w_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int, _c.c_int]),
    "pl_pose_metrics_accum_w": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int, _P, _c.c_int, _P, _P, _P, _P, _P, _P]),
    "pl_adamw_flat": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_float, _c.c_float, _c.c_float,
                                 _c.c_float, _c.c_float, _c.c_int64, _c.c_float, _P]),
    "pl_adamw_flat_dev": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _P, _c.c_float, _c.c_float, _c.c_float,
                                     _c.c_float, _c.c_int64, _P, _c.c_float, _P]),
    "pl_adamw_flat_planes": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_float, _P, _c.c_float, _c.c_float, _c.c_float,
                                        _c.c_float, _c.c_int64, _P, _c.c_float, _c.POINTER(PLAdamWPlanes), _P]),
    "pl_grad_norm_scratch_bytes": (_c.c_size_t, [_c.c_int]),
    "pl_grad_norm_clip": (_c.c_int, [_P, _c.c_int64, _c.POINTER(PLGradRange), _c.c_int, _c.c_float, _c.c_int, _c.c_float, _P,
                                     _c.c_int, _P, _P, _P]),
    "pl_adamw_flat_clip": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_float, _c.c_float, _c.c_float,
                                      _c.c_float, _c.c_float, _c.c_int64, _c.c_float, _P, _P]),
    "pl_adamw_flat_dev_clip": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _P, _c.c_float, _c.c_float, _c.c_float,
                                          _c.c_float, _c.c_int64, _P, _c.c_float, _P, _P]),
    "pl_adamw_flat_planes_clip": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_float, _P, _c.c_float, _c.c_float, _c.c_float,
                                             _c.c_float, _c.c_int64, _P, _c.c_float, _c.POINTER(PLAdamWPlanes), _P, _P]),
    "pl_adamw_flat_planes_clip_ema": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_float, _P, _c.c_float, _c.c_float, _c.c_float,
                                                 _c.c_float, _c.c_int64, _P, _c.c_float, _c.POINTER(PLAdamWPlanes), _P,
                                                 _c.POINTER(PLEma), _P]),
    "pl_swap_f32": (_c.c_int, [_P, _P, _c.c_int64, _P]),
    "pl_wplanes_bytes": (_c.c_size_t, [_D]),
    "pl_wplanes_layer_bytes": (_c.c_size_t, [_D]),
    "pl_weight_plane_scale": (_c.c_float, []),
    "pl_wplanes_refresh": (_c.c_int, [_D, _P]),
    "pl_range_monitor": (_c.c_int, [_P]),
    "pl_flip_pose": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P]),
    "pl_counter_add": (_c.c_int, [_P, _c.c_int64, _P]),
    "pl_flip_pose_ex": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_float, _c.c_float, _P]),
    "pl_flip_w_nhwc": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P]),
    "pl_softargmax3d_nhwc_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_softargmax3d_nhwc_bwd": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_conv2d_nhwc_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                                  _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "pl_conv2d_nhwc_scratch_bytes_ex": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                                     _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "pl_conv2d_nhwc_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int,
                                      _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _P, _c.c_size_t,
                                      _P]),
    "pl_conv2d_nhwc_wgrad_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "pl_conv2d_nhwc_wgrad": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int,
                                        _c.c_int, _c.c_int, _c.c_int, _P, _c.c_int, _P, _c.c_size_t, _P]),
    "pl_bn_train_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    "pl_bn_train_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _c.c_float, _c.c_float, _P, _P, _P, _c.c_int,
                                   _P, _P, _P, _P, _P, _P]),
    "pl_bn_train_bwd": (_c.c_int, [_P, _P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_add_relu_fwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_mask_by_bits": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_conv_act_plane_scale": (_c.c_float, []),
    "pl_planes_split": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_float, _P, _P]),
    "pl_planes_split_strided": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_float, _P, _P]),
    "pl_bn_train_fwd_ex": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _c.c_float, _c.c_float, _P, _P, _P, _c.c_int,
                                      _P, _P, _P, _P, _P, _P, _c.c_int, _P, _P, _P]),
    "pl_gemm_stat_groups": (_c.c_int, [_c.c_int64]),
    "pl_bn_train_bwd_ex": (_c.c_int, [_P, _P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int, _P, _P]),
    "pl_add_relu_fwd_ex": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _c.c_int, _P]),
    "pl_mask_add_by_bits": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_bn_join_bwd": (_c.c_int, [_P, _P, _P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P, _P, _c.c_int, _P, _P]),
    "pl_maxpool3x3s2_nhwc": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_maxpool3x3s2_nhwc_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_maxpool3x3s2_nhwc_idx": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_maxpool3x3s2_nhwc_bwd_idx": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_upsample2x_zero_nhwc": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_colsum_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    "pl_colsum": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_deconv4x4s2_nhwc_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64]),
    "pl_deconv4x4s2_nhwc_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P,
                                           _c.c_int, _P, _c.c_int, _P, _c.c_size_t, _P]),
    "pl_nhwc_to_nchw": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_gather_rows2": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_pose_augment_gather": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64, _P]),
    "pl_row_weights_gather": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.POINTER(PLPoseAug), _c.c_uint64, _P]),
    "pl_row_weights_gather_host": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.POINTER(PLPoseAug), _c.c_uint64]),
    "pl_pose_augment_host": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64]),
    "pl_pose_augment_gather_t": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64,
                                            _P, _P, _P, _P, _P]),
    "pl_pose_augment_host_t": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64,
                                          _P, _P, _P, _P]),
    "pl_pose_prepare": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _c.c_int64, _c.c_int, _P, _P]),
    "pl_pose_prepare_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _c.c_int64, _c.c_int, _P]),
    "pl_pose_stats_chunk_rows": (_c.c_int64, []),
    "pl_pose_stats_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    "pl_pose_stats": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_pose_stats_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P]),
    "pl_pose_affine": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _c.c_int, _P, _P]),
    "pl_pose_affine_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P, _c.c_int, _P]),
    "pl_track_remap": (_c.c_int, [_P, _c.c_int64, _c.c_int, _P, _P]),
    "pl_track_remap_host": (_c.c_int, [_P, _c.c_int64, _c.c_int, _P]),
    "pl_track_prepare": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_float, _c.c_float, _c.c_float, _c.c_int, _c.c_float, _P, _P, _P,
                                    _P, _P]),
    "pl_track_prepare_host": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_float, _c.c_float, _c.c_float, _c.c_int, _c.c_float, _P, _P,
                                         _P, _P]),
    "pl_track_filter_tile_frames": (_c.c_int, [_c.c_int64, _c.c_int64, _c.c_int]),
    "pl_track_filter": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P, _c.c_int, _P, _P]),
    "pl_track_filter_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P, _c.c_int, _P]),
    "pl_track_velocity_errors": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int, _P, _P, _P, _P, _P]),
    "pl_track_velocity_errors_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int, _P, _P, _P, _P]),
    "pl_camera_project": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P, _P]),
    "pl_camera_project_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_camera_project_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "pl_camera_project_bwd_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P, _P]),
    "pl_camera_reproj_errors": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _c.c_float, _c.c_float,
                                           _P, _P]),
    "pl_camera_reproj_errors_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _c.c_float,
                                                _c.c_float, _P]),
    "pl_camera_reproj_loss_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64]),
    "pl_camera_reproj_loss_fwd_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int,
                                                 _c.c_float, _c.c_float, _c.c_float, _P, _P, _P, _P, _P]),
    "pl_camera_reproj_loss_fwd_bwd_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int,
                                                      _c.c_float, _c.c_float, _c.c_float, _P, _P, _P, _P]),
    "pl_camera_fit_translation": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _c.c_int, _P, _P, _P]),
    "pl_camera_fit_translation_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _c.c_int, _P, _P]),
    "pl_frame_warp_gather": (_c.c_int, [_c.POINTER(PLFrameWarp), _P]),
    "pl_frame_warp_host": (_c.c_int, [_c.POINTER(PLFrameWarp)]),
    "pl_pose_augment_gather_crop": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64,
                                               _c.POINTER(PLPoseCrop), _P, _P]),
    "pl_pose_augment_gather_crop_t": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug),
                                                 _c.c_uint64, _P, _P, _P, _P, _c.POINTER(PLPoseCrop), _P, _P]),
    "pl_pose_augment_host_crop": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64,
                                             _c.POINTER(PLPoseCrop), _P]),
    "pl_pose_augment_host_crop_t": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.POINTER(PLPoseAug), _c.c_uint64,
                                               _P, _P, _P, _P, _c.POINTER(PLPoseCrop), _P]),
    "pl_frame_warp_gather_crop": (_c.c_int, [_c.POINTER(PLFrameWarp), _c.POINTER(PLPoseCrop), _P, _P]),
    "pl_frame_warp_host_crop": (_c.c_int, [_c.POINTER(PLFrameWarp), _c.POINTER(PLPoseCrop), _P]),
    "pl_pose_crop_boxes": (_c.c_int, [_P, _c.c_int64, _c.POINTER(PLPoseCrop), _P, _P]),
    "pl_pose_crop_boxes_host": (_c.c_int, [_P, _c.c_int64, _c.POINTER(PLPoseCrop), _P]),
    "pl_crop_poses": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _P, _P]),
    "pl_crop_poses_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _P]),
    "pl_flip_tta_pack": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P]),
    "pl_flip_tta_merge": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P]),
    "pl_softargmax_dl_scale": (_c.c_int, [_P, _c.c_int64, _c.c_int, _P, _P]),
    "pl_softargmax_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P]),
    "pl_softargmax_bwd": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                     _P, _P]),
    "pl_heatmap_gaussian": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_float, _P, _P, _P]),
    "pl_heatmap_gaussian_host": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_float, _P, _P]),
    "pl_softargmax_hm_fwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_float,
                                        _P, _P, _P, _P, _P]),
    "pl_softargmax3d_nhwc_hm_fwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_float, _P, _P, _P,
                                               _P, _P]),
    "pl_softargmax_hm_bwd": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int, _c.c_int,
                                        _c.c_float, _P, _P, _P]),
    "pl_softargmax3d_nhwc_hm_bwd_ex": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_float,
                                                  _P, _P, _P, _c.c_int, _P, _P]),
    "pl_softargmax_hm_dl_scale": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _P, _P]),
    "pl_gemm_f32": (_c.c_int, [_c.c_int, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                               _c.c_int, _P, _P]),
    "pl_gemm_arith": (_c.c_int, [_c.c_int, _c.c_int, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                 _c.c_int, _P, _P]),
    "pl_gemm_planes_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int64, _c.c_int64]),
    "pl_gemm_planes": (_c.c_int, [_c.c_int, _c.c_int, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                  _c.c_float, _c.c_float, _P, _P]),
    "pl_gemm_planes_splits": (_c.c_int, [_c.c_int64, _c.c_int64, _c.c_int64]),
    "pl_gemm_planes_raw": (_c.c_int, [_c.c_int, _c.c_int, _P, _c.c_int64, _c.c_int64, _P, _c.c_int64, _c.c_int64, _P,
                                      _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_float, _P, _P, _P, _P]),
    "pl_conv2d_planes_fwd": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                        _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_float, _P, _P, _P]),
    "pl_softargmax3d_nhwc_bwd_ex": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _c.c_int,
                                               _P, _P]),
    "pl_colsum_planes": (_c.c_int, [_P, _c.c_int, _c.c_int64, _c.c_int64, _P, _P, _P, _P]),
    "pl_deconv4x4s2_planes_fwd": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                             _c.c_int64, _c.c_int64, _P, _c.c_float, _P, _P]),
    "pl_conv2d_planes_fwd_ep": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                           _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_float,
                                           _c.POINTER(PLPlanesEpilogue), _P]),
    "pl_deconv4x4s2_planes_fwd_ep": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                                _c.c_int64, _c.c_int64, _P, _c.c_float, _c.POINTER(PLPlanesEpilogue), _P]),
    "pl_conv2d_planes_wgrad": (_c.c_int, [_c.c_int, _P, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                          _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P, _c.c_float,
                                          _P, _P, _P]),
    "pl_conv2d_planes_fwd_hw": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                           _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _P, _c.c_float, _P, _P, _P]),
    "pl_conv2d_planes_fwd_ep_hw": (_c.c_int, [_c.c_int, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64, _P,
                                              _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                              _c.c_int, _P, _c.c_float, _c.POINTER(PLPlanesEpilogue), _P]),
    "pl_conv2d_planes_wgrad_hw": (_c.c_int, [_c.c_int, _P, _c.c_int64, _P, _c.c_int64, _c.c_int64, _c.c_int64, _c.c_int64,
                                             _c.c_int64, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                             _c.c_int, _P, _c.c_float, _P, _P, _P]),
    "pl_vit_attn_supported": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int]),
    "pl_vit_embed_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P, _c.c_int, _P, _P]),
    "pl_vit_embed_bwd_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int]),
    "pl_vit_embed_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _P, _P, _P]),
    "pl_vit_ln_fwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P, _P, _c.c_float, _P, _P, _P, _P]),
    "pl_vit_ln_bwd_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int]),
    "pl_vit_ln_bwd": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P, _P, _P, _P, _P]),
    "pl_vit_attn_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P, _P, _P]),
    "pl_vit_attn_bwd": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P, _P]),
    "pl_vit_gelu_fwd": (_c.c_int, [_P, _c.c_int64, _P, _P]),
    "pl_vit_gelu_bwd": (_c.c_int, [_P, _P, _c.c_int64, _P, _P]),
    "pl_vit_head_fwd": (_c.c_int, [_P, _c.c_int64, _c.c_int, _P, _P, _c.c_int, _P, _P]),
    "pl_vit_head_bwd_scratch_bytes": (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int]),
    "pl_vit_head_bwd": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _P, _c.c_int, _P, _P, _P, _P]),
    "pl_vit_planes_scratch_bytes": (_c.c_size_t, []),
    "pl_vit_planes_dyn": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P]),
    "pl_vit_ln_fwd_bf16": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P, _P, _c.c_float, _P, _P, _P,
                                      _c.c_int64, _P, _P]),
    "pl_vit_ln_bwd_bf16": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _P, _P, _P, _P, _P, _c.c_int64, _P,
                                      _P, _P]),
    "pl_vit_attn_fwd_bf16": (_c.c_int, [_P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P, _P, _c.c_int64, _P,
                                        _P]),
    "pl_vit_attn_bwd_bf16": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P, _P,
                                        _c.c_int64, _P]),
    "pl_vit_gelu_fwd_bf16": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_vit_gelu_bwd_bf16": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P]),
    "pl_vit_bf16_pack": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P]),
    "pl_prof_enable": (_c.c_int, [_c.c_int]),
    "pl_prof_read": (_c.c_int, [_c.c_double, _c.c_double, _c.POINTER(_c.c_double), _c.POINTER(_c.c_int64),
                                _c.POINTER(_c.c_double)]),
}

_lib = None


class PoseliftError(RuntimeError):
    pass


def lib():
    """The loaded library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PoseliftError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().pl_last_error().decode("utf-8", "replace")
        raise PoseliftError(f"{what} failed (status {rc}): {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
# range_guard._bind once the guard was ever enabled: the library keeps the record pointer per calling thread, and every call
# that launches asks current_stream_ptr() for its stream on the thread and device it runs on -- the one place to hand it over
_range_bind = None
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def current_stream_ptr():
    """hipStream_t of torch's current stream on the current device.  (torch.cuda.current_stream().cuda_stream builds a Stream
    object per call: 9 us, 170 times per conv training step.)
    Every wrapper that launches must take its stream from here, on the thread that makes the call and right before it: once
    the range guard was enabled this is also where the calling thread's library state is handed the device's record
    (range_guard._bind; the library keeps that pointer per thread).  A wrapper that cached a stream pointer, or passed a
    user's, would launch with another device's record or none."""
    if _raw_stream is not None and _cur_device is not None:
        dev = _cur_device()
        if _range_bind is not None:
            _range_bind(dev)
        return _raw_stream(dev)
    if _range_bind is not None:
        _range_bind(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def on_device(dev):
    """`with on_device(t.device):` -- torch.cuda.device(dev), minus its cost when dev already is the current device (the
    one-process-per-GPU case: always)."""
    idx = dev.index if isinstance(dev, torch.device) else dev
    if _cur_device is not None and (idx is None or idx == _cur_device()):
        return _NO_SWITCH
    return torch.cuda.device(dev)


def aligned16(t):
    """`t` itself when its storage starts on a 16-byte boundary, else a copy that does (every fresh allocation does).
    The entry points refuse a caller's pointer that a kernel reads or writes 16 bytes at a time and that is not 16-byte
    aligned ("Alignment contract of caller pointers"); a contiguous view of a larger tensor -- table[n:],
    table[i * B:(i + 1) * B] -- need not be.  The copy is an autograd op, so gradients still reach a misaligned leaf.  On the
    aligned path this is one integer test: no sync, no allocation."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def require_aligned16_out(t, name):
    """An `out=` tensor that a kernel writes in place cannot be copied behind the caller's back: refuse it by name."""
    if t.data_ptr() % 16 != 0:
        raise PoseliftError(f"{name} must be 16-byte aligned (data_ptr() % 16 == {t.data_ptr() % 16}): it is written in place")


def require_device_tensor(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise PoseliftError(
            f"{name} is on {t.device}: the lifter runs on an MI355X (ROCm) device only; "
            "there is no CPU path")
    if t.dtype != dtype:
        raise PoseliftError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise PoseliftError(f"{name} must be contiguous")
