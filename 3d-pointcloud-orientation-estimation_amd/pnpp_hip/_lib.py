"""ctypes binding of libpnpp_hip.so (the C ABI declared in include/pnpp_hip.h).

There is deliberately no fallback: if the shared library is missing or cannot be loaded, every
entry point raises.  PyTorch is used only for device memory, streams and autograd bookkeeping.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpnpp_hip.so")

PNPP_MAX_LAYERS = 4
PNPP_OK, PNPP_ERR_ARG, PNPP_ERR_RANGE, PNPP_ERR_LAUNCH, PNPP_ERR_WORKSPACE = 0, -1, -2, -3, -4
NORM_NONE, NORM_BATCH, NORM_LAYER = 0, 1, 2

_fp = C.c_void_p  # device pointers travel as integers (tensor.data_ptr())


class SaDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("S", C.c_int), ("K", C.c_int), ("D", C.c_int), ("L", C.c_int),
                ("C", C.c_int * PNPP_MAX_LAYERS), ("group_all", C.c_int), ("training", C.c_int),
                ("eps", C.c_float), ("momentum", C.c_float)]


_PL = _fp * PNPP_MAX_LAYERS


class SaFwdArgs(C.Structure):
    _fields_ = [("xyz", _fp), ("points", _fp), ("centre_idx", _fp), ("neighbour_idx", _fp),
                ("conv_w", _PL), ("conv_b", _PL), ("bn_w", _PL), ("bn_b", _PL), ("bn_rm", _PL), ("bn_rv", _PL), ("bn_nbt", _PL),
                ("new_xyz", _fp), ("out", _fp), ("saved", _fp), ("scratch", _fp)]


class SaBwdArgs(C.Structure):
    _fields_ = [("xyz", _fp), ("points", _fp), ("conv_w", _PL), ("bn_w", _PL), ("bn_b", _PL),
                ("dout", _fp), ("saved", _fp), ("scratch", _fp),
                ("d_conv_w", _PL), ("d_conv_b", _PL), ("d_bn_w", _PL), ("d_bn_b", _PL), ("dpoints", _fp)]


class SlabReduce(C.Structure):
    _fields_ = [("slab", _fp), ("nsplit", C.c_int), ("Nc", C.c_int), ("kp_pad", C.c_int), ("Kvalid", C.c_int), ("perm_D", C.c_int),
                ("out", _fp), ("ldo", C.c_int)]


SA_TAIL_NONE, SA_TAIL_SLAB_REDUCE, SA_TAIL_SLAB_REDUCE2 = 0, 1, 2


class SaTail(C.Structure):   # a level's trailing dW reduction handed on (pnpp_sa_backward_ex / pnpp_sa_run_tail)
    _fields_ = [("kind", C.c_int), ("blocks", C.c_int), ("r", SlabReduce * 2)]


class SaInferArgs(C.Structure):
    _fields_ = [("xyz", _fp), ("points", _fp), ("centre_idx", _fp), ("neighbour_idx", _fp), ("idx_out", _fp), ("weights", _fp),
                ("new_xyz", _fp), ("out", _fp)]


class PnInferDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("D", C.c_int), ("L", C.c_int), ("C", C.c_int * PNPP_MAX_LAYERS),
                ("input_transform", C.c_int), ("transform_after", C.c_int), ("relu_last", C.c_int), ("eps", C.c_float)]


class PnInferArgs(C.Structure):
    _fields_ = [("x", _fp), ("stride_b", C.c_int64), ("stride_n", C.c_int64), ("stride_c", C.c_int64), ("trans", _fp), ("trans_feat", _fp),
                ("weights", _fp), ("scratch", _fp), ("out", _fp), ("feat_out", _fp), ("feat_layer", C.c_int)]


class PtInferDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("n_valid", C.c_int), ("in_dim", C.c_int), ("E", C.c_int), ("H", C.c_int), ("F", C.c_int),
                ("depth", C.c_int), ("eps", C.c_float)]


class PtInferLayerParams(C.Structure):
    _fields_ = [(n, _fp) for n in ("in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b",
                                   "norm1_w", "norm1_b", "norm2_w", "norm2_b")]


PT_IN_PROJ, PT_OUT_PROJ, PT_LINEAR1, PT_LINEAR2, PT_NORM1, PT_NORM2, PT_INPUT_PROJ = range(7)


class FcDesc(C.Structure):
    _fields_ = [("M", C.c_int), ("K", C.c_int), ("N", C.c_int), ("norm", C.c_int), ("relu", C.c_int),
                ("training", C.c_int), ("eps", C.c_float), ("momentum", C.c_float), ("drop_scale", C.c_float)]


class FcFwdArgs(C.Structure):
    _fields_ = [("x", _fp), ("w", _fp), ("b", _fp), ("nw", _fp), ("nb", _fp), ("rm", _fp), ("rv", _fp), ("nbt", _fp),
                ("mask", _fp), ("mask_out", _fp), ("drop_p", C.c_float), ("rng_seed", C.c_uint64), ("rng_counter", _fp),
                ("y", _fp), ("saved", _fp), ("scratch", _fp)]


class FcBwdArgs(C.Structure):
    _fields_ = [("x", _fp), ("w", _fp), ("b", _fp), ("nw", _fp), ("nb", _fp), ("mask", _fp), ("dy", _fp),
                ("saved", _fp), ("scratch", _fp), ("dx", _fp), ("dw", _fp), ("db", _fp), ("dnw", _fp), ("dnb", _fp)]


class PnPoolDesc(C.Structure):
    _fields_ = [("B", C.c_int), ("N", C.c_int), ("K", C.c_int), ("C", C.c_int), ("relu", C.c_int), ("training", C.c_int),
                ("eps", C.c_float), ("momentum", C.c_float)]


class PnPoolFwdArgs(C.Structure):
    _fields_ = [("a", _fp), ("w", _fp), ("b", _fp), ("gamma", _fp), ("beta", _fp), ("rm", _fp), ("rv", _fp), ("nbt", _fp),
                ("out", _fp), ("saved", _fp), ("scratch", _fp)]


class PnPoolBwdArgs(C.Structure):
    _fields_ = [("a", _fp), ("w", _fp), ("gamma", _fp), ("dout", _fp), ("saved", _fp), ("scratch", _fp), ("da", _fp), ("dw", _fp),
                ("db", _fp), ("dgamma", _fp), ("dbeta", _fp)]


PNPP_AUG_MAX_TARGETS = 4
AUG_YAW, AUG_SCALE, AUG_JITTER = 1, 2, 4
AUG_ANGLE, AUG_VM, AUG_AXIS, AUG_DIR8 = range(4)


class AugmentTarget(C.Structure):
    _fields_ = [("kind", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("inp", _fp), ("out", _fp), ("counts", _fp)]


class AugmentDesc(C.Structure):
    _fields_ = [("flags", C.c_uint), ("scale_lo", C.c_float), ("scale_hi", C.c_float), ("sigma", C.c_float), ("clip", C.c_float),
                ("n_targets", C.c_int), ("targets", AugmentTarget * PNPP_AUG_MAX_TARGETS), ("dirs8", _fp)]


VIEW_MAX_G, VIEW_DIRS, VIEW_ANGLES = 128, 1, 2


class ViewDesc(C.Structure):   # pnpp_view_desc
    _fields_ = [("G", C.c_int), ("splat", C.c_int), ("thickness", C.c_float), ("elev_lo", C.c_float), ("elev_hi", C.c_float),
                ("drop", C.c_float), ("min_keep", C.c_int), ("flags", C.c_uint), ("view_dirs", _fp)]


VOXEL_MAX_GRID, OUTLIER_MAX_K = 1024, 127                # include/pnpp_hip.h: PNPP_VOXEL_MAX_GRID, PNPP_OUTLIER_MAX_K
SCAN_NONE, SCAN_CENTROID, SCAN_SPHERE, SCAN_BOX = 0, 1, 1, 2   # pnpp_normalize_clouds' centre / scale modes
NORMALS_NONE, NORMALS_AWAY, NORMALS_TOWARD = range(3)  # pnpp_estimate_normals' orientation modes
NORMALS_KMIN, NORMALS_KMAX = 3, 128
YAW_ANGLE_BLOCK, YAW_TILE, YAW_QUERIES, YAW_MAX_ORDERS = 8, 1024, 256, 16   # include/pnpp_hip.h: PNPP_YAW_*
PNPP_OPTIM_MAX_GROUPS = 8
ORIENT_BINS, ORIENT_STRIDE, ORIENT_MAX_LABELS = 360, 728, 64   # pnpp_orient_eval's accumulator (include/pnpp_hip.h)
SCHED_CONSTANT, SCHED_COSINE, SCHED_STEP = range(3)


class OptimDesc(C.Structure):   # pnpp_optim_desc: the scheduled optimiser's update, passed to the kernel by value
    _fields_ = [("n_groups", C.c_int), ("decoupled", C.c_int), ("end", C.c_uint64 * PNPP_OPTIM_MAX_GROUPS),
                ("lr_mult", C.c_float * PNPP_OPTIM_MAX_GROUPS), ("weight_decay", C.c_float * PNPP_OPTIM_MAX_GROUPS),
                ("sched_kind", C.c_int), ("warmup", C.c_uint64), ("total", C.c_uint64), ("every", C.c_uint64),
                ("start_factor", C.c_double), ("min_factor", C.c_double), ("gamma", C.c_double),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("grad_scale", C.c_float),
                ("max_norm", C.c_float), ("ema_decay", C.c_float), ("zero_grad", C.c_int)]


# name -> (restype, argtypes); this table is also what tests/test_abi.py checks against the header
_i, _f, _u64, _sz = C.c_int, C.c_float, C.c_uint64, C.c_size_t
# int fn(double *buf, size_t n_doubles, void *stream, void *user): sums buf over the ranks in place (SyncBN, pnpp_set_stats_exchange)
STATS_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)
SIGNATURES = {
    "pnpp_last_error": (C.c_char_p, []),
    "pnpp_abi_version": (_i, []),
    "pnpp_profile_enable": (_i, [_i]),
    "pnpp_profile_report": (_i, [C.c_char_p, _sz]),
    "pnpp_square_distance": (_i, [_fp, _fp, _i, _i, _i, _fp, _fp]),
    "pnpp_knn": (_i, [_fp, _fp, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_fps": (_i, [_fp, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_ball_query": (_i, [_fp, _fp, _i, _i, _i, _f, _i, _fp, _fp]),
    "pnpp_ball_query_r2": (_i, [_fp, _fp, _i, _i, _i, _f, _i, _fp, _fp]),
    "pnpp_sample_random": (_i, [_u64, _u64, _i, _i, _i, _fp, _fp]),
    "pnpp_subsample_points": (_i, [_u64, _u64, _fp, _fp, _fp, _i, _i, _i, _fp, _fp]),
    "pnpp_augment_clouds": (_i, [_u64, _u64, _fp, _fp, _fp, _i, C.c_int64, _i, C.POINTER(AugmentDesc), _fp, _fp]),
    "pnpp_sample_random_dev": (_i, [_u64, _fp, _u64, _i, _i, _i, _fp, _fp]),
    "pnpp_sample_random_dev2": (_i, [_u64, _fp, _u64, _i, _i, _i, _fp, _i, _i, _fp, _fp]),
    "pnpp_index_points": (_i, [_fp, _fp, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_index_points_bwd": (_i, [_fp, _fp, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_sa_saved_bytes": (_sz, [C.POINTER(SaDesc)]),
    "pnpp_sa_scratch_bytes": (_sz, [C.POINTER(SaDesc)]),
    "pnpp_sa_forward": (_i, [C.POINTER(SaDesc), C.POINTER(SaFwdArgs), _fp]),
    "pnpp_sa_backward": (_i, [C.POINTER(SaDesc), C.POINTER(SaBwdArgs), _fp]),
    "pnpp_sa_backward_ex": (_i, [C.POINTER(SaDesc), C.POINTER(SaBwdArgs), C.POINTER(SaTail), C.POINTER(SaTail), _fp]),
    "pnpp_sa_run_tail": (_i, [C.POINTER(SaTail), _fp]),
    "pnpp_sa_saved_neighbours": (_fp, [C.POINTER(SaDesc), _fp]),
    "pnpp_knn_pair": (_i, [_fp, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp]),
    "pnpp_knn_pair_partials": (_i, [_i, _i, _i]),
    "pnpp_sa_group_pair": (_i, [C.POINTER(SaDesc), C.POINTER(SaDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_sa_saved_argmax": (_fp, [C.POINTER(SaDesc), _fp]),
    "pnpp_sa_saved_relu_mask": (_i, [C.POINTER(SaDesc), _fp, _fp, _fp, _i, _fp, _fp]),
    "pnpp_sa_infer_supported": (_i, [C.POINTER(SaDesc)]),
    "pnpp_sa_infer_weights_bytes": (_sz, [C.POINTER(SaDesc)]),
    "pnpp_sa_infer_weights_layout": (_i, [C.POINTER(SaDesc), _i, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_sz)]),
    "pnpp_sa_infer_fold": (_i, [C.POINTER(SaDesc), C.POINTER(SaFwdArgs), _fp, _fp]),
    "pnpp_sa_infer": (_i, [C.POINTER(SaDesc), C.POINTER(SaInferArgs), _fp]),
    "pnpp_sa_infer_group_pair": (_i, [C.POINTER(SaDesc), C.POINTER(SaDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_fc_infer_fold": (_i, [_i, _i, _fp, _fp, _fp, _fp, _fp, _fp, _f, _fp, _fp, _fp]),
    "pnpp_pn_infer_supported": (_i, [C.POINTER(PnInferDesc)]),
    "pnpp_pn_infer_weights_bytes": (_sz, [C.POINTER(PnInferDesc)]),
    "pnpp_pn_infer_weights_layout": (_i, [C.POINTER(PnInferDesc), _i, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_sz)]),
    "pnpp_pn_infer_scratch_bytes": (_sz, [C.POINTER(PnInferDesc)]),
    "pnpp_pn_infer_fold": (_i, [C.POINTER(PnInferDesc), C.POINTER(SaFwdArgs), _fp, _fp]),
    "pnpp_pn_infer": (_i, [C.POINTER(PnInferDesc), C.POINTER(PnInferArgs), _fp]),
    "pnpp_pt_infer_supported": (_i, [C.POINTER(PtInferDesc)]),
    "pnpp_pt_infer_weights_bytes": (_sz, [C.POINTER(PtInferDesc)]),
    "pnpp_pt_infer_weights_layout": (_i, [C.POINTER(PtInferDesc), _i, _i, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_sz)]),
    "pnpp_pt_infer_fold": (_i, [C.POINTER(PtInferDesc), _i, C.POINTER(PtInferLayerParams), _fp, _fp, _fp, _fp]),
    "pnpp_pt_infer_scratch_bytes": (_sz, [C.POINTER(PtInferDesc)]),
    "pnpp_pt_infer_head": (_i, [C.POINTER(PtInferDesc), _fp, _fp, _fp, _fp, _fp]),
    "pnpp_pt_infer_tail": (_i, [C.POINTER(PtInferDesc), _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_pt_infer_pool": (_i, [C.POINTER(PtInferDesc), _fp, _fp, _fp, _i, _fp, _fp]),
    "pnpp_attention_infer": (_i, [_fp, _i, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_attention_infer_supported": (_i, [_i, _i, _i, _i, _i]),
    "pnpp_attention_split_fwd": (_i, [_fp, _i, _i, _i, _i, _i, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_split_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_split_supported": (_i, [_i, _i, _i, _i, _i]),
    # ragged batches: the namesake's list with the lengths tensor after n_valid (after the descriptor for pnpp_pt_infer_*)
    "pnpp_attention_fwd_ragged": (_i, [_fp, _i, _i, _i, _fp, _i, _i, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_bwd_ragged": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _fp, _i, _i, _fp, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_split_fwd_ragged": (_i, [_fp, _i, _i, _i, _fp, _i, _i, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_split_bwd_ragged": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _fp, _i, _i, _fp, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_infer_ragged": (_i, [_fp, _i, _i, _i, _fp, _i, _i, _fp, _fp]),
    "pnpp_mean_points_ragged": (_i, [_fp, _i, _i, _fp, _i, _fp, _fp]),
    "pnpp_mean_points_bwd_ragged": (_i, [_fp, _i, _i, _fp, _i, _fp, _fp]),
    "pnpp_pt_infer_head_ragged": (_i, [C.POINTER(PtInferDesc), _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_pt_infer_tail_ragged": (_i, [C.POINTER(PtInferDesc), _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_pt_infer_pool_ragged": (_i, [C.POINTER(PtInferDesc), _fp, _fp, _fp, _fp, _i, _fp, _fp]),
    # ... of the index primitives and the paired launches: the lengths tensor after N (after xyz for the two descriptor calls)
    "pnpp_knn_ragged": (_i, [_fp, _fp, _i, _i, _i, _fp, _i, _fp, _fp]),
    "pnpp_fps_ragged": (_i, [_fp, _i, _i, _fp, _i, _fp, _fp, _fp]),
    "pnpp_ball_query_ragged": (_i, [_fp, _fp, _i, _i, _i, _fp, _f, _i, _fp, _fp]),
    "pnpp_ball_query_r2_ragged": (_i, [_fp, _fp, _i, _i, _i, _fp, _f, _i, _fp, _fp]),
    "pnpp_sample_random_ragged": (_i, [_u64, _u64, _i, _i, _fp, _i, _fp, _fp]),
    "pnpp_sample_random_dev_ragged": (_i, [_u64, _fp, _u64, _i, _i, _fp, _i, _fp, _fp]),
    "pnpp_sample_random_dev2_ragged": (_i, [_u64, _fp, _u64, _i, _i, _fp, _i, _fp, _i, _i, _fp, _fp]),
    "pnpp_knn_pair_ragged": (_i, [_fp, _i, _i, _fp, _fp, _i, _i, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp]),
    "pnpp_sa_group_pair_ragged": (_i, [C.POINTER(SaDesc), C.POINTER(SaDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_sa_infer_group_pair_ragged": (_i, [C.POINTER(SaDesc), C.POINTER(SaDesc), _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp]),
    # surface normals: xyz, B, N, [lengths,] k, orient, ref, out, out_stride, curv, idx, stream
    "pnpp_estimate_normals": (_i, [_fp, _i, _i, _i, _i, _fp, _fp, _i, _fp, _fp, _fp]),
    "pnpp_estimate_normals_ragged": (_i, [_fp, _i, _i, _fp, _i, _i, _fp, _fp, _i, _fp, _fp, _fp]),
    # yaw symmetry: xyz, B, N, [lengths,] centre, table, G, workspace, bytes, nearest_dist, nearest_idx, stream
    "pnpp_yaw_workspace_bytes": (_sz, [_i, _i, _i]),
    "pnpp_yaw_profile": (_i, [_fp, _i, _i, _fp, _fp, _i, _fp, _sz, _fp, _fp, _fp]),
    "pnpp_yaw_profile_ragged": (_i, [_fp, _i, _i, _fp, _fp, _fp, _i, _fp, _sz, _fp, _fp, _fp]),
    # workspace, bytes, B, N, lengths, G, tol, orders (host), n_orders, distance, floor, score, order, count, angles, angle_stride, stream
    "pnpp_yaw_symmetry": (_i, [_fp, _sz, _i, _i, _fp, _i, _f, C.POINTER(C.c_int32), _i, _fp, _fp, _fp, _fp, _fp, _fp, _i, _fp]),
    # single-view scan: seed, stream id, xyz_in, xyz_out, lengths_in, lengths_out, index_out, B, N, C, desc, params, stream
    "pnpp_view_clouds": (_i, [_u64, _u64, _fp, _fp, _fp, _fp, _fp, _i, C.c_int64, _i, C.POINTER(ViewDesc), _fp, _fp]),
    # raw-scan preparation: B, N -> bytes
    "pnpp_voxel_workspace_bytes": (_sz, [_i, C.c_int64]),
    # xyz_in, xyz_out, lengths_in, lengths_out, index_out, B, N, C, cell, grid, workspace, bytes, stream
    "pnpp_voxel_downsample": (_i, [_fp, _fp, _fp, _fp, _fp, _i, C.c_int64, _i, _f, _i, _fp, _sz, _fp]),
    # xyz, lists, lengths, B, N, C, k, statistic, stream
    "pnpp_outlier_statistic": (_i, [_fp, _fp, _fp, _i, C.c_int64, _i, _i, _fp, _fp]),
    # xyz_in, xyz_out, statistic, lengths_in, lengths_out, index_out, stats_out, B, N, C, k, std_ratio, stream
    "pnpp_outlier_filter": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, C.c_int64, _i, _i, C.c_double, _fp]),
    # xyz_in, xyz_out, lengths, B, N, C, centre mode, scale mode, centre_out, scale_out, stream
    "pnpp_normalize_clouds": (_i, [_fp, _fp, _fp, _i, C.c_int64, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_build_flags": (C.c_uint, []),
    "pnpp_debug_wsd3_timeouts": (_i, []),
    "pnpp_fc_saved_bytes": (_sz, [C.POINTER(FcDesc)]),
    "pnpp_fc_scratch_bytes": (_sz, [C.POINTER(FcDesc)]),
    "pnpp_fc_forward": (_i, [C.POINTER(FcDesc), C.POINTER(FcFwdArgs), _fp]),
    "pnpp_fc_backward": (_i, [C.POINTER(FcDesc), C.POINTER(FcBwdArgs), _fp]),
    "pnpp_vm_head_kl": (_i, [_fp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_vm_fc_head_kl_step": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_vm_fc_head_kl_step_sample": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _u64, _fp, _u64, _i, _i, _i, _fp, _i, _i,
                                            _fp, _fp]),
    "pnpp_vm_head_kl_mean": (_i, [_fp, _fp, _fp, _i, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_vm_head_bwd": (_i, [_fp, _fp, _fp, _i, _fp, _fp]),
    "pnpp_vm_kl_single": (_i, [_fp, _fp, _fp, _fp, _i, _fp, _fp, _fp, _fp]),
    "pnpp_vm_match_loss": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_mvm_fc_head_match_step": (_i, [_fp] * 9 + [_i, _i, _i, _f, _f] + [_fp] * 11 + [_u64, _fp, _u64, _i, _i, _i, _fp, _i, _i, _fp, _fp]),
    "pnpp_mvm_head": (_i, [_fp, _fp, _fp, _i, _i, _f, _f, _fp, _fp, _fp, _fp]),
    "pnpp_mvm_head_bwd": (_i, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _f, _f, _fp, _fp, _fp, _fp]),
    "pnpp_mvm_grid_kl": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_mvm_head_grid_kl": (_i, [_fp, _fp, _fp, _fp, _fp, _i, _i, _f, _f, _i] + [_fp] * 8),
    "pnpp_soft_ce": (_i, [_fp, _fp, _i, _i, _fp, _fp, _fp]),
    "pnpp_mvm_decode": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _f, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnpp_orient_eval": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _fp, _i, _fp, _i, _fp, _fp, C.c_int64, _fp, _fp, _fp, _fp]),
    "pnpp_log_softmax": (_i, [_fp, _i, _i, _fp, _fp]),
    "pnpp_log_softmax_bwd": (_i, [_fp, _fp, _i, _i, _fp, _fp]),
    "pnpp_linear_log_softmax": (_i, [_fp, _fp, _fp, _i, _i, _i, _fp, _fp]),
    "pnpp_nll_loss": (_i, [_fp, _fp, _i, _i, _fp, _fp, _i, _fp]),
    "pnpp_nll_loss_bwd": (_i, [_fp, _fp, _i, _i, _fp, _fp]),
    "pnpp_l2_normalize": (_i, [_fp, _i, _i, _f, _fp, _fp]),
    "pnpp_l2_normalize_bwd": (_i, [_fp, _fp, _i, _i, _f, _fp, _fp]),
    "pnpp_mse": (_i, [_fp, _fp, _sz, _fp, _fp, _fp]),
    "pnpp_mse_rows": (_i, [_fp, _fp, _i, _i, _fp, _fp, _fp]),
    "pnpp_orth_loss": (_i, [_fp, _fp, _i, _i, _fp, _fp, _fp, _fp]),
    "pnpp_proj_probs": (_i, [_fp, _fp, _i, _i, _fp, _fp]),
    "pnpp_proj_probs_bwd": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp]),
    "pnpp_linear_smallk": (_i, [_fp, _fp, _fp, _i, _i, _i, _fp, _fp]),
    "pnpp_attention_fwd": (_i, [_fp, _i, _i, _i, _i, _i, _fp, _f, _fp, _fp, _fp]),
    "pnpp_attention_dropout_mask": (_i, [_u64, _u64, _i, _i, _i, _f, _fp, _fp, _fp]),
    "pnpp_attention_dropout_mask_dev": (_i, [_u64, _fp, _u64, _i, _i, _i, _f, _fp, _fp, _fp]),
    "pnpp_add_layernorm": (_i, [_fp, _fp, _fp, _fp, _i, _i, _f, _fp, _fp]),
    "pnpp_mean_points": (_i, [_fp, _i, _i, _i, _fp, _fp]),
    "pnpp_linear_smallk_bwd_scratch_bytes": (_sz, [_i, _i]),
    "pnpp_linear_smallk_bwd": (_i, [_fp, _fp, _i, _i, _i, _fp, _fp, _fp, _fp]),
    "pnpp_attention_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _f, _fp, _fp, _fp]),
    "pnpp_add_layernorm_bwd_scratch_bytes": (_sz, [_i, _i]),
    "pnpp_add_layernorm_bwd": (_i, [_fp, _fp, _fp, _fp, _i, _i, _f, _fp, _fp, _fp, _fp]),
    "pnpp_mean_points_bwd": (_i, [_fp, _i, _i, _i, _fp, _fp]),
    "pnpp_set_matmul_precision": (_i, [_i]),
    "pnpp_set_stats_exchange": (_i, [STATS_EXCHANGE_FN, C.c_void_p, C.c_void_p, _sz]),
    "pnpp_stats_exchange_enabled": (_i, []),
    "pnpp_get_matmul_precision": (_i, []),
    "pnpp_set_split_products": (_i, [_i]),
    "pnpp_get_split_products": (_i, []),
    "pnpp_set_store_policy": (_i, [_i]),
    "pnpp_get_store_policy": (_i, []),
    "pnpp_adam_step": (_i, [_fp, _fp, _fp, _fp, _sz, _i, _f, _f, _f, _f, _f, _fp]),
    "pnpp_adam_step_zero": (_i, [_fp, _fp, _fp, _fp, _sz, _i, _f, _f, _f, _f, _f, _fp]),
    "pnpp_adam_step_dev": (_i, [_fp, _fp, _fp, _fp, _sz, _fp, _f, _f, _f, _f, _f, _i, _fp]),
    "pnpp_adam_step_clip": (_i, [_fp, _fp, _fp, _fp, _sz, _i, _f, _f, _f, _f, _f, _fp, _f, _i, _fp]),
    "pnpp_adam_step_dev_clip": (_i, [_fp, _fp, _fp, _fp, _sz, _fp, _f, _f, _f, _f, _f, _fp, _f, _i, _fp]),
    "pnpp_sumsq": (_i, [_fp, _sz, _fp, _fp, _sz, _fp]),
    "pnpp_adamw_step": (_i, [C.POINTER(OptimDesc), _fp, _fp, _fp, _fp, _fp, _sz, _fp, _fp, _fp]),
    "pnpp_lr_factor": (_i, [C.POINTER(OptimDesc), _u64, C.POINTER(C.c_double)]),
    "pnpp_pn_pool_saved_bytes": (_sz, [C.POINTER(PnPoolDesc)]),
    "pnpp_pn_pool_scratch_bytes": (_sz, [C.POINTER(PnPoolDesc)]),
    "pnpp_pn_pool_forward": (_i, [C.POINTER(PnPoolDesc), C.POINTER(PnPoolFwdArgs), _fp]),
    "pnpp_pn_pool_backward": (_i, [C.POINTER(PnPoolDesc), C.POINTER(PnPoolBwdArgs), _fp]),
    "pnpp_pn_pool_saved_route": (_fp, [C.POINTER(PnPoolDesc), _fp]),
    "pnpp_pn_pool_saved_zsel": (_fp, [C.POINTER(PnPoolDesc), _fp]),
    "pnpp_pn_pool_saved_ypre": (_fp, [C.POINTER(PnPoolDesc), _fp]),
    "pnpp_fc_recompute_output": (_i, [C.POINTER(FcDesc), _fp, _fp, _fp, _fp]),
    "pnpp_pn_transform": (_i, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, _i, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_pn_transform_bwd": (_i, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_regularizer": (_i, [_fp, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_regularizer_bwd": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp]),
    "pnpp_pn_add_identity": (_i, [_fp, _i, _i, _fp, _fp]),
    "pnpp_pn_concat": (_i, [_fp, _fp, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_pn_concat_bwd": (_i, [_fp, _i, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_bn_relu": (_i, [_fp, _i, _i, _fp, _fp, _fp, _fp, _fp, _i, _f, _f, _fp, _fp, _fp, _fp]),
    "pnpp_pn_bn_relu_bwd": (_i, [_fp, _fp, _fp, _i, _i, _fp, _fp, _fp, _i, _fp, _fp, _fp, _fp]),
    # ragged batches of the vanilla PointNet: packed point rows addressed through offs (B + 1), see include/pnpp_hip.h
    "pnpp_pn_offsets": (_i, [_fp, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_pool_saved_bytes_ragged": (_sz, [C.POINTER(PnPoolDesc), _i]),
    "pnpp_pn_pool_scratch_bytes_ragged": (_sz, [C.POINTER(PnPoolDesc), _i]),
    "pnpp_pn_pool_forward_ragged": (_i, [C.POINTER(PnPoolDesc), C.POINTER(PnPoolFwdArgs), _fp, _i, _fp]),
    "pnpp_pn_pool_backward_ragged": (_i, [C.POINTER(PnPoolDesc), C.POINTER(PnPoolBwdArgs), _fp, _i, _fp]),
    "pnpp_pn_transform_ragged": (_i, [_fp, _i, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_pn_transform_bwd_ragged": (_i, [_fp, _i, C.c_int64, C.c_int64, C.c_int64, _fp, _fp, _fp, _i, _i, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_concat_ragged": (_i, [_fp, _fp, _i, _fp, _i, _i, _i, _i, _fp, _fp]),
    "pnpp_pn_concat_bwd_ragged": (_i, [_fp, _fp, _i, _i, _i, _i, _fp, _fp, _fp]),
    "pnpp_pn_infer_ragged": (_i, [C.POINTER(PnInferDesc), C.POINTER(PnInferArgs), _fp, _fp]),
}

_lib = None


class HipExtensionMissing(RuntimeError):
    pass


def lib():
    """The loaded shared library (loads on first use; never falls back to anything else)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionMissing(
                f"{LIB_PATH} is missing: build it with `python -m pnpp_hip.build` (hipcc, gfx950). "
                "This package has no CPU or PyTorch fallback.")
        try:
            h = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise HipExtensionMissing(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if h.pnpp_abi_version() != 5:
            raise HipExtensionMissing("libpnpp_hip.so ABI version mismatch; rebuild it")
        _lib = h
    return _lib


def last_error() -> str:
    return lib().pnpp_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    """Turns a pnpp_status into the exception type the reference's Python surface would raise."""
    if rc == PNPP_OK:
        return
    msg = last_error()
    if rc == PNPP_ERR_ARG:
        raise ValueError(msg)
    raise RuntimeError(msg)
