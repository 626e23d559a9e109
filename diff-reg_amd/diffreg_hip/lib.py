"""ctypes binding of libdiffreg_hip.so (C ABI declared in include/diffreg_hip.h).

The library is the product: there is NO CPU fallback.  Importing this module on a box where the
library was not built raises ImportError; calling an op with CPU tensors raises RuntimeError.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdiffreg_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError("libdiffreg_hip.so is missing (%s): run `python __graft_entry__.py build` or "
                      "`make -C diff-reg_amd/csrc`" % LIB_PATH)

_lib = ctypes.CDLL(LIB_PATH)

c_int, c_size_t, c_void_p, c_char_p, c_double, c_float = (ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p,
                                                          ctypes.c_char_p, ctypes.c_double, ctypes.c_float)

# name -> (restype, argtypes); kept in the order of include/diffreg_hip.h
SIGNATURES = {
    "dr_version": (c_int, []),
    "dr_strerror": (c_char_p, [c_int]),
    "dr_last_hip_error": (c_char_p, []),
    "dr_sinkhorn_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dr_sinkhorn_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_sinkhorn_f16": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "dr_sinkhorn_f64": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                c_void_p, c_void_p, c_size_t, c_void_p]),
}


class LayerWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("q_proj", "k_proj", "v_proj", "merge", "mlp0", "mlp2", "norm1_w", "norm1_b",
                                        "norm2_w", "norm2_b")]


class LoopConfig(ctypes.Structure):
    _fields_ = [("variant", c_int), ("C", c_int), ("H", c_int), ("n_layers", c_int), ("steps", c_int),
                ("sk_iters", c_int), ("voxel", c_float), ("origin", c_float * 3), ("sample_rate", c_float),
                ("max_condition_num", c_float), ("flags", c_int), ("h_alphas_cumprod", c_void_p),
                ("h_times", c_void_p)]


class LoopWeights(ctypes.Structure):
    _fields_ = [("layers", ctypes.POINTER(LayerWeights)), ("src_proj", c_void_p), ("bin_score", c_void_p),
                ("pe_freq", c_void_p), ("prepacked", c_void_p)]


class FusionLayerWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "lin_w", "lin_b", "norm1_w", "norm1_b",
                                        "expand_w", "expand_b", "squeeze_w", "squeeze_b", "norm2_w", "norm2_b")]


class FusionWeights(ctypes.Structure):
    _fields_ = [("layers", ctypes.POINTER(FusionLayerWeights))] + \
               [(n, c_void_p) for n in ("img_emb_w", "img_emb_b", "pcd_emb_w", "pcd_emb_b", "img_in_w", "img_in_b", "dino_w",
                                        "dino_b", "all_w", "all_b", "pcd_in_w", "pcd_in_b", "out_w", "out_b", "src_proj",
                                        "bin_score", "prepacked")]


class CircleLossParams(ctypes.Structure):
    """dr_circle_loss_params (include/diffreg_hip.h)"""
    _fields_ = [(n, c_float) for n in ("pos_margin", "neg_margin", "pos_optimal", "neg_optimal", "log_scale", "pos_overlap", "neg_overlap")]


class FineLossParams(ctypes.Structure):
    """dr_fine_loss_params (include/diffreg_hip.h)"""
    _fields_ = [(n, c_float) for n in ("pos_radius_3d", "neg_radius_3d", "pos_radius_2d", "neg_radius_2d", "pos_margin", "neg_margin", "pos_optimal",
                                       "neg_optimal", "log_scale")]


class PlanesLinear(ctypes.Structure):
    """dr_planes_linear (include/diffreg_hip.h)"""
    _fields_ = [("rows", c_int), ("C", c_int), ("nblk", c_int),
                ("a0", c_void_p), ("bound0", c_void_p), ("k0", c_int),
                ("a1", c_void_p), ("bound1", c_void_p), ("k1", c_int),
                ("packed", c_void_p), ("mode", c_int),
                ("out", c_void_p), ("ldo", c_int), ("blk_stride", c_int),
                ("cos_t", c_void_p), ("sin_t", c_void_p), ("rot_mask", c_int), ("rot_C", c_int), ("scale", c_float),
                ("out_image", c_void_p), ("out_image_k", c_int), ("out_k0", c_int), ("out_bound", c_void_p),
                ("relu", c_int),
                ("gamma", c_void_p), ("beta", c_void_p), ("resid", c_void_p), ("ldr", c_int), ("bound_resid", c_void_p),
                ("ln_bound", c_void_p), ("bias", c_void_p), ("bias_max", c_void_p), ("ln_postadd", c_int), ("weight_layout", c_int),
                ("split_workspace", c_void_p), ("split_workspace_bytes", c_size_t)]


class Loop2D3DConfig(ctypes.Structure):
    _fields_ = [("C", c_int), ("H", c_int), ("n_layers", c_int), ("img_dim", c_int), ("dino_dim", c_int), ("pcd_dim", c_int),
                ("steps", c_int), ("sk_iters", c_int), ("sample_rate", c_float), ("max_condition_num", c_float),
                ("flags", c_int), ("h_alphas_cumprod", c_void_p), ("h_times", c_void_p)]


class LoopTrace(ctypes.Structure):
    """dr_loop_trace: per-step records and (ABI 0.2.0) the teacher-forcing inputs / outputs of the parity tests"""
    _fields_ = [("x0", c_void_p), ("R_forwd", c_void_p), ("t_forwd", c_void_p), ("cond", c_void_p), ("feats_nopos", c_void_p),
                ("feats_pos", c_void_p), ("force_x", c_void_p), ("force_R", c_void_p), ("force_t", c_void_p), ("x_next", c_void_p),
                ("topk_idx", c_void_p), ("wconf", c_void_p)]


class DebugGemmProblem(ctypes.Structure):
    """dr_debug_gemm_problem (include/diffreg_hip_debug.h): one problem of the f32-input GEMM in its internal form"""
    _fields_ = [(n, c_void_p) for n in ("A", "A2", "W", "out", "cos_t", "sin_t", "bias", "addend")] + \
               [(n, c_int) for n in ("rows", "ncols", "K", "K1", "lda", "lda2", "ldo", "epilogue", "rot_C")] + \
               [("scale", c_float), ("nbatch", c_int)] + [(n, ctypes.c_longlong) for n in ("stride_a", "stride_w", "stride_o")]


_P = ctypes.POINTER
SIGNATURES.update({
    "dr_init": (c_int, []),
    "dr_prof_enable": (None, [c_int]),
    "dr_prof_collect": (c_int, [c_void_p, c_void_p, c_void_p]),
    "dr_vol_pe_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_linear_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                              c_float, c_void_p]),
    "dr_plane_image_bytes": (c_size_t, [c_int, c_int]),
    "dr_planes_from_f32": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_planes_from_f32_bounded": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_attention_planes": (c_int, [c_int] * 5 + [c_void_p] * 10 + [c_void_p]),
    "dr_attention_planes_f16": (c_int, [c_int] * 5 + [c_void_p] * 10 + [c_void_p]),
    "dr_planes_to_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "dr_plane_weight_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dr_pack_weight_planes_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_plane_weight_bytes_wide": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dr_plane_split_workspace_bytes": (c_size_t, [c_int]),
    "dr_plane_split_status": (c_int, [c_void_p, c_void_p, c_int]),
    "dr_pack_weight_planes_wide_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_ln_bound_f32": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_linear_planes_f32": (c_int, [ctypes.POINTER(PlanesLinear), c_void_p]),
    "dr_bias_max_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_rotary_planes_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p, c_int, c_int,
                                     c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong, c_void_p]),
    "dr_loop2d3d_prepack_bytes": (c_size_t, [ctypes.POINTER(Loop2D3DConfig)]),
    "dr_loop2d3d_prepack": (c_int, [ctypes.POINTER(Loop2D3DConfig), ctypes.POINTER(FusionWeights), c_void_p, c_size_t, c_void_p]),
    "dr_gemm_nt_batched_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong, c_void_p, ctypes.c_longlong,
                                       c_float, c_void_p]),
    "dr_linear_ex_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]),
    "dr_kpconv_gather_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                     c_void_p, c_int, c_void_p]),
    "dr_kpconv_gather_mode_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                          c_int, c_int, c_void_p, c_int, c_void_p]),
    "dr_kpconv_gather_backward_mode_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                                   c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dr_col_stats_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_col_stats_f32": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_norm_apply_f32": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float,
                                  c_int, c_void_p, c_int, c_void_p]),
    "dr_gather_pool_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dr_kpconv_gather_backward_f32": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                              c_void_p, c_int, c_void_p, c_void_p]),
    "dr_norm_backward_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_norm_backward_f32": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                     c_void_p, c_float, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "dr_gather_pool_backward_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_attention_layer_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dr_attention_layer_f32": (c_int, [_P(LayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 9 +
                               [c_void_p, c_size_t, c_void_p]),
    "dr_attention_layer_pe_f32": (c_int, [_P(LayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 11 +
                                  [c_void_p, c_size_t, c_void_p]),
    "dr_attention_layer_train_saved_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dr_attention_layer_train_forward_f32": (c_int, [_P(LayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 10 + [c_size_t, c_void_p]),
    "dr_attention_layer_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dr_attention_layer_backward_f32": (c_int, [_P(LayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 12 + [_P(LayerWeights), c_void_p, c_size_t, c_void_p]),
    "dr_procrustes_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_procrustes_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 5 + [c_int, c_float, c_float] + [c_void_p] * 7 + [c_void_p, c_size_t, c_void_p]),
    "dr_device_status": (c_int, [c_void_p, c_int]),
    "dr_denoise_loop_status": (c_int, [c_void_p, c_void_p, c_int]),
    "dr_procrustes_backward_f32": (c_int, [c_int, c_int, c_int, c_int] + [c_void_p] * 9),
    "dr_debug_sinkhorn_spin_limit": (None, [ctypes.c_uint]),
    "dr_debug_enable_env": (None, [c_int]),
    "dr_debug_launch_chain": (c_int, [c_int, c_int, c_int, c_void_p]),
    "dr_debug_gemm_config": (None, [c_int]),
    "dr_debug_gemm_f32": (c_int, [_P(DebugGemmProblem), c_int, c_void_p]),
    "dr_debug_attention_config": (None, [c_int]),
    "dr_debug_attention_split": (None, [c_int]),
    "dr_debug_attention_last_form": (c_int, []),
    "dr_debug_procrustes_last_form": (c_int, []),
    "dr_debug_pgemm_acc_forms": (c_int, [c_int]),
    "dr_pnp_ransac_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_pnp_ransac_f64": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_double, ctypes.c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                  c_void_p]),
    "dr_patch_similarity_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p]),
    "dr_unique_pairs_workspace_bytes": (c_size_t, [c_int]),
    "dr_unique_pairs_i64": (c_int, [c_int, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_corr_gather_f32": (c_int, [c_int, c_void_p, c_void_p, ctypes.c_longlong, c_int] + [c_void_p] * 14),
    # ABI 0.4.0: patch partition and ground-truth overlaps of the 2D-3D model (csrc/partition2d3d.hip; wrappers in diffreg_hip/partition2d3d.py)
    "dr_point_to_node_partition_workspace_bytes": (c_size_t, [c_int]),
    "dr_point_to_node_partition_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 9 + [c_size_t, c_void_p]),
    "dr_patchify_f32": (c_int, [c_int] * 5 + [c_void_p] * 14),
    "dr_node_correspondences_2d3d_workspace_bytes": (c_size_t, [c_int, c_int, c_int, ctypes.c_longlong]),
    "dr_node_correspondences_2d3d_f32": (c_int, [c_int] * 4 + [c_void_p] * 11 + [c_float, c_float, ctypes.c_longlong] + [c_void_p] * 9 + [c_size_t, c_void_p]),
    "dr_mutual_nn_radius_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_mutual_nn_radius_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_radius_pairs_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_radius_pairs_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                    c_void_p]),
    # ABI 0.5.0: the 2D-3D point backbone's GroupNorm, kNN interpolation and KPConv neighbour count (csrc/backbone2d3d.hip; diffreg_hip/pcd_backbone2d3d.py)
    "dr_group_norm_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_group_norm_stats_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_group_norm_apply_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int] + [c_void_p] * 4 + [c_void_p, c_int] + [c_void_p] * 4 +
                                [c_float, c_int, c_void_p, c_int, c_void_p]),
    "dr_group_norm_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_group_norm_backward_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int] + [c_void_p] * 3 +
                                   [c_void_p, c_int] + [c_void_p] * 3 + [c_float, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int,
                                                                          c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_knn_interpolate_f32": (c_int, [c_int] * 4 + [c_void_p] * 5 + [c_int, c_void_p]),
    "dr_knn_interpolate_backward_f32": (c_int, [c_int] * 4 + [c_void_p] * 4 + [c_int, c_void_p, c_void_p]),
    "dr_kpconv_neighbor_count_f32": (c_int, [c_int] * 4 + [c_void_p] * 4),
    "dr_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_match_matrix_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "dr_gt_noising_f64": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "dr_focal_loss_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "dr_match_recall_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_motion_l1_f32": (c_int, [c_int, c_int] + [c_void_p] * 10),
    "dr_motion_l1_backward_f32": (c_int, [c_int, c_int] + [c_void_p] * 11),
    "dr_layernorm_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dr_layernorm_backward_workspace_bytes": (c_size_t, [c_int]),
    "dr_layernorm_backward_f32": (c_int, [c_int, c_int] + [c_void_p] * 9),
    "dr_attention_f32": (c_int, [c_int] * 5 + [c_void_p] * 3 + [c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "dr_attention_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_attention_backward_f32": (c_int, [c_int] * 5 + [c_void_p] * 5 + [c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 3 + [c_void_p, c_size_t, c_void_p]),
    "dr_softmax_rows_f32": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_dual_softmax_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_dual_softmax_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_dual_softmax_backward_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_softmax_backward_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "dr_relu_backward_f32": (c_int, [ctypes.c_longlong, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_rotary_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "dr_focal_loss_backward_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "dr_sinkhorn_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dr_sinkhorn_backward_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
    "dr_scatter_rows_f32": (c_int, [c_int, c_int, c_void_p, ctypes.c_int64, c_void_p, c_void_p, c_void_p, ctypes.c_int64, c_void_p, c_void_p]),
    "dr_mutual_match_f64": (c_int, [c_int, c_int, c_int, c_void_p, c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_mutual_match_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_top1_union_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dr_top1_union_f64": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_top1_union_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_loop_prepack_bytes": (c_size_t, [_P(LoopConfig)]),
    "dr_loop_prepack": (c_int, [_P(LoopConfig), _P(LoopWeights), c_void_p, c_size_t, c_void_p]),
    "dr_denoise_loop_workspace_bytes": (c_size_t, [_P(LoopConfig), c_int, c_int, c_int]),
    "dr_denoise_loop": (c_int, [_P(LoopConfig), _P(LoopWeights), c_int, c_int, c_int] + [c_void_p] * 14 +
                        [_P(LoopTrace), c_void_p, c_size_t, c_void_p]),
    "dr_denoise_loop_2d3d_workspace_bytes": (c_size_t, [_P(Loop2D3DConfig), c_int, c_int, c_int]),
    "dr_denoise_loop_2d3d": (c_int, [_P(Loop2D3DConfig), _P(FusionWeights), c_int, c_int, c_int] + [c_void_p] * 16 +
                             [_P(LoopTrace), c_void_p, c_size_t, c_void_p]),
    "dr_inlier_ratio_f32": (c_int, [c_int] * 4 + [c_void_p] * 7 + [c_float, c_void_p, c_void_p, c_void_p]),
    "dr_nrfmr_f32": (c_int, [c_int] * 4 + [c_void_p] * 9 + [c_int, c_void_p, c_void_p, c_float, c_float] + [c_void_p] * 4),
    "dr_ransac_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_ransac_corr_f64": (c_int, [c_int] * 4 + [c_void_p] * 4 + [c_double, c_int, ctypes.c_uint64] + [c_void_p] * 7 +
                           [c_size_t, c_void_p]),
    "dr_registration_recall_f64": (c_int, [c_int] + [c_void_p] * 5 + [c_double, c_void_p, c_void_p, c_void_p]),
    "dr_grid_subsample_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_grid_subsample_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "dr_grid_subsample_vision3d_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "dr_radius_count_hist_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_radius_count_hist_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 4 + [c_float, c_int] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dr_radius_neighbors_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_radius_neighbors_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 4 + [c_float, c_int] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dr_mutual_topk_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_mutual_topk_select_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_float, c_int] + [c_void_p] * 4 +
                                  [ctypes.c_longlong, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_denoiser_match_f32": (c_int, [_P(LoopConfig), _P(LoopWeights), c_int, c_int, c_int] + [c_void_p] * 9 +
                              [c_void_p, c_size_t, c_void_p]),    # ABI 0.3.0: the 2D-3D training branch (dr_fusion_layer_grads has the layout of dr_fusion_layer_weights: FusionLayerWeights binds both)
    "dr_fusion_layer_train_saved_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "dr_fusion_layer_train_forward_f32": (c_int, [_P(FusionLayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    "dr_fusion_layer_backward_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "dr_fusion_layer_backward_f32": (c_int, [_P(FusionLayerWeights), c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 7 +
                                     [_P(FusionLayerWeights), c_void_p, c_size_t, c_void_p]),
    "dr_l2_normalize_f32": (c_int, [c_int, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dr_l2_normalize_backward_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dr_circle_loss_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_circle_loss_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 4 + [_P(CircleLossParams), c_void_p, c_void_p,
                                                                                                       c_size_t, c_void_p]),
    "dr_circle_loss_backward_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 4 +
                                    [_P(CircleLossParams)] + [c_void_p] * 5 + [c_size_t, c_void_p]),
    # ABI 0.6.0: the 2D-3D fine loss
    "dr_fine_loss_saved_bytes": (c_size_t, [c_int]),
    "dr_fine_loss_f32": (c_int, [c_int] * 4 + [c_void_p] * 8 + [c_int, _P(FineLossParams), c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_fine_loss_backward_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_fine_loss_backward_f32": (c_int, [c_int] * 4 + [c_void_p] * 8 + [c_int, _P(FineLossParams), c_void_p, c_size_t] + [c_void_p] * 4 +
                                  [c_size_t, c_void_p]),
    # ABI 0.7.0: the 2D-3D evaluation metrics
    "dr_sparse_corr_eval_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_sparse_corr_eval_i64": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                        c_void_p, c_size_t, c_void_p]),
    "dr_corr_eval_workspace_bytes": (c_size_t, [c_int]),
    "dr_corr_eval_f32": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_double, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                 c_void_p]),
    "dr_registration_eval_workspace_bytes": (c_size_t, [c_int]),
    "dr_registration_eval_f64": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    # ABI 0.7.0, second set: the geometry head and the feature-layout glue of the 2D-3D forward
    "dr_back_project_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_float, c_float, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "dr_render_f32": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "dr_resize_tokens_f32": (c_int, [c_int] * 5 + [c_void_p] * 3),
    "dr_resize_tokens_backward_f32": (c_int, [c_int] * 5 + [c_void_p] * 3),
    "dr_rows_normalize_chw_f32": (c_int, [c_int, ctypes.c_int64, c_void_p, c_void_p, c_void_p]),
    "dr_rows_normalize_chw_backward_f32": (c_int, [c_int, ctypes.c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dr_rows_normalize_chw_backward_rows_f32": (c_int, [c_int, ctypes.c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # ABI 0.7.0, fourth set: the image backbone's inference forward on token rows
    "dr_conv2d_rows_f32": (c_int, [c_int] * 8 + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "dr_resize_rows_f32": (c_int, [c_int] * 5 + [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    # ABI 0.7.0, fifth set: the image backbone's backward on token rows
    "dr_conv2d_rows_backward_data_f32": (c_int, [c_int] * 8 + [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "dr_conv2d_rows_backward_weight_workspace_bytes": (c_size_t, [c_int] * 8),
    "dr_conv2d_rows_backward_weight_f32": (c_int, [c_int] * 8 + [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_resize_rows_backward_f32": (c_int, [c_int] * 5 + [c_void_p, c_int, c_void_p, c_int, c_void_p]),
})


class GemmRowsF16Args(ctypes.Structure):
    """dr_gemm_rows_f16_args"""
    _fields_ = [("a", c_void_p), ("w_packed", c_void_p), ("bias", c_void_p), ("gamma", c_void_p), ("addend", c_void_p), ("out", c_void_p),
                ("M", c_int), ("K", c_int), ("N", c_int), ("lda", c_int), ("ldo", c_int), ("ld_addend", c_int), ("mode", c_int),
                ("colscale_cols", c_int), ("colscale", c_float)]


class VitBlockF16(ctypes.Structure):
    """dr_vit_block_f16"""
    _fields_ = [(n, c_void_p) for n in ("norm1_g", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_g", "norm2_b", "fc1_w", "fc1_b",
                                        "fc2_w", "fc2_b", "ls2")]


class VitConfigF16(ctypes.Structure):
    """dr_vit_config_f16"""
    _fields_ = [("H", c_int), ("W", c_int), ("p", c_int), ("D", c_int), ("heads", c_int), ("Dh", c_int), ("depth", c_int), ("eps", c_float),
                ("img", c_void_p), ("img_f32", c_int), ("patch_w", c_void_p), ("patch_b", c_void_p), ("cls", c_void_p), ("pos", c_void_p),
                ("blocks", ctypes.POINTER(VitBlockF16)), ("norm_g", c_void_p), ("norm_b", c_void_p), ("x_prenorm", c_void_p), ("x_norm", c_void_p),
                ("n_take", c_int), ("take", ctypes.POINTER(c_int)), ("take_out", ctypes.POINTER(c_void_p)), ("workspace", c_void_p),
                ("workspace_bytes", c_size_t)]


SIGNATURES.update({
    # added after ABI 0.7.0, sixth set: the fp16 ViT encoder (csrc/vit.hip)
    "dr_pack_weight_f16_bytes": (c_size_t, [c_int, c_int]),
    "dr_pack_weight_f16": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dr_gemm_rows_f16": (c_int, [ctypes.POINTER(GemmRowsF16Args), c_void_p]),
    "dr_layernorm_rows_f16": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_void_p, c_int, c_void_p]),
    "dr_attention_rows_f16": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "dr_patch_rows_f16": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "dr_vit_workspace_bytes": (c_size_t, [c_int] * 5),
    "dr_vit_forward_f16": (c_int, [ctypes.POINTER(VitConfigF16), c_void_p]),
    "dr_debug_gemm_rows_tile": (None, [c_int]),
    # added after ABI 0.7.0, seventh set: the Depth-Anything DPT head's forward on token rows (csrc/conv2d.hip)
    "dr_conv2d_rows_act_f32": (c_int, [c_int] * 8 + [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                       c_void_p]),
    "dr_conv_transpose2d_rows_f32": (c_int, [c_int] * 5 + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "dr_conv2d_rows_project_f32": (c_int, [c_int] * 8 + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p]),
})


class GemmRowsF32Args(ctypes.Structure):
    """dr_gemm_rows_f32_args"""
    _fields_ = [("a", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("gamma", c_void_p), ("addend", c_void_p), ("out", c_void_p),
                ("M", c_int), ("K", c_int), ("N", c_int), ("lda", c_int), ("ldw", c_int), ("ldo", c_int), ("ld_addend", c_int), ("mode", c_int),
                ("colscale_cols", c_int), ("colscale", c_float)]


class VitBlockF32(ctypes.Structure):
    """dr_vit_block_f32"""
    _fields_ = [(n, c_void_p) for n in ("norm1_g", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "norm2_g", "norm2_b", "fc1_w", "fc1_b",
                                        "fc2_w", "fc2_b", "ls2")]


class VitConfigF32(ctypes.Structure):
    """dr_vit_config_f32"""
    _fields_ = [("H", c_int), ("W", c_int), ("p", c_int), ("D", c_int), ("heads", c_int), ("Dh", c_int), ("depth", c_int), ("eps", c_float),
                ("img", c_void_p), ("patch_w", c_void_p), ("patch_b", c_void_p), ("cls", c_void_p), ("pos", c_void_p),
                ("blocks", ctypes.POINTER(VitBlockF32)), ("norm_g", c_void_p), ("norm_b", c_void_p), ("x_prenorm", c_void_p), ("x_norm", c_void_p),
                ("n_take", c_int), ("norm_take", c_int), ("take", ctypes.POINTER(c_int)), ("take_out", ctypes.POINTER(c_void_p)),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


SIGNATURES.update({
    # added after ABI 0.7.0, eighth set: Depth-Anything's float32 ViT encoder (csrc/vit_f32.hip)
    "dr_gemm_rows_f32": (c_int, [ctypes.POINTER(GemmRowsF32Args), c_void_p]),
    "dr_patch_rows_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "dr_vit_workspace_bytes_f32": (c_size_t, [c_int] * 5),
    "dr_vit_forward_f32": (c_int, [ctypes.POINTER(VitConfigF32), c_void_p]),
    "dr_debug_gemm_rows_f32_tile": (None, [c_int]),
})


class ImageNorm(ctypes.Structure):
    """dr_image_norm"""
    _fields_ = [("mean", ctypes.c_double * 3), ("std", ctypes.c_double * 3)]


SIGNATURES.update({
    # added after ABI 0.7.0, tenth set: the input transform in front of Depth-Anything (csrc/image_transform.hip)
    "dr_image_cubic_chw_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(ImageNorm), c_void_p, c_void_p]),
})
SIGNATURES.update({
    # added after ABI 0.7.0, eleventh set: the ground-truth half of the 3D / 4D training collate (csrc/collate_gt.hip)
    "dr_blend_flow_knn3_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 8),
    "dr_coarse_gt_matches_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_coarse_gt_matches_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 7 + [c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
})


class OptimTensor(ctypes.Structure):
    """dr_optim_tensor"""
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("state0", c_void_p), ("state1", c_void_p), ("numel", c_size_t)]


class SgdOptions(ctypes.Structure):
    """dr_sgd_options"""
    _fields_ = [("lr", c_double), ("weight_decay", c_double), ("momentum", c_double), ("dampening", c_double),
                ("nesterov", c_int), ("maximize", c_int), ("zero_grads", c_int)]


class AdamOptions(ctypes.Structure):
    """dr_adam_options"""
    _fields_ = [("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
                ("decoupled", c_int), ("maximize", c_int), ("zero_grads", c_int)]


SIGNATURES.update({
    # added after ABI 0.7.0, twelfth set: the gradient gate and the SGD / Adam update (csrc/optim.hip)
    "dr_grads_finite_multi_f32": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "dr_sgd_step_multi_f32": (c_int, [c_void_p, c_size_t, ctypes.POINTER(SgdOptions), c_void_p, c_void_p, c_void_p]),
    "dr_adam_step_multi_f32": (c_int, [c_void_p, c_size_t, ctypes.POINTER(AdamOptions), c_void_p, c_void_p, c_void_p]),
    "dr_optim_finish": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
})
_ITEM_ARGS = [c_int, c_int, c_int, c_void_p, c_double, c_double, c_void_p, c_void_p, c_int, c_void_p, c_double, c_double]
SIGNATURES.update({
    # added after ABI 0.7.0, thirteenth set: the pixel-point ground truth of a 2D-3D dataset item (csrc/item2d3d.hip)
    "dr_corr_2d3d_mutual_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_corr_2d3d_mutual_f64": (c_int, _ITEM_ARGS + [ctypes.c_longlong] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dr_corr_2d3d_radius_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_corr_2d3d_radius_f64": (c_int, _ITEM_ARGS + [ctypes.c_longlong] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dr_overlap_2d3d_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_overlap_2d3d_f64": (c_int, _ITEM_ARGS + [ctypes.c_longlong] * 2 + [c_void_p] * 4 + [c_size_t, c_void_p]),
    "dr_column_mean_seq_f32": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
})


class NicpProblem(ctypes.Structure):
    """dr_nicp_problem"""
    _fields_ = [("P", c_int), ("n_corr", c_int), ("n_nodes", c_int), ("n_edges", c_int), ("K", c_int), ("max_nodes", c_int),
                ("nodes", c_void_p), ("m_offsets", c_void_p), ("src_corr", c_void_p), ("tgt_corr", c_void_p), ("c_offsets", c_void_p),
                ("anchor_indices", c_void_p), ("anchor_weights", c_void_p), ("edges", c_void_p), ("edge_weights", c_void_p),
                ("e_offsets", c_void_p)]


class NicpOptions(ctypes.Structure):
    """dr_nicp_options"""
    _fields_ = [("num_iterations", c_int), ("lr", c_double), ("gamma", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("w_landmark", c_double), ("w_arap", c_double), ("w_ortho", c_double)]


class NicpState(ctypes.Structure):
    """dr_nicp_state"""
    _fields_ = [("rotations", c_void_p), ("translations", c_void_p), ("exp_avg_rot", c_void_p), ("exp_avg_trn", c_void_p),
                ("exp_avg_sq_rot", c_void_p), ("exp_avg_sq_trn", c_void_p), ("step", c_void_p)]


SIGNATURES.update({
    # added after ABI 0.7.0, fourteenth set: non-rigid ICP on an embedded deformation graph (csrc/nonrigid.hip)
    "dr_nicp_node_capacity": (c_int, []),
    "dr_ed_graph_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_ed_graph_f32": (c_int, [c_int] * 5 + [c_void_p] * 4 + [c_double, c_double] + [c_void_p] * 5 + [ctypes.c_longlong] + [c_void_p] * 5
                        + [c_size_t, c_void_p]),
    "dr_ed_warp_f32": (c_int, [c_int] * 4 + [c_void_p] * 7 + [c_double] + [c_void_p] * 3),
    "dr_nicp_workspace_bytes": (c_size_t, [c_int] * 5),
    "dr_nicp_cost_grad_f32": (c_int, [ctypes.POINTER(NicpProblem), c_void_p, c_void_p, c_double, c_double, c_double] + [c_void_p] * 5
                              + [c_size_t, c_void_p]),
    "dr_nicp_adam_f32": (c_int, [ctypes.POINTER(NicpProblem), ctypes.POINTER(NicpOptions), ctypes.POINTER(NicpState), c_int] + [c_void_p] * 5
                         + [c_size_t, c_void_p]),
})


class Item3dArgs(ctypes.Structure):
    """dr_item3d_args"""
    _fields_ = [("P", c_int), ("n_src_raw", c_int), ("n_tgt_raw", c_int), ("n_src", c_int), ("n_tgt", c_int),
                ("src_raw", c_void_p), ("s_raw_offsets", c_void_p), ("tgt_raw", c_void_p), ("t_raw_offsets", c_void_p), ("flow_raw", c_void_p),
                ("src_sel", c_void_p), ("tgt_sel", c_void_p), ("s_offsets", c_void_p), ("t_offsets", c_void_p), ("rot_ab", c_void_p),
                ("coin", c_void_p), ("src_jitter", c_void_p), ("tgt_jitter", c_void_p), ("noise", c_double), ("recompute_flow", c_int),
                ("rot", c_void_p), ("trans", c_void_p), ("src_out", c_void_p), ("tgt_out", c_void_p), ("flow_out", c_void_p),
                ("rot_out", c_void_p), ("trans_out", c_void_p), ("tsfm_out", c_void_p), ("status", c_void_p)]


SIGNATURES.update({
    # added after ABI 0.7.0, fifteenth set: the 3D / 4D dataset item (csrc/item3d.hip)
    "dr_item3d_prepare_f32": (c_int, [ctypes.POINTER(Item3dArgs), c_void_p]),
    "dr_radius_pairs_ragged_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_radius_pairs_ragged_f32": (c_int, [c_int, c_int, c_int] + [c_void_p] * 5 + [c_float, c_void_p, ctypes.c_longlong] + [c_void_p] * 5
                                   + [c_size_t, c_void_p]),
})


class NicpGnOptions(ctypes.Structure):
    """dr_nicp_gn_options"""
    _fields_ = [("num_iterations", c_int), ("corr_lambda", c_double), ("arap_lambda", c_double), ("lm_lambda", c_double)]


SIGNATURES.update({
    # added after ABI 0.7.0, sixteenth set: Gauss-Newton non-rigid ICP and the batched SPD factor-and-solve (csrc/nonrigid_gn.hip)
    "dr_nicp_gn_workspace_bytes": (c_size_t, [c_int] * 6),
    "dr_nicp_gn_f32": (c_int, [ctypes.POINTER(NicpProblem), ctypes.POINTER(NicpGnOptions), c_void_p, ctypes.POINTER(NicpState), c_int]
                       + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "dr_nicp_gn_normal_f32": (c_int, [ctypes.POINTER(NicpProblem), ctypes.POINTER(NicpGnOptions)] + [c_void_p] * 7 + [c_size_t, c_void_p]),
    "dr_spd_solve_f64": (c_int, [c_int, c_int] + [c_void_p] * 5),
})


SIGNATURES.update({
    # added after ABI 0.7.0, seventeenth set: furthest-point sampling (csrc/fps.hip); the debug setter forces the streaming instantiation
    "dr_fps_onchip_capacity": (c_int, []),
    "dr_fps_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_fps_nodes_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int, c_int] + [c_void_p] * 6 + [c_size_t, c_void_p]),
    "dr_fps_batch_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_debug_fps_force_streaming": (None, [c_int]),
})


class GeoGraphOptions(ctypes.Structure):
    """dr_geo_graph_options"""
    _fields_ = [("num_neighbors", c_int), ("num_anchors", c_int), ("max_distance", c_float), ("node_coverage", c_float), ("max_degree", c_int),
                ("onchip_cap_override", c_int)]


SIGNATURES.update({
    # added after ABI 0.7.0, eighteenth set: the geodesic deformation graph of a point cloud (csrc/geo_graph.hip)
    "dr_geo_graph_onchip_capacity": (c_int, []),
    "dr_geo_graph_workspace_bytes": (c_size_t, [c_int] * 5),
    "dr_geo_graph_f32": (c_int, [c_int] * 5 + [c_void_p] * 4 + [ctypes.POINTER(GeoGraphOptions)] + [c_void_p] * 8 + [c_size_t, c_void_p]),
    "dr_geo_graph_edges": (c_int, [c_int] * 3 + [c_void_p] * 5 + [ctypes.c_longlong] + [c_void_p] * 3),
})


SIGNATURES.update({
    # added after ABI 0.7.0, nineteenth set: the non-rigid evaluation (csrc/knn_points.hip)
    "dr_knn_points_max_k": (c_int, []),
    "dr_knn_points_tile": (c_int, []),
    "dr_knn_points_block": (c_int, []),
    "dr_knn_points_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 4 + [c_int] + [c_void_p] * 4),
    "dr_nn_stats_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_nn_stats_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 4 + [c_float] + [c_void_p] * 3 + [c_size_t, c_void_p]),
    "dr_flow_metrics_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_flow_metrics_f32": (c_int, [c_int, c_int] + [c_void_p] * 7 + [c_float] * 7 + [c_void_p] * 3 + [c_size_t, c_void_p]),
})

SIGNATURES.update({
    # added after ABI 0.7.0, twentieth set: the RANSAC-free rigid estimators (csrc/lgr.hip; wrappers in diffreg_hip/registration.py)
    "dr_lgr_wave_limit": (c_int, []),
    "dr_sc_block": (c_int, []),
    "dr_sc_tile": (c_int, []),
    "dr_weighted_procrustes_f32": (c_int, [c_int, c_int] + [c_void_p] * 5 + [c_float, c_float, c_int] + [c_void_p] * 3),
    "dr_lgr_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_lgr_f32": (c_int, [c_int, c_int] + [c_void_p] * 5 + [c_int] + [c_void_p] * 6 + [c_float, c_int, c_int, c_float, c_float] +
                   [c_void_p] * 8 + [c_size_t, c_void_p]),
    "dr_spatial_consistency_f32": (c_int, [c_int, c_int] + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 + [c_float] + [c_void_p] * 4),
    "dr_sc_row_sums_f32": (c_int, [c_int, c_int] + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 + [c_float] + [c_void_p] * 4),
    "dr_sc_leading_eigenvector_workspace_bytes": (c_size_t, [c_int, c_int]),
    "dr_sc_leading_eigenvector_f32": (c_int, [c_int, c_int] + [c_void_p] * 4 + [c_float] + [c_void_p] * 2 + [c_int] + [c_void_p] * 4 +
                                      [c_size_t, c_void_p]),
})


SIGNATURES.update({
    # added after ABI 0.7.0, twenty-first set: point-to-point ICP (csrc/icp.hip; wrappers in diffreg_hip/registration.py) and Open3D's voxel origin
    "dr_icp_p2p_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "dr_icp_p2p_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int] + [c_void_p] * 5 + [c_float, c_int, c_float, c_float] +
                       [c_void_p] * 7 + [c_size_t, c_void_p]),
    "dr_grid_subsample_open3d_f32": (c_int, [c_int, c_int, c_void_p, c_void_p, c_float] + [c_void_p] * 5 + [c_size_t, c_void_p]),
})


class DebugDdimArgs(ctypes.Structure):
    """dr_debug_ddim_args (include/diffreg_hip_debug.h): the DDIM kernel's launch argument, field for field"""
    _fields_ = [(n, c_void_p) for n in ("x", "x0", "shift", "noise", "src_mask", "tgt_mask")] + \
               [(n, c_int) for n in ("N", "M", "first_step")] + [(n, c_double) for n in ("sra", "srm1", "c", "sigma")] + [("sqrt_an", c_float)]


SIGNATURES.update({
    # diagnostics (include/diffreg_hip_debug.h): one launch of a row / state kernel of the loops, for tests/test_row_state_edges_gpu.py
    "dr_debug_layernorm_f32": (c_int, [c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dr_debug_fourier_f32": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "dr_debug_pair_min_scratch_bytes": (c_size_t, [c_int]),
    "dr_debug_pair_min_f64": (c_int, [c_int, c_int, c_int] + [c_void_p] * 6),
    "dr_debug_ddim_f64": (c_int, [ctypes.POINTER(DebugDdimArgs), c_int, c_void_p]),
    "dr_debug_state_map": (c_int, [c_int, c_void_p, c_void_p, ctypes.c_longlong, c_void_p]),
})


def _bind(table):
    for name, (res, args) in table.items():
        if not hasattr(_lib, name):          # the sets added under one ABI number are detected by symbol
            raise ImportError("libdiffreg_hip.so has no %s: it was built from an older tree than this binding; rebuild (make -C diff-reg_amd/csrc)"
                              % name)
        fn = getattr(_lib, name)
        fn.restype = res
        fn.argtypes = args


_bind(SIGNATURES)
_INIT_DONE = False

ABI_VERSION = 700          # DR_ABI_VERSION of the include/diffreg_hip.h these signatures were written against
if _lib.dr_version() // 100 != ABI_VERSION // 100:
    raise ImportError("libdiffreg_hip.so is ABI %d, this binding is written against %d: rebuild (make -C diff-reg_amd/csrc)"
                      % (_lib.dr_version(), ABI_VERSION))


def ensure_init():
    """kernel attributes (dynamic LDS) -- needs a GPU, so it runs lazily before the first launch."""
    global _INIT_DONE
    if not _INIT_DONE:
        # tools/ only: the library ignores the DR_* tuning variables unless this one explicit switch is set
        if os.environ.get("DR_DIAGNOSTICS") == "1":
            _lib.dr_debug_enable_env(1)
        check(_lib.dr_init())
        _INIT_DONE = True


SK_OUT_CONF, SK_OUT_LOG, SK_MINSHIFT, SK_APPLY_MASK, SK_OUT_F32, SK_STRICT = 0x0, 0x1, 0x2, 0x4, 0x8, 0x10
SK_RAGGED = 0x20    # rows / columns outside the masks do not exist (a padded tile = its unpadded problem)


def raw():
    return _lib


def check(code):
    if code != 0:
        msg = _lib.dr_strerror(code).decode()
        if code == -2:
            msg += ": " + _lib.dr_last_hip_error().decode()
        raise RuntimeError("libdiffreg_hip: %s (%d)" % (msg, code))


def loop_status(workspace, clear=True):
    """dr_denoise_loop_status: waits for the current stream of the workspace's device and raises if the LAST loop call that ran on this
    workspace reported a device-side failure (DR_ETIMEOUT of a co-resident Sinkhorn launch).  The word belongs to the workspace, so
    concurrent engines / concurrent batches of one engine (one workspace each) are told apart."""
    st = torch.cuda.current_stream(workspace.device).cuda_stream
    check(_lib.dr_denoise_loop_status(ptr(workspace), c_void_p(st), 1 if clear else 0))


def device_status(device=None, clear=True):
    """Waits for the current stream of `device` and raises if a kernel reported a device-side failure since the last check
    (DR_ETIMEOUT: the single-launch Sinkhorn gave up waiting for a workgroup that was not resident; the outputs of that call are
    unspecified -- the flag is process-wide and sticky: the first reader with clear=True consumes it; DR_EINVAL: an evaluation entry of the
    2D-3D metrics skipped an index outside its range, where the reference raises an IndexError).
    Called wherever the host mirrors synchronise anyway (match counts)."""
    st = torch.cuda.current_stream(device).cuda_stream
    check(_lib.dr_device_status(c_void_p(st), 1 if clear else 0))


def ptr(t):
    """device pointer of a contiguous ROCm tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libdiffreg_hip ops need tensors on a ROCm device (got %s); there is no CPU path" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("libdiffreg_hip ops need contiguous tensors")
    return c_void_p(t.data_ptr())


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """the current HIP stream of the tensor's device as a void* (the raw-handle query where this torch build has it: a tenth of the cost of building
    a torch.cuda.Stream object, and every library call makes one)"""
    if _RAW_STREAM is not None:
        dev = t.device
        return c_void_p(_RAW_STREAM(dev.index if dev.index is not None else torch.cuda.current_device()))
    return c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def mask_u8(m):
    if m is None:
        return None
    if m.dtype == torch.bool:
        return m.contiguous().view(torch.uint8)
    return (m != 0).contiguous().view(torch.uint8)


# ---- plane images (two-plane fp16 operand images of the layer GEMMs) -------------------------------------------------
PL_F32, PL_PLANES, PL_LN = 0, 1, 2


def planes_from_f32(x):
    """x [rows, K] fp32 -> (image uint8, bound [rows])"""
    ensure_init()
    x = x.contiguous()
    rows, K = x.shape
    img = torch.zeros(_lib.dr_plane_image_bytes(rows, K), dtype=torch.uint8, device=x.device)
    bnd = torch.empty(rows, device=x.device)
    check(_lib.dr_planes_from_f32(rows, K, ptr(x), K, ptr(img), ptr(bnd), stream_of(x)))
    return img, bnd


def planes_from_f32_bounded(x, bound_in):
    ensure_init()
    x = x.contiguous()
    rows, K = x.shape
    img = torch.zeros(_lib.dr_plane_image_bytes(rows, K), dtype=torch.uint8, device=x.device)
    bnd = torch.empty(rows, device=x.device)
    check(_lib.dr_planes_from_f32_bounded(rows, K, ptr(x), K, ptr(bound_in.contiguous()), ptr(img), ptr(bnd), stream_of(x)))
    return img, bnd


def attention_planes(q, k, v, H, q_mask=None, k_mask=None, f16=False):
    """q [P,Lq,C], k, v [P,Lk,C] float32 (rotary already applied) -> softmax(q k^T / sqrt(d)) v per head, [P,Lq,C], through the
    plane-image attention kernel (images built here: head-padded columns, one k / v bound per segment)."""
    ensure_init()
    P, Lq, C = q.shape
    Lk = k.shape[1]
    d = C // H
    dp = (d + 15) // 16 * 16

    def pad(x):
        y = torch.zeros(x.shape[0] * x.shape[1], H * dp, device=x.device)
        xr = x.reshape(-1, H, d)
        y.view(-1, H, dp)[:, :, :d] = xr
        return y
    qi, qb = planes_from_f32(pad(q))
    kb_in = k.abs().amax((1, 2)).repeat_interleave(Lk)
    vb_in = v.abs().amax((1, 2)).repeat_interleave(Lk)
    ki, kb = planes_from_f32_bounded(pad(k), kb_in)
    vi, vb = planes_from_f32_bounded(pad(v), vb_in)
    oi = torch.zeros(_lib.dr_plane_image_bytes(P * Lq, H * dp), dtype=torch.uint8, device=q.device)
    ob = torch.zeros(P * Lq, device=q.device)
    check((_lib.dr_attention_planes_f16 if f16 else _lib.dr_attention_planes)(P, Lq, Lk, H, d, ptr(qi), ptr(qb), ptr(ki), ptr(kb), ptr(vi), ptr(vb), ptr(mask_u8(q_mask)), ptr(mask_u8(k_mask)),
                                   ptr(oi), ptr(ob), stream_of(q)))
    o = planes_to_f32(oi, ob, P * Lq, H * dp).view(P * Lq, H, dp)[:, :, :d]
    return o.reshape(P, Lq, C)


def planes_to_f32(img, bnd, rows, K):
    out = torch.empty(rows, K, device=img.device)
    check(_lib.dr_planes_to_f32(rows, K, ptr(img), ptr(bnd), ptr(out), K, stream_of(out)))
    return out


def pack_weight_planes(W, nblk, C, piece_len=None, piece_pad=None, wide=False):
    """W [nblk * C, K] -> packed image (uint8 tensor); wide: the wide-wave layout (dr_pack_weight_planes_wide_f32; pass wide=True to linear_planes too)"""
    ensure_init()
    W = W.contiguous()
    K = W.shape[1]
    piece_len = piece_len or K
    piece_pad = piece_pad or K
    nbytes = (_lib.dr_plane_weight_bytes_wide if wide else _lib.dr_plane_weight_bytes)(nblk, C, K, piece_len, piece_pad)
    if nbytes == 0:
        raise RuntimeError("unsupported plane weight shape")
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=W.device)
    check((_lib.dr_pack_weight_planes_wide_f32 if wide else _lib.dr_pack_weight_planes_f32)(nblk, C, K, piece_len, piece_pad, ptr(W), ptr(buf), stream_of(W)))
    return buf


def ln_bound(gamma, beta):
    out = torch.empty(1, device=gamma.device)
    check(_lib.dr_ln_bound_f32(gamma.numel(), ptr(gamma), ptr(beta), ptr(out), stream_of(gamma)))
    return out


def linear_planes(rows, C, nblk, a0, b0, k0, packed, mode, *, a1=None, b1=None, k1=0, out=None, ldo=0, blk_stride=0, cos_t=None,
                  sin_t=None, rot_mask=0, rot_C=0, scale=1.0, out_image=None, out_image_k=0, out_k0=0, out_bound=None, relu=False,
                  gamma=None, beta=None, resid=None, ldr=0, bound_resid=None, lnb=None, bias=None, ln_postadd=False, wide=False, split_ws=None):
    """dr_linear_planes_f32; bias [nblk * C]: its per-block maxima are computed here (dr_bias_max_f32).  split_ws: a uint8 tensor of
    plane_split_workspace(C) bytes -- lets a launch that fills at most half the chip split its tiles' k range over two workgroups"""
    a = PlanesLinear()
    a.rows, a.C, a.nblk = rows, C, nblk
    dp = lambda t_: None if t_ is None else t_.data_ptr()
    a.a0, a.bound0, a.k0 = dp(a0), dp(b0), k0
    a.a1, a.bound1, a.k1 = dp(a1), dp(b1), k1
    a.packed, a.mode = dp(packed), mode
    a.out, a.ldo, a.blk_stride = dp(out), ldo, blk_stride
    a.cos_t, a.sin_t, a.rot_mask, a.rot_C, a.scale = dp(cos_t), dp(sin_t), rot_mask, rot_C, scale
    a.out_image, a.out_image_k, a.out_k0, a.out_bound = dp(out_image), out_image_k, out_k0, dp(out_bound)
    a.relu = 1 if relu else 0
    a.gamma, a.beta, a.resid, a.ldr, a.bound_resid, a.ln_bound = dp(gamma), dp(beta), dp(resid), ldr, dp(bound_resid), dp(lnb)
    bmax = None
    if bias is not None:
        bias = bias.contiguous().float()
        bmax = torch.empty(nblk, device=bias.device)
        check(_lib.dr_bias_max_f32(nblk, C, ptr(bias), ptr(bmax), stream_of(a0)))
    a.bias, a.bias_max, a.ln_postadd = dp(bias), dp(bmax), 1 if ln_postadd else 0
    a.weight_layout = 1 if wide else 0
    a.split_workspace, a.split_workspace_bytes = dp(split_ws), (split_ws.numel() if split_ws is not None else 0)
    check(_lib.dr_linear_planes_f32(ctypes.byref(a), stream_of(a0)))


def rotary_planes(x, x_blk, C, nblk, cs_t, rot_mask, rot_C, b0, packed, k, out_image, image_blk_stride, out_bound, bound_blk_stride, scale=1.0,
                  wide=False):
    """dr_rotary_planes_f32: x [rows, ldx] fp32 (what linear_planes wrote in PL_F32 mode without rotary) -> the images and bounds of PL_PLANES"""
    ensure_init()
    check(_lib.dr_rotary_planes_f32(x.shape[0], C, nblk, ptr(x), x.stride(0), x_blk, ptr(cs_t), rot_mask, rot_C, scale, ptr(b0), ptr(packed), k,
                                    1 if wide else 0, ptr(out_image), image_blk_stride, ptr(out_bound), bound_blk_stride, stream_of(x)))


def plane_split_workspace(C, device):
    """the exchange workspace of dr_planes_linear.split_workspace (uint8 tensor)"""
    return torch.empty(_lib.dr_plane_split_workspace_bytes(C), dtype=torch.uint8, device=device)


def plane_split_status(split_ws, clear=True):
    """raises (DR_ETIMEOUT) if a workgroup of the last split launch on this workspace never met its partner"""
    check(_lib.dr_plane_split_status(ptr(split_ws), stream_of(split_ws), 1 if clear else 0))


def scatter_rows(src, src_index, dst_index, dst, validate=True, status=None):
    """dst[dst_index[i]] = src[src_index[i]] (rows; split_feats of the reference).  Index tensors may live on the host (torch
    indexing accepts that); out-of-range indices raise IndexError like torch's indexed assignment (validate=True reads a 4-byte
    device flag, i.e. synchronises the stream; validate=False leaves such rows unwritten and the flag unread: pass `status`, a zeroed
    int32 device tensor, to share one flag between several calls and check it once with scatter_rows_check)."""
    ensure_init()
    src = src.contiguous().float()
    si = src_index.to(device=src.device, dtype=torch.int64).contiguous()
    di = dst_index.to(device=src.device, dtype=torch.int64).contiguous()
    assert dst.is_contiguous() and dst.dtype == torch.float32 and dst.shape[-1] == src.shape[-1] and dst.device == src.device
    assert si.numel() == di.numel()
    C = src.shape[-1]
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=src.device)
    check(_lib.dr_scatter_rows_f32(si.numel(), C, ptr(src), src.numel() // C, ptr(si), ptr(di), ptr(dst), dst.numel() // C,
                                   ptr(status), stream_of(src)))
    if validate and int(status.item()):
        raise IndexError("scatter_rows: index out of range (src rows %d, dst rows %d)" % (src.numel() // C, dst.numel() // C))
    return dst


def scatter_rows_check(status):
    if int(status.item()):
        raise IndexError("scatter_rows: index out of range")


# ---- forward half of the training branch (csrc/train.hip) -------------------------------------------------------------------------
MATCH_SINKHORN, MATCH_DUAL_SOFTMAX = 0, 1


def _train_ws(P, N, M, dev):
    return torch.empty(_lib.dr_train_workspace_bytes(P, N, M), dtype=torch.uint8, device=dev)


def match_matrix(matches, P, N, M):
    """rows (b, i, j) of matches [K,3] int64 -> [P,N,M] float32 with 1 at the rows (match_2_conf_matrix, loss.py:316-320)"""
    ensure_init()
    matches = matches.to(torch.int64).contiguous()
    out = torch.empty(P, N, M, device=matches.device)
    check(_lib.dr_match_matrix_f32(P, N, M, matches.shape[0], ptr(matches), ptr(out), stream_of(out)))
    return out


def gt_noising(matrix_gt, randn, sqrt_ac, sqrt_one_minus_ac):
    """pipeline.py:209-214 -> matrix_gt_disturbed [P,N,M] float64"""
    ensure_init()
    matrix_gt, randn = matrix_gt.contiguous().float(), randn.contiguous().float()
    P, N, M = matrix_gt.shape
    out = torch.empty(P, N, M, dtype=torch.float64, device=matrix_gt.device)
    ws = _train_ws(P, N, M, out.device)
    check(_lib.dr_gt_noising_f64(P, N, M, ptr(matrix_gt), ptr(randn), float(sqrt_ac), float(sqrt_one_minus_ac), ptr(out), ptr(ws), stream_of(out)))
    return out


def focal_loss(conf, conf_gt, weight=None, alpha=0.25, gamma=2.0, pos_w=1.0, neg_w=1.0, match_type="sinkhorn"):
    """compute_correspondence_loss (loss.py:273-314) -> 0-d float32 tensor"""
    ensure_init()
    conf, conf_gt = conf.contiguous().float(), conf_gt.contiguous().float()
    weight = weight.contiguous().float() if weight is not None else None
    P, N, M = conf.shape
    loss = torch.empty((), device=conf.device)
    ws = _train_ws(P, N, M, conf.device)
    mt = {"sinkhorn": MATCH_SINKHORN, "dual_softmax": MATCH_DUAL_SOFTMAX}[match_type]
    check(_lib.dr_focal_loss_f32(P, N, M, ptr(conf), ptr(conf_gt), ptr(weight), alpha, gamma, pos_w, neg_w, mt, ptr(loss), ptr(ws), stream_of(conf)))
    return loss


def match_recall(conf_gt, match_pred):
    """compute_match_recall (loss.py:323-345) -> (recall, precision) 0-d float32 tensors"""
    ensure_init()
    conf_gt = conf_gt.contiguous().float()
    match_pred = match_pred.to(torch.int64).contiguous()
    P, N, M = conf_gt.shape
    out = torch.empty(2, device=conf_gt.device)
    ws = _train_ws(P, N, M, conf_gt.device)
    check(_lib.dr_match_recall_f32(P, N, M, ptr(conf_gt), match_pred.shape[0], ptr(match_pred), ptr(out), ptr(ws), stream_of(conf_gt)))
    return out[0], out[1]


def motion_l1(s_pcd, R_pred, t_pred, R_gt, t_gt, overlap_mask, flow=None):
    """the L1 motion term of ge_coarse_loss (loss.py:108-128) -> 0-d float32 tensor"""
    ensure_init()
    P, N, _ = s_pcd.shape
    f = lambda x: x.contiguous().float()
    s_pcd, R_pred, t_pred, R_gt, t_gt = f(s_pcd), f(R_pred), f(t_pred.reshape(P, 3)), f(R_gt), f(t_gt.reshape(P, 3))
    flow = f(flow) if flow is not None else None
    loss = torch.empty((), device=s_pcd.device)
    ws = _train_ws(P, N, 1, s_pcd.device)
    om = mask_u8(overlap_mask)
    check(_lib.dr_motion_l1_f32(P, N, ptr(s_pcd), ptr(flow), ptr(R_pred), ptr(t_pred), ptr(R_gt), ptr(t_gt), ptr(om), ptr(loss),
                                ptr(ws), stream_of(s_pcd)))
    return loss


def motion_l1_backward(s_pcd, R_pred, t_pred, R_gt, t_gt, overlap_mask, flow=None):
    """d loss / d (R_pred, t_pred) of motion_l1 -> ([P,3,3], [P,3,1])"""
    ensure_init()
    P, N, _ = s_pcd.shape
    f = lambda x: x.contiguous().float()
    s_pcd, R_pred, t_pred, R_gt, t_gt = f(s_pcd), f(R_pred), f(t_pred.reshape(P, 3)), f(R_gt), f(t_gt.reshape(P, 3))
    flow = f(flow) if flow is not None else None
    gR, gt = torch.empty(P, 3, 3, device=s_pcd.device), torch.empty(P, 3, device=s_pcd.device)
    ws = _train_ws(P, N, 1, s_pcd.device)
    om = mask_u8(overlap_mask)
    check(_lib.dr_motion_l1_backward_f32(P, N, ptr(s_pcd), ptr(flow), ptr(R_pred), ptr(t_pred), ptr(R_gt), ptr(t_gt), ptr(om), ptr(gR), ptr(gt), ptr(ws),
                                         stream_of(s_pcd)))
    return gR, gt.view(P, 3, 1)


def _out_or_empty(out, shape, like):
    """the caller's result tensor (float32, contiguous, on the inputs' device, `shape`) or a fresh one"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    if out.dtype != torch.float32 or out.device != like.device or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("out= must be a contiguous float32 tensor of shape %s on %s" % (tuple(shape), like.device))
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    """nn.LayerNorm over the last dim -> (y, mean_rstd [rows,2]); out = (y, mean_rstd) to write into"""
    ensure_init()
    x = x.contiguous().float()
    rows, C = x.reshape(-1, x.shape[-1]).shape
    y = _out_or_empty(out[0] if out else None, x.shape, x)
    st = _out_or_empty(out[1] if out else None, (rows, 2), x)
    check(_lib.dr_layernorm_f32(rows, C, ptr(x), ptr(gamma.contiguous()), ptr(beta.contiguous()), eps, ptr(y), ptr(st), stream_of(x)))
    return y, st


def layernorm_backward(x, gamma, mean_rstd, grad_y, out=None):
    """-> (grad_x, grad_gamma, grad_beta); out = the three tensors to write into"""
    ensure_init()
    x, grad_y = x.contiguous().float(), grad_y.contiguous().float()
    rows, C = x.reshape(-1, x.shape[-1]).shape
    gx = _out_or_empty(out[0] if out else None, x.shape, x)
    gg, gb = _out_or_empty(out[1] if out else None, (C,), x), _out_or_empty(out[2] if out else None, (C,), x)
    ws = torch.empty(_lib.dr_layernorm_backward_workspace_bytes(C), dtype=torch.uint8, device=x.device)
    check(_lib.dr_layernorm_backward_f32(rows, C, ptr(x), ptr(gamma.contiguous()), ptr(mean_rstd), ptr(grad_y), ptr(gx), ptr(gg), ptr(gb), ptr(ws), stream_of(x)))
    return gx, gg, gb


def attention(q, k, v, H, q_mask=None, k_mask=None, out=None):
    """fused softmax(q k^T / sqrt(d)) v per head: q [B,L,C], k / v [B,S,C] (token layout, head h in columns h d ..) -> [B,L,C]"""
    ensure_init()
    B, L, C = q.shape
    S, d = k.shape[1], C // H
    q, k, v = q.contiguous().float(), k.contiguous().float(), v.contiguous().float()
    out = _out_or_empty(out, q.shape, q)
    check(_lib.dr_attention_f32(B, H, L, S, d, ptr(q), ptr(k), ptr(v), C, ptr(mask_u8(q_mask)), ptr(mask_u8(k_mask)), 1.0 / d ** 0.5, ptr(out), stream_of(q)))
    return out


def attention_backward(q, k, v, o, grad_o, H, q_mask=None, k_mask=None, out=None):
    """backward of attention(): -> (grad_q, grad_k, grad_v), fused (dr_attention_backward_f32); out = the three tensors to write into"""
    ensure_init()
    B, L, C = q.shape
    S, d = k.shape[1], C // H
    q, k, v, o, g = (t_.contiguous().float() for t_ in (q, k, v, o, grad_o))
    gq, gk, gv = (_out_or_empty(out[i] if out else None, t_.shape, q) for i, t_ in enumerate((q, k, v)))
    wsb = _lib.dr_attention_backward_workspace_bytes(B, H, L)
    ws = torch.empty(wsb, dtype=torch.uint8, device=q.device)
    check(_lib.dr_attention_backward_f32(B, H, L, S, d, ptr(q), ptr(k), ptr(v), ptr(o), ptr(g), C, ptr(mask_u8(q_mask)), ptr(mask_u8(k_mask)), 1.0 / d ** 0.5,
                                         ptr(gq), ptr(gk), ptr(gv), ptr(ws), wsb, stream_of(q)))
    return gq, gk, gv


def softmax_rows(scores, scale, q_mask=None, k_mask=None, out=None):
    """scores [B,H,L,S] -> softmax over S of scale * scores with the layer's key mask"""
    ensure_init()
    scores = scores.contiguous().float()
    B, H, L, S = scores.shape
    P = _out_or_empty(out, scores.shape, scores)
    qm, km = mask_u8(q_mask), mask_u8(k_mask)
    check(_lib.dr_softmax_rows_f32(B, H, L, S, ptr(scores), float(scale), ptr(qm), ptr(km), ptr(P), stream_of(scores)))
    return P


def softmax_backward(P, grad_P, scale, out=None):
    ensure_init()
    P, grad_P = P.contiguous(), grad_P.contiguous().float()
    out = _out_or_empty(out, P.shape, P)
    check(_lib.dr_softmax_backward_f32(P.numel() // P.shape[-1], P.shape[-1], ptr(P), ptr(grad_P), float(scale), ptr(out), stream_of(P)))
    return out


def relu_backward(y, grad_y, out=None):
    ensure_init()
    y, grad_y = y.contiguous(), grad_y.contiguous().float()
    out = _out_or_empty(out, y.shape, y)
    check(_lib.dr_relu_backward_f32(y.numel(), ptr(y), ptr(grad_y), ptr(out), stream_of(y)))
    return out


def rotary(x, cos_t, sin_t, inverse=False, scale=1.0, out=None):
    """embed_rotary on rows [rows, C] with half tables [rows, C/2] (inverse = its transpose)"""
    ensure_init()
    x = x.contiguous().float()
    out = _out_or_empty(out, x.shape, x)
    rows, C = x.reshape(-1, x.shape[-1]).shape
    check(_lib.dr_rotary_f32(rows, C, ptr(x), ptr(cos_t.contiguous()), ptr(sin_t.contiguous()), 1 if inverse else 0, float(scale), ptr(out), stream_of(x)))
    return out


def focal_loss_backward(conf, conf_gt, alpha=0.25, gamma=2.0, pos_w=1.0, neg_w=1.0, out=None):
    """d loss / d conf of the sinkhorn-form focal loss (loss.py:311-314) -> [P,N,M] float32"""
    ensure_init()
    conf, conf_gt = conf.contiguous().float(), conf_gt.contiguous().float()
    P, N, M = conf.shape
    g = _out_or_empty(out, conf.shape, conf)
    ws = _train_ws(P, N, M, conf.device)
    check(_lib.dr_focal_loss_backward_f32(P, N, M, ptr(conf), ptr(conf_gt), alpha, gamma, pos_w, neg_w, ptr(g), ptr(ws), stream_of(conf)))
    return g


def sinkhorn_backward(scores, bin_score, iters, src_mask, tgt_mask, grad_conf, out=None):
    """backward of conf = exp(log_optimal_transport(scores, bin_score, iters, masks))[:, :-1, :-1] -> (grad_scores [P,N,M], grad_bin_score 0-d);
    out = (grad_scores [P,N,M], grad_bin_score per pair [P]) to write into"""
    ensure_init()
    scores, grad_conf = scores.contiguous().float(), grad_conf.contiguous().float()
    P, N, M = scores.shape
    gs = _out_or_empty(out[0] if out else None, scores.shape, scores)
    ga = _out_or_empty(out[1] if out else None, (P,), scores)
    wsb = _lib.dr_sinkhorn_backward_workspace_bytes(P, N, M, int(iters))
    ws = torch.empty(wsb, dtype=torch.uint8, device=scores.device)
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    bs = torch.as_tensor(bin_score).detach().reshape(1).float().to(scores.device).contiguous()
    check(_lib.dr_sinkhorn_backward_f32(P, N, M, ptr(scores), ptr(sm), ptr(tm), ptr(bs), int(iters), ptr(grad_conf), ptr(gs), ptr(ga), ptr(ws), wsb,
                                        stream_of(scores)))
    return gs, ga.sum()


def mutual_match(conf, thr=0.0, mutual=True, cap=None, want_mask=False):
    """Matching.get_match on device: conf [P,N,M] float32 / float64 -> (matches [P,cap,3] int64, mconf [P,cap], count [P] int32,
    mask [P,N,M] uint8 or None); rows beyond count[p] are undefined, count > cap means the list was truncated."""
    ensure_init()
    conf = conf.contiguous()
    P, N, M = conf.shape
    cap = cap or (N + M)
    dev = conf.device
    matches = torch.zeros(P, cap, 3, dtype=torch.int64, device=dev)
    mconf = torch.zeros(P, cap, dtype=conf.dtype, device=dev)
    count = torch.zeros(P, dtype=torch.int32, device=dev)
    mask = torch.zeros(P, N, M, dtype=torch.uint8, device=dev) if want_mask else None
    fn = _lib.dr_mutual_match_f64 if conf.dtype == torch.float64 else _lib.dr_mutual_match_f32
    check(fn(P, N, M, ptr(conf), float(thr), 1 if mutual else 0, cap, ptr(matches), ptr(mconf), ptr(count), ptr(mask), stream_of(conf)))
    return matches, mconf, count, mask


def sinkhorn_f16(scores, bin_score, iters, src_mask=None, tgt_mask=None, *, minshift=False, apply_mask=False, ragged=False):
    """dr_sinkhorn_f16 (opt-in): [B,N,M] float16 scores -> float16 conf; tiles up to 256 x 256"""
    ensure_init()
    assert scores.dim() == 3 and scores.dtype == torch.float16
    scores = scores.contiguous()
    B, N, M = scores.shape
    flags = (SK_MINSHIFT if minshift else 0) | (SK_APPLY_MASK if apply_mask else 0) | (SK_RAGGED if ragged else 0)
    out = torch.empty(B, N, M, dtype=torch.float16, device=scores.device)
    bs = bin_score.detach().to(device=scores.device, dtype=torch.float32).reshape(1).contiguous()
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    check(_lib.dr_sinkhorn_f16(B, N, M, ptr(scores), ptr(sm), ptr(tm), ptr(bs), int(iters), flags, ptr(out), stream_of(scores)))
    return out


def sinkhorn(scores, bin_score, iters, src_mask=None, tgt_mask=None, *, minshift=False, apply_mask=False,
             log_output=False, out_f32=False, strict=False, ragged=False, out=None):
    """Batched Sinkhorn with dustbins on [B,N,M] fp32/fp64 scores.

    Returns conf [B,N,M] (= exp(log_optimal_transport(...))[:, :-1, :-1]) or, with log_output, the full
    [B,N+1,M+1] log assignment (3D/models/matching.py:61-93)."""
    assert scores.dim() == 3
    scores = scores.contiguous()
    B, N, M = scores.shape
    f64 = scores.dtype == torch.float64
    if not f64 and scores.dtype != torch.float32:
        raise RuntimeError("sinkhorn: fp32 or fp64 scores only")
    flags = (SK_OUT_LOG if log_output else 0) | (SK_MINSHIFT if minshift else 0) | \
            (SK_APPLY_MASK if apply_mask else 0) | (SK_OUT_F32 if (f64 and out_f32) else 0) | (SK_STRICT if strict else 0) | \
            (SK_RAGGED if ragged else 0)
    odt = torch.float32 if (not f64 or out_f32) else torch.float64
    shape = (B, N + 1, M + 1) if log_output else (B, N, M)
    if out is None:
        out = torch.empty(shape, dtype=odt, device=scores.device)
    else:
        assert out.shape == shape and out.dtype == odt and out.is_contiguous()
    bs = bin_score.detach().to(device=scores.device, dtype=torch.float32).reshape(1).contiguous()
    wsb = _lib.dr_sinkhorn_workspace_bytes(B, N, M, 8 if f64 else 4, flags)
    ws = torch.empty(wsb, dtype=torch.uint8, device=scores.device) if wsb else None
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    fn = _lib.dr_sinkhorn_f64 if f64 else _lib.dr_sinkhorn_f32
    check(fn(B, N, M, ptr(scores), ptr(sm), ptr(tm), ptr(bs), int(iters), flags, ptr(out), ptr(ws), wsb,
             stream_of(scores)))
    return out


# ------------------------------------------------------------------------------------------------
# thin wrappers of the remaining ops (all tensors on the ROCm device, float32 unless noted)
# ------------------------------------------------------------------------------------------------
def pe_freq(C, device):
    """div_term of VolumetricPositionEncoding.forward (position_encoding.py:58), computed by torch so
    that the table is the reference's own."""
    import math
    d = C // 3
    # evaluated on the host like the oracle/reference CPU run, then moved (a device exp may differ by an ulp)
    return torch.exp(torch.arange(0, d, 2, dtype=torch.float) * (-math.log(10000.0) / d)).to(device).contiguous()


def vol_pe(xyz, C, origin, voxel, R=None, t=None, rows_per_pair=None):
    """xyz [rows,3] -> (cos, sin) tables [rows, C/2] of the (optionally warped) points."""
    ensure_init()
    xyz = xyz.contiguous().float()
    rows = xyz.shape[0]
    cos = torch.empty(rows, C // 2, device=xyz.device)
    sin = torch.empty_like(cos)
    fr = pe_freq(C, xyz.device)
    if R is not None:
        R = R.contiguous().float()
        t = t.contiguous().float()
    check(_lib.dr_vol_pe_f32(rows, rows_per_pair or max(rows, 1), C, ptr(xyz), ptr(R), ptr(t), float(origin[0]),
                             float(origin[1]), float(origin[2]), float(voxel), ptr(fr), ptr(cos), ptr(sin), stream_of(xyz)))
    return cos, sin


def linear(x, W, epilogue=0, cos=None, sin=None, rot_C=0, scale=1.0):
    ensure_init()
    x = x.contiguous()
    W = W.contiguous()
    out = torch.empty(x.shape[0], W.shape[0], device=x.device)
    check(_lib.dr_linear_f32(x.shape[0], W.shape[0], x.shape[1], ptr(x), ptr(W), ptr(out), epilogue, ptr(cos), ptr(sin),
                             rot_C, float(scale), stream_of(x)))
    return out


def bmm_nt(a, b, scale=1.0):
    """a [..., R, K] @ b[..., N, K]^T over the leading (batch) dims, one launch (dr_gemm_nt_batched_f32; K is zero-padded to a multiple of 4)"""
    ensure_init()
    lead = a.shape[:-2]
    R, K = a.shape[-2:]
    N = b.shape[-2]
    a, b = a.reshape(-1, R, K).contiguous().float(), b.reshape(-1, N, K).contiguous().float()
    pad = (-K) % 4
    if pad:
        a, b = torch.nn.functional.pad(a, (0, pad)), torch.nn.functional.pad(b, (0, pad))
    nb = a.shape[0]
    out = torch.empty(nb, R, N, device=a.device)
    check(_lib.dr_gemm_nt_batched_f32(nb, R, N, K + pad, ptr(a), R * (K + pad), ptr(b), N * (K + pad), ptr(out), R * N, float(scale), stream_of(a)))
    return out.view(*lead, R, N)


def linear_ex(x, W, bias=None, epilogue=0, scale=1.0, K=None):
    """x [rows, lda >= K] @ W[ncols, K]^T (+ bias) -> [rows, ncols]"""
    ensure_init()
    K = W.shape[1] if K is None else K
    out = torch.empty(x.shape[0], W.shape[0], device=x.device)
    check(_lib.dr_linear_ex_f32(x.shape[0], W.shape[0], K, ptr(x), x.stride(0), ptr(W), ptr(bias), ptr(out), out.stride(0), epilogue,
                                float(scale), stream_of(x)))
    return out


def gemm_problem(A, W, out, rows, ncols, K, lda, ldo, A2=None, K1=0, lda2=0, bias=None, addend=None, epilogue=0, cos=None, sin=None,
                 rot_C=0, scale=1.0, nbatch=0, stride_a=0, stride_w=0, stride_o=0):
    """-> DebugGemmProblem for debug_gemm.  Tensors are passed by their data pointer, so views with an offset (a column offset of `out`, a
    row window of A) address exactly what they show; the caller keeps every tensor alive and sizes it for rows / lda / ldo / strides."""
    def dp(t):
        if t is None:
            return None
        if not t.is_cuda:
            raise RuntimeError("libdiffreg_hip ops need tensors on a ROCm device (got %s); there is no CPU path" % t.device)
        return t.data_ptr()
    return DebugGemmProblem(dp(A), dp(A2), dp(W), dp(out), dp(cos), dp(sin), dp(bias), dp(addend), rows, ncols, K, K1, lda, lda2, ldo,
                            epilogue, rot_C, float(scale), nbatch, stride_a, stride_w, stride_o)


def debug_gemm(problems, stream_tensor, checked=True):
    """one grouped launch of 1..4 problems (gemm_problem) through dr_debug_gemm_f32 on the current stream of stream_tensor's device;
    checked=False returns the status code instead of raising"""
    ensure_init()
    arr = (DebugGemmProblem * len(problems))(*problems)
    rc = _lib.dr_debug_gemm_f32(arr, len(problems), stream_of(stream_tensor))
    if checked:
        check(rc)
    return rc


KP_INFLUENCE = {"constant": 0, "linear": 1, "gaussian": 2}


def kpconv_gather(q_pts, s_pts, neighb_inds, x, kernel_points, extent, influence="linear", aggregation="sum"):
    """-> weighted features [Nq, ceil4(K*Cin)] (see dr_kpconv_gather_mode_f32; KP_influence / aggregation_mode of blocks.py:304-326)"""
    ensure_init()
    Nq, H = neighb_inds.shape
    K, Cin = kernel_points.shape[0], x.shape[1]
    ld = (K * Cin + 3) // 4 * 4
    out = torch.empty(Nq, ld, device=x.device)
    check(_lib.dr_kpconv_gather_mode_f32(Nq, s_pts.shape[0], H, Cin, K, ptr(q_pts.contiguous()), ptr(s_pts.contiguous()),
                                         ptr(neighb_inds.contiguous()), ptr(x.contiguous()), ptr(kernel_points.contiguous()), float(extent),
                                         KP_INFLUENCE[influence], {"sum": 0, "closest": 1}[aggregation], ptr(out), ld, stream_of(x)))
    return out


def col_stats(x):
    """per-column mean and 1/sqrt(var + 1e-5) over the rows of x [N, C] (InstanceNorm1d of BatchNormBlock)"""
    ensure_init()
    N, C = x.shape
    mean, rstd = torch.empty(C, device=x.device), torch.empty(C, device=x.device)
    wsb = _lib.dr_col_stats_workspace_bytes(N, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    check(_lib.dr_col_stats_f32(N, C, ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(ws), wsb, stream_of(x)))
    return mean, rstd


def norm_apply(a, stats_a, b=None, stats_b=None, slope=0.1, activate=True):
    """act( norm(a) + [norm(b) | b | 0] )"""
    ensure_init()
    N, C = a.shape
    out = torch.empty(N, C, device=a.device)
    mb, rb = stats_b if stats_b is not None else (None, None)
    check(_lib.dr_norm_apply_f32(N, C, ptr(a), a.stride(0), ptr(stats_a[0]), ptr(stats_a[1]), ptr(b), b.stride(0) if b is not None else 0,
                                 ptr(mb), ptr(rb), float(slope), 1 if activate else 0, ptr(out), C, stream_of(a)))
    return out


def gather_pool(x, inds, first_only=False):
    """max_pool / closest_pool over index lists [n2, H] (int64; indices >= len(x) read a zero row)"""
    ensure_init()
    n2, H = inds.shape
    out = torch.empty(n2, x.shape[1], device=x.device)
    inds = inds.contiguous()
    check(_lib.dr_gather_pool_f32(n2, H, H, x.shape[1], ptr(x.contiguous()), x.shape[0], ptr(inds), 1 if first_only else 0, ptr(out),
                                  stream_of(x)))
    return out


def kpconv_gather_backward(q_pts, s_pts, neighb_inds, x, kernel_points, extent, grad_weighted, influence="linear", aggregation="sum"):
    """d loss / d x [Ns, Cin] of kpconv_gather (grad_weighted [Nq, ceil4(K*Cin)])"""
    ensure_init()
    Nq, H = neighb_inds.shape
    K, Cin = kernel_points.shape[0], x.shape[1]
    gw = grad_weighted.contiguous()
    gx = torch.empty_like(x)
    check(_lib.dr_kpconv_gather_backward_mode_f32(Nq, s_pts.shape[0], H, Cin, K, ptr(q_pts.contiguous()), ptr(s_pts.contiguous()),
                                                  ptr(neighb_inds.contiguous()), ptr(x.contiguous()), ptr(kernel_points.contiguous()), float(extent),
                                                  KP_INFLUENCE[influence], {"sum": 0, "closest": 1}[aggregation], ptr(gw), gw.shape[1], ptr(gx),
                                                  stream_of(x)))
    return gx


def norm_backward(grad_out, out, a, stats_a, b=None, stats_b=None, slope=0.1, activate=True):
    """backward of norm_apply -> (grad_a, grad_b or None)"""
    ensure_init()
    N, C = a.shape
    g = grad_out.contiguous()
    ga = torch.empty(N, C, device=a.device)
    gb = torch.empty(N, C, device=a.device) if b is not None else None
    mb, rb = stats_b if stats_b is not None else (None, None)
    wsb = _lib.dr_norm_backward_workspace_bytes(N, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=a.device)
    check(_lib.dr_norm_backward_f32(N, C, ptr(g), C, ptr(out), out.stride(0) if out is not None else 0, ptr(a), a.stride(0), ptr(stats_a[0]), ptr(stats_a[1]),
                                    ptr(b), b.stride(0) if b is not None else 0, ptr(mb), ptr(rb), float(slope), 1 if activate else 0, ptr(ga), C,
                                    ptr(gb), C, ptr(ws), wsb, stream_of(a)))
    return ga, gb


def gather_pool_backward(x, inds, grad_out, first_only=False):
    """backward of gather_pool -> grad_x (shape of x)"""
    ensure_init()
    n2, H = inds.shape
    gx = torch.empty_like(x)
    check(_lib.dr_gather_pool_backward_f32(n2, H, H, x.shape[1], ptr(x.contiguous()), x.shape[0], ptr(inds.contiguous()), 1 if first_only else 0,
                                           ptr(grad_out.contiguous()), ptr(gx), stream_of(x)))
    return gx


def _at_col(t, col):
    """device pointer of column `col` of a contiguous row-major [rows, width] tensor (a column slice addressed through its leading dimension)"""
    if not t.is_cuda or not t.is_contiguous():
        raise RuntimeError("libdiffreg_hip ops need contiguous ROCm tensors")
    return c_void_p(t.data_ptr() + col * t.element_size())


def group_norm_stats(x, G, eps=1e-5):
    """(mean, rstd) [G] of nn.GroupNorm(G, C) over the rows of x [N, C] (dr_group_norm_stats_f32)"""
    ensure_init()
    N, C = x.shape
    mean, rstd = torch.empty(G, device=x.device), torch.empty(G, device=x.device)
    wsb = _lib.dr_group_norm_workspace_bytes(N, C)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=x.device)
    check(_lib.dr_group_norm_stats_f32(N, C, G, ptr(x), x.stride(0), float(eps), ptr(mean), ptr(rstd), ptr(ws), wsb, stream_of(x)))
    return mean, rstd


def group_norm_apply(a, stats_a, gamma_a, beta_a, b=None, stats_b=None, gamma_b=None, beta_b=None, slope=None):
    """act( GN(a) + [GN(b) | b | 0] ), act = LeakyReLU(slope) or none when slope is None (dr_group_norm_apply_f32)"""
    ensure_init()
    N, C = a.shape
    G = stats_a[0].shape[0]
    out = torch.empty(N, C, device=a.device)
    mb, rb = stats_b if stats_b is not None else (None, None)
    check(_lib.dr_group_norm_apply_f32(N, C, G, ptr(a), a.stride(0), ptr(stats_a[0]), ptr(stats_a[1]), ptr(gamma_a), ptr(beta_a), ptr(b),
                                       b.stride(0) if b is not None else 0, ptr(mb), ptr(rb), ptr(gamma_b if mb is not None else None),
                                       ptr(beta_b if mb is not None else None), float(slope or 0.0), 0 if slope is None else 1, ptr(out), C,
                                       stream_of(a)))
    return out


def group_norm_backward(grad_out, out, a, stats_a, gamma_a, b=None, stats_b=None, gamma_b=None, slope=None):
    """backward of group_norm_apply -> (grad_a, grad_b or None, d gamma_a, d beta_a, d gamma_b or None, d beta_b or None)"""
    ensure_init()
    N, C = a.shape
    G = stats_a[0].shape[0]
    g = grad_out.contiguous()
    dev = a.device
    ga = torch.empty(N, C, device=dev)
    gb = torch.empty(N, C, device=dev) if b is not None else None
    dga, dba = torch.empty(C, device=dev), torch.empty(C, device=dev)
    mb, rb = stats_b if stats_b is not None else (None, None)
    dgb, dbb = (torch.empty(C, device=dev), torch.empty(C, device=dev)) if mb is not None else (None, None)
    wsb = _lib.dr_group_norm_backward_workspace_bytes(N, C, G)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    check(_lib.dr_group_norm_backward_f32(N, C, G, ptr(g), C, ptr(out), out.stride(0), ptr(a), a.stride(0), ptr(stats_a[0]), ptr(stats_a[1]), ptr(gamma_a),
                                          ptr(b), b.stride(0) if b is not None else 0, ptr(mb), ptr(rb), ptr(gamma_b if mb is not None else None),
                                          float(slope or 0.0), 0 if slope is None else 1, ptr(ga), C, ptr(dga), ptr(dba), ptr(gb), C, ptr(dgb), ptr(dbb),
                                          ptr(ws), wsb, stream_of(a)))
    return ga, gb, dga, dba, dgb, dbb


def knn_interpolate(q_pts, s_pts, neighb_inds, x, out=None, col=0):
    """knn_interpolate_pack_mode(q, s, x, inds) -> [Nq, C], or written into columns col .. col + C - 1 of `out` [Nq, width] (returned)"""
    ensure_init()
    Nq, H = neighb_inds.shape
    C = x.shape[1]
    if out is None:
        out, col = torch.empty(Nq, C, device=x.device), 0
    check(_lib.dr_knn_interpolate_f32(Nq, s_pts.shape[0], H, C, ptr(q_pts.contiguous()), ptr(s_pts.contiguous()), ptr(neighb_inds.contiguous()),
                                      ptr(x.contiguous()), _at_col(out, col), out.shape[1], stream_of(x)))
    return out


def knn_interpolate_backward(q_pts, s_pts, neighb_inds, grad_out, C, col=0):
    """d loss / d x [Ns, C] of knn_interpolate from columns col .. col + C - 1 of grad_out [Nq, width]"""
    ensure_init()
    Nq, H = neighb_inds.shape
    g = grad_out.contiguous()
    gx = torch.empty(s_pts.shape[0], C, device=g.device)
    check(_lib.dr_knn_interpolate_backward_f32(Nq, s_pts.shape[0], H, C, ptr(q_pts.contiguous()), ptr(s_pts.contiguous()), ptr(neighb_inds.contiguous()),
                                               _at_col(g, col), g.shape[1], ptr(gx), stream_of(g)))
    return gx


def kpconv_neighbor_count(neighb_inds, x, Ns):
    """int32 [Nq]: KPConv's neighbours with a positive feature sum, as dr_kpconv_gather_f32 counts them"""
    ensure_init()
    Nq, H = neighb_inds.shape
    counts = torch.empty(Nq, dtype=torch.int32, device=x.device)
    check(_lib.dr_kpconv_neighbor_count_f32(Nq, Ns, H, x.shape[1], ptr(neighb_inds.contiguous()), ptr(x.contiguous()), ptr(counts), stream_of(x)))
    return counts


_LAYER_KEYS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight", "mlp.2.weight",
               "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")


def layer_weights(tensors):
    """tensors: the 10 tensors of one GeometryAttentionLayer in _LAYER_KEYS order (kept alive by the caller)."""
    lw = LayerWeights()
    for (name, _), tns in zip(LayerWeights._fields_, tensors):
        assert tns.is_cuda and tns.is_contiguous() and tns.dtype == torch.float32
        setattr(lw, name, tns.data_ptr())
    return lw


def attention_layer(tensors, C, H, x, y, cos_x=None, sin_x=None, cos_y=None, sin_y=None, x_mask=None, y_mask=None, xq=None, yk=None):
    """x [P,Lx,C] attends y [P,Ly,C] (GeometryAttentionLayer.forward).  Rotary tables given: pe_type 'rotary'.  No tables: no position code inside
    the layer (entangled form), or -- with xq = x + pe_x, yk = y + pe_y -- pe_type 'sinusoidal' (transformero.py:50-57)."""
    ensure_init()
    P, Lx, _ = x.shape
    Ly = y.shape[1]
    lw = layer_weights(tensors)
    out = torch.empty_like(x)
    wsb = _lib.dr_attention_layer_workspace_bytes(P, Lx, Ly, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    xm, ym = mask_u8(x_mask), mask_u8(y_mask)
    cont = lambda a: None if a is None else a.contiguous().float()
    x, y, xq, yk, cos_x, sin_x, cos_y, sin_y = (cont(a) for a in (x, y, xq, yk, cos_x, sin_x, cos_y, sin_y))
    check(_lib.dr_attention_layer_pe_f32(ctypes.byref(lw), C, H, P, Lx, Ly, ptr(x), ptr(y), ptr(xq), ptr(yk), ptr(cos_x), ptr(sin_x), ptr(cos_y),
                                         ptr(sin_y), ptr(xm), ptr(ym), ptr(out), ptr(ws), wsb, stream_of(x)))
    return out


def attention_layer_train_forward(tensors, C, H, x, y, cos_x, sin_x, cos_y, sin_y, x_mask=None, y_mask=None):
    """GeometryAttentionLayer.forward keeping what the backward needs: x [B,L,C], y [B,S,C] -> (out [B,L,C], saved: an opaque uint8 tensor)"""
    ensure_init()
    B, L, _ = x.shape
    S = y.shape[1]
    lw = layer_weights(tensors)
    out = torch.empty(B, L, C, device=x.device)
    nb = _lib.dr_attention_layer_train_saved_bytes(B, L, S, C)
    saved = torch.empty(nb, dtype=torch.uint8, device=x.device)
    xm, ym = mask_u8(x_mask), mask_u8(y_mask)
    check(_lib.dr_attention_layer_train_forward_f32(ctypes.byref(lw), C, H, B, L, S, ptr(x), ptr(y), ptr(cos_x), ptr(sin_x), ptr(cos_y), ptr(sin_y),
                                                    ptr(xm), ptr(ym), ptr(out), ptr(saved), nb, stream_of(x)))
    return out, saved


def attention_layer_backward(tensors, C, H, x, y, cos_x, sin_x, cos_y, sin_y, x_mask, y_mask, saved, grad_out):
    """-> grad_x [B,L,C], grad_y [B,S,C], the ten parameter gradients in the order of lib._LAYER_KEYS"""
    ensure_init()
    B, L, _ = x.shape
    S = y.shape[1]
    lw = layer_weights(tensors)
    grads = [torch.empty_like(t_) for t_ in tensors]
    gw = layer_weights(grads)
    gx, gy = torch.empty(B, L, C, device=x.device), torch.empty(B, S, C, device=x.device)
    wsb = _lib.dr_attention_layer_backward_workspace_bytes(B, H, L, S, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    xm, ym = mask_u8(x_mask), mask_u8(y_mask)
    check(_lib.dr_attention_layer_backward_f32(ctypes.byref(lw), C, H, B, L, S, ptr(x), ptr(y), ptr(cos_x), ptr(sin_x), ptr(cos_y), ptr(sin_y),
                                               ptr(xm), ptr(ym), ptr(saved), ptr(grad_out), ptr(gx), ptr(gy), ctypes.byref(gw), ptr(ws), wsb,
                                               stream_of(x)))
    return gx, gy, grads


# vision3d TransformerLayer parameters (vision3d/layers/transformer.py:58-301) in the order of dr_fusion_layer_weights' fields
FUSION_LAYER_KEYS = ("attention.attention.q_token_layer.weight", "attention.attention.q_token_layer.bias",
                     "attention.attention.k_token_layer.weight", "attention.attention.k_token_layer.bias",
                     "attention.attention.v_token_layer.weight", "attention.attention.v_token_layer.bias",
                     "attention.linear.weight", "attention.linear.bias", "attention.norm.weight", "attention.norm.bias",
                     "output.expand.weight", "output.expand.bias", "output.squeeze.weight", "output.squeeze.bias",
                     "output.norm.weight", "output.norm.bias")


def fusion_layer_weights(tensors):
    """tensors: the 16 tensors of one vision3d TransformerLayer in FUSION_LAYER_KEYS order (kept alive by the caller)."""
    lw = FusionLayerWeights()
    for (name, _), tns in zip(FusionLayerWeights._fields_, tensors):
        assert tns.is_cuda and tns.is_contiguous() and tns.dtype == torch.float32
        setattr(lw, name, tns.data_ptr())
    return lw


def fusion_layer_train_forward(tensors, C, H, x, y, y_mask=None):
    """TransformerLayer.forward(x, y, y) keeping what the backward needs: x [B,L,C], y [B,S,C] float32 contiguous, y_mask [B,S] (True = a valid
    key) or None -> (out [B,L,C], saved: an opaque uint8 tensor)"""
    ensure_init()
    B, L, _ = x.shape
    S = y.shape[1]
    lw = fusion_layer_weights(tensors)
    out = torch.empty(B, L, C, device=x.device)
    nb = _lib.dr_fusion_layer_train_saved_bytes(B, L, S, C)
    saved = torch.empty(nb, dtype=torch.uint8, device=x.device)
    check(_lib.dr_fusion_layer_train_forward_f32(ctypes.byref(lw), C, H, B, L, S, ptr(x), ptr(y), ptr(mask_u8(y_mask)), ptr(out), ptr(saved), nb,
                                                 stream_of(x)))
    return out, saved


def fusion_layer_backward(tensors, C, H, x, y, y_mask, saved, grad_out):
    """-> grad_x [B,L,C], grad_y [B,S,C], the 16 parameter gradients in FUSION_LAYER_KEYS order"""
    ensure_init()
    B, L, _ = x.shape
    S = y.shape[1]
    lw = fusion_layer_weights(tensors)
    grads = [torch.empty_like(t_) for t_ in tensors]
    gw = fusion_layer_weights(grads)
    gx, gy = torch.empty(B, L, C, device=x.device), torch.empty(B, S, C, device=x.device)
    wsb = _lib.dr_fusion_layer_backward_workspace_bytes(B, H, L, S, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    check(_lib.dr_fusion_layer_backward_f32(ctypes.byref(lw), C, H, B, L, S, ptr(x), ptr(y), ptr(mask_u8(y_mask)), ptr(saved), ptr(grad_out.contiguous()),
                                            ptr(gx), ptr(gy), ctypes.byref(gw), ptr(ws), wsb, stream_of(x)))
    return gx, gy, grads


def l2_normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=1, eps) of rows x [R,C] -> (y, norms [R])"""
    ensure_init()
    x = x.contiguous().float()
    y = torch.empty_like(x)
    n = torch.empty(x.shape[0], device=x.device)
    check(_lib.dr_l2_normalize_f32(x.shape[0], x.shape[1], ptr(x), float(eps), ptr(y), ptr(n), stream_of(x)))
    return y, n


def l2_normalize_backward(y, norms, grad_y, eps=1e-12):
    ensure_init()
    gx = torch.empty_like(y)
    check(_lib.dr_l2_normalize_backward_f32(y.shape[0], y.shape[1], ptr(y), ptr(norms), float(eps), ptr(grad_y.contiguous().float()), ptr(gx),
                                            stream_of(y)))
    return gx


def circle_params(pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_overlap, neg_overlap):
    return CircleLossParams(float(pos_margin), float(neg_margin), float(pos_optimal), float(neg_optimal), float(log_scale), float(pos_overlap),
                            float(neg_overlap))


def _circle_inputs(img, pcd, img_idx, pcd_idx, min_ov, max_ov):
    f = lambda t_: t_.detach().contiguous().float()
    i = lambda t_: t_.detach().contiguous().to(torch.int64)
    return f(img), f(pcd), i(img_idx), i(pcd_idx), f(min_ov), f(max_ov)


def circle_loss(img, pcd, img_idx, pcd_idx, min_ov, max_ov, params):
    """weighted circle loss of feat_dists(img [M,C], pcd [N,C]) (dr_circle_loss_f32) -> 0-dim device tensor"""
    ensure_init()
    img, pcd, ii, jj, mn, mx = _circle_inputs(img, pcd, img_idx, pcd_idx, min_ov, max_ov)
    (M, C), N = img.shape, pcd.shape[0]
    loss = torch.empty((), device=img.device)
    wsb = _lib.dr_circle_loss_workspace_bytes(M, N, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=img.device)
    check(_lib.dr_circle_loss_f32(M, N, C, ptr(img), ptr(pcd), ii.numel(), ptr(ii), ptr(jj), ptr(mn), ptr(mx), ctypes.byref(params), ptr(loss), ptr(ws),
                                  wsb, stream_of(img)))
    return loss


def circle_loss_backward(img, pcd, img_idx, pcd_idx, min_ov, max_ov, params, grad_loss=None):
    """-> (loss, d loss / d img [M,C], d loss / d pcd [N,C]) scaled by grad_loss (0-dim device tensor or None = 1)"""
    ensure_init()
    img, pcd, ii, jj, mn, mx = _circle_inputs(img, pcd, img_idx, pcd_idx, min_ov, max_ov)
    (M, C), N = img.shape, pcd.shape[0]
    loss = torch.empty((), device=img.device)
    gi, gp = torch.empty_like(img), torch.empty_like(pcd)
    gl = None if grad_loss is None else grad_loss.detach().reshape(()).float().contiguous()
    wsb = _lib.dr_circle_loss_workspace_bytes(M, N, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=img.device)
    check(_lib.dr_circle_loss_backward_f32(M, N, C, ptr(img), ptr(pcd), ii.numel(), ptr(ii), ptr(jj), ptr(mn), ptr(mx), ctypes.byref(params), ptr(gl),
                                           ptr(loss), ptr(gi), ptr(gp), ptr(ws), wsb, stream_of(img)))
    return loss, gi, gp


def fine_params(pos_radius_3d, neg_radius_3d, pos_radius_2d, neg_radius_2d, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale):
    return FineLossParams(*(float(v) for v in (pos_radius_3d, neg_radius_3d, pos_radius_2d, neg_radius_2d, pos_margin, neg_margin, pos_optimal,
                                               neg_optimal, log_scale)))


def _fine_inputs(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices):
    f = lambda t_: t_.detach().contiguous().float()
    i = lambda t_: t_.detach().contiguous().to(torch.int64)
    ip, fi, pp, px, fp, T = f(img_points), f(img_feats), f(pcd_points), f(pcd_pixels), f(pcd_feats), f(transform)
    sp, si = i(img_sel_pixels), i(pcd_sel_indices)
    (HW, C), N, M = fi.shape, fp.shape[0], si.shape[0]
    if ip.shape != (HW, 3) or pp.shape != (N, 3) or px.shape != (N, 2) or fp.shape != (N, C) or T.shape != (4, 4) or sp.shape != (M, 2):
        raise RuntimeError("fine_loss: shapes img_points %s img_feats %s pcd_points %s pcd_pixels %s pcd_feats %s transform %s img_sel_pixels %s "
                           "pcd_sel_indices %s" % tuple(tuple(t_.shape) for t_ in (ip, fi, pp, px, fp, T, sp, si)))
    return (ip, fi, pp, px, fp, T, sp, si), (HW, N, M, C)


def fine_loss(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params):
    """FineMatchingLoss.forward behind its random_choice (dr_fine_loss_f32): img_points [HW,3], img_feats [HW,C], pcd_points [N,3], pcd_pixels
    [N,2], pcd_feats [N,C], transform [4,4], img_sel_pixels [M,2] (v, u), pcd_sel_indices [M] -> (loss, recall, saved): two 0-dim views of one
    device tensor, and the opaque statistics fine_loss_backward wants.  M <= 1024, C <= 256 (raises beyond)."""
    ensure_init()
    ts, (HW, N, M, C) = _fine_inputs(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices)
    dev = ts[1].device
    out = torch.empty(2, device=dev)
    nb = _lib.dr_fine_loss_saved_bytes(M)
    saved = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    check(_lib.dr_fine_loss_f32(HW, N, M, C, *(ptr(t_) for t_ in ts), int(image_w), ctypes.byref(params), ptr(out), ptr(saved), nb, stream_of(ts[1])))
    return out[0], out[1], saved


def fine_loss_backward(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices, image_w, params, saved,
                       grad_loss=None):
    """-> (d loss / d img_feats [HW,C], d loss / d pcd_feats [N,C]), dense, scaled by grad_loss (0-dim device tensor or None = 1)"""
    ensure_init()
    ts, (HW, N, M, C) = _fine_inputs(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, img_sel_pixels, pcd_sel_indices)
    dev = ts[1].device
    gi, gp = torch.empty(HW, C, device=dev), torch.empty(N, C, device=dev)
    gl = None if grad_loss is None else grad_loss.detach().reshape(()).float().contiguous()
    wsb = _lib.dr_fine_loss_backward_workspace_bytes(M, C)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
    check(_lib.dr_fine_loss_backward_f32(HW, N, M, C, *(ptr(t_) for t_ in ts), int(image_w), ctypes.byref(params), ptr(saved), saved.numel(), ptr(gl),
                                         ptr(gi), ptr(gp), ptr(ws), wsb, stream_of(ts[1])))
    return gi, gp


def dual_softmax(sim, temperature, src_mask=None, tgt_mask=None, out=None):
    """sim [P,N,M] float32 -> conf = softmax_dim1(sim / T | source rows) * softmax_dim2(sim / T | target columns) (matching.py:193-205)"""
    ensure_init()
    sim = sim.contiguous().float()
    P, N, M = sim.shape
    conf = _out_or_empty(out, sim.shape, sim)
    stats = torch.empty(2 * P * M, dtype=torch.float32, device=sim.device)
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    check(_lib.dr_dual_softmax_f32(P, N, M, ptr(sim), float(temperature), ptr(sm), ptr(tm), ptr(conf), ptr(stats), stream_of(sim)))
    return conf


def dual_softmax_backward(sim, temperature, src_mask, tgt_mask, grad_conf, out=None):
    """d loss / d sim of conf = dual_softmax(sim, temperature, masks) given d loss / d conf (dr_dual_softmax_backward_f32)"""
    ensure_init()
    sim, grad_conf = sim.contiguous().float(), grad_conf.contiguous().float()
    P, N, M = sim.shape
    gs = _out_or_empty(out, sim.shape, sim)
    nb = _lib.dr_dual_softmax_backward_workspace_bytes(P, N, M)
    ws = torch.empty(nb, dtype=torch.uint8, device=sim.device)
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    check(_lib.dr_dual_softmax_backward_f32(P, N, M, ptr(sim), float(temperature), ptr(sm), ptr(tm), ptr(grad_conf), ptr(gs), ptr(ws), nb, stream_of(sim)))
    return gs


def procrustes(conf, src_pcd, tgt_pcd, src_mask, tgt_mask, sample_rate, max_condition_num, use_mask_len=False,
               want_topk=False):
    """SoftProcrustesLayer.forward on device.  conf [P,N,M] float32 -> R,t,R_forwd,t_forwd,cond(f64),ok(bool)[,idx]."""
    ensure_init()
    if conf.dtype != torch.float32:
        raise RuntimeError("procrustes: float32 conf expected (the reference raises on float64, quirk Q3)")
    conf = conf.contiguous()
    P, N, M = conf.shape
    dev = conf.device
    R = torch.empty(P, 3, 3, device=dev); t = torch.empty(P, 3, 1, device=dev)
    Rf = torch.empty(P, 3, 3, device=dev); tf = torch.empty(P, 3, 1, device=dev)
    cond = torch.empty(P, dtype=torch.float64, device=dev)
    ok = torch.empty(P, dtype=torch.int32, device=dev)
    K = int(float(torch.tensor(float(max(N, M)), dtype=torch.float32) * sample_rate))
    idx = torch.zeros(P, K, dtype=torch.int32, device=dev) if want_topk else None     # (a pair's own K may be smaller -- 4D: the tail stays 0)
    sm, tm = mask_u8(src_mask), mask_u8(tgt_mask)
    wsb = _lib.dr_procrustes_workspace_bytes(P, N, M)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    check(_lib.dr_procrustes_f32(P, N, M, ptr(conf), ptr(src_pcd.contiguous().float()), ptr(tgt_pcd.contiguous().float()),
                                 ptr(sm), ptr(tm), 1 if use_mask_len else 0, float(sample_rate), float(max_condition_num),
                                 ptr(R), ptr(t), ptr(Rf), ptr(tf), ptr(cond), ptr(ok), ptr(idx), ptr(ws), wsb, stream_of(conf)))
    res = (R, t, Rf, tf, cond, ok.bool())
    return res + (idx,) if want_topk else res


def procrustes_backward(conf, src_pcd, tgt_pcd, topk_idx, grad_R, grad_t, k_count=None):
    """d loss / d conf [P,N,M] of the weighted Procrustes fit on the entries `topk_idx` [P,K] (int32) selected by procrustes(..., want_topk=True)"""
    ensure_init()
    conf = conf.contiguous().float()
    P, N, M = conf.shape
    K = topk_idx.shape[1]
    g = torch.empty(P, N, M, device=conf.device)
    kc = k_count.to(device=conf.device, dtype=torch.int32).contiguous() if k_count is not None else None
    check(_lib.dr_procrustes_backward_f32(P, N, M, K, ptr(conf), ptr(src_pcd.contiguous().float()), ptr(tgt_pcd.contiguous().float()),
                                          ptr(topk_idx.contiguous()), ptr(kc), ptr(grad_R.contiguous().float().reshape(P, 9)),
                                          ptr(grad_t.contiguous().float().reshape(P, 3)), ptr(g), stream_of(conf)))
    return g


def top1_union(conf):
    """conf [P,N,M] (f32/f64) -> list of int64 [K_p,3] match tensors (one host sync for the counts)."""
    ensure_init()
    conf = conf.contiguous()
    P, N, M = conf.shape
    out = torch.empty(P, N + M, 3, dtype=torch.int64, device=conf.device)
    cnt = torch.empty(P, dtype=torch.int32, device=conf.device)
    f64 = conf.dtype == torch.float64
    fn = _lib.dr_top1_union_f64 if f64 else _lib.dr_top1_union_f32
    wsb = _lib.dr_top1_union_workspace_bytes(P, N, M, 8 if f64 else 4)
    ws = torch.empty(wsb, dtype=torch.uint8, device=conf.device) if wsb else None
    check(fn(P, N, M, ptr(conf), ptr(out), ptr(cnt), ptr(ws), wsb, stream_of(conf)))
    counts = cnt.cpu().tolist()
    return [out[p, :counts[p]] for p in range(P)]


# ------------------------------------------------------------------------------------------------
# evaluation harness.  matches int64 [P,cap,3], count int32 [P] (the loop's own output layout)
# ------------------------------------------------------------------------------------------------
def _f32c(x, shape):
    x = x.to(torch.float32).reshape(shape).contiguous()
    return x


def inlier_ratio(matches, count, s_pcd, t_pcd, rot, trn, inlier_thr, s2t_flow=None):
    """-> (ir [P] float32, n_inlier [P] int32)   (MatchMotionLoss.compute_inlier_ratio, 3D/models/loss.py:383-410)"""
    matches = matches.contiguous()
    P, cap, _ = matches.shape
    N, M = s_pcd.shape[1], t_pcd.shape[1]
    dev = matches.device
    ir = torch.empty(P, device=dev)
    n_inl = torch.empty(P, dtype=torch.int32, device=dev)
    flow = None if s2t_flow is None else _f32c(s2t_flow, (P, N, 3))
    check(_lib.dr_inlier_ratio_f32(P, cap, N, M, ptr(matches), ptr(count.contiguous()), ptr(_f32c(s_pcd, (P, N, 3))),
                                   ptr(_f32c(t_pcd, (P, M, 3))), ptr(_f32c(rot, (P, 9))), ptr(_f32c(trn, (P, 3))), ptr(flow),
                                   float(inlier_thr), ptr(ir), ptr(n_inl), stream_of(matches)))
    return ir, n_inl


def nrfmr(matches, count, s_pcd, t_pcd, raw_pcd, raw_flow, raw_offsets, metric_index, q_offsets, max_q, rot, trn,
          knn_radius=0.1, recall_thr=0.04, want_blended=False):
    """-> (nrfmr [P] float32, n_recalled [P] int32[, blended [sum Q,3]])   (compute_nrfmr, 3D/lib/tester.py:150-210)"""
    matches = matches.contiguous()
    P, cap, _ = matches.shape
    N, M = s_pcd.shape[1], t_pcd.shape[1]
    dev = matches.device
    out = torch.empty(P, device=dev)
    n_rec = torch.empty(P, dtype=torch.int32, device=dev)
    bl = torch.empty(metric_index.shape[0], 3, device=dev) if want_blended else None
    check(_lib.dr_nrfmr_f32(P, cap, N, M, ptr(matches), ptr(count.contiguous()), ptr(_f32c(s_pcd, (P, N, 3))),
                            ptr(_f32c(t_pcd, (P, M, 3))), ptr(_f32c(raw_pcd, (-1, 3))), ptr(_f32c(raw_flow, (-1, 3))),
                            ptr(raw_offsets.contiguous()), ptr(metric_index.contiguous()), ptr(q_offsets.contiguous()), int(max_q),
                            ptr(_f32c(rot, (P, 9))), ptr(_f32c(trn, (P, 3))), float(knn_radius), float(recall_thr), ptr(out),
                            ptr(n_rec), ptr(bl), stream_of(matches)))
    return (out, n_rec, bl) if want_blended else (out, n_rec)


def ransac_corr(matches, count, s_pcd, t_pcd, distance_thr=0.05, iters=50000, seed=0, pair_ids=None):
    """-> dict(rot [P,3,3], trn [P,3,1] float64, fitness [P], inlier_rmse [P], best_iter [P] int32)
    (ransac_regist_coarse / Open3D correspondence RANSAC, 3D/models/loss.py:13-24, 347-379)"""
    matches = matches.contiguous()
    P, cap, _ = matches.shape
    N, M = s_pcd.shape[1], t_pcd.shape[1]
    dev = matches.device
    f64 = dict(dtype=torch.float64, device=dev)
    rot, trn = torch.empty(P, 3, 3, **f64), torch.empty(P, 3, 1, **f64)
    fit, rmse = torch.empty(P, **f64), torch.empty(P, **f64)
    bi = torch.empty(P, dtype=torch.int32, device=dev)
    wsb = _lib.dr_ransac_workspace_bytes(P, cap, int(iters))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    ids = None if pair_ids is None else pair_ids.to(device=dev, dtype=torch.int64).contiguous()
    check(_lib.dr_ransac_corr_f64(P, cap, N, M, ptr(matches), ptr(count.contiguous()), ptr(_f32c(s_pcd, (P, N, 3))),
                                  ptr(_f32c(t_pcd, (P, M, 3))), float(distance_thr), int(iters), int(seed), ptr(ids), ptr(rot),
                                  ptr(trn), ptr(fit), ptr(rmse), ptr(bi), ptr(ws), wsb, stream_of(matches)))
    return dict(rot=rot, trn=trn, fitness=fit, inlier_rmse=rmse, best_iter=bi)


def registration_recall(rot_est, trn_est, rot_gt, trn_gt, info, thr=0.2):
    """-> (err [P] float64, success [P] int32)   (compute_registration_recall, 3D/models/loss.py:27-44, 415-448)"""
    P = rot_est.shape[0]
    dev = rot_est.device
    err = torch.empty(P, dtype=torch.float64, device=dev)
    ok = torch.empty(P, dtype=torch.int32, device=dev)
    d = lambda x, s: x.to(torch.float64).reshape(s).contiguous()
    check(_lib.dr_registration_recall_f64(P, ptr(d(rot_est, (P, 9))), ptr(d(trn_est, (P, 3))), ptr(_f32c(rot_gt, (P, 9))),
                                          ptr(_f32c(trn_gt, (P, 3))), ptr(d(info, (P, 36))), float(thr), ptr(err), ptr(ok),
                                          stream_of(rot_est)))
    return err, ok


# ------------------------------------------------------------------------------------------------
# evaluation metrics of the 2D-3D model (ABI 0.7.0, csrc/eval2d3d.hip): one pair per call, asynchronous, results stay on the device
# ------------------------------------------------------------------------------------------------
def _i64c(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()


def _t44(x, dev):
    return torch.as_tensor(x).to(device=dev, dtype=torch.float64).reshape(4, 4).contiguous()


def sparse_corr_eval(img_num_nodes, pcd_num_nodes, img_node_corr_indices, pcd_node_corr_indices, gt_img_node_corr_indices,
                     gt_pcd_node_corr_indices, gt_node_corr_min_overlaps=None, acceptance_overlap=0.0):
    """-> (out [4] float64: list precision, set precision, recall, hit_ratio; counts [4] int32: unique predictions, unique GT, unique positives,
    listed positives)   (EvalFunction.evaluate_coarse_matching, EXP/loss.py:247-264; evaluate_sparse_correspondences, registration_utils.py:202-225)"""
    ensure_init()
    dev = img_node_corr_indices.device
    pi, pp = _i64c(img_node_corr_indices, dev), _i64c(pcd_node_corr_indices, dev)
    gi, gp = _i64c(gt_img_node_corr_indices, dev), _i64c(gt_pcd_node_corr_indices, dev)
    ov = None if gt_node_corr_min_overlaps is None else _f32c(torch.as_tensor(gt_node_corr_min_overlaps).to(dev), (-1,))
    out = torch.empty(4, dtype=torch.float64, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    wsb = _lib.dr_sparse_corr_eval_workspace_bytes(int(img_num_nodes), int(pcd_num_nodes))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_sparse_corr_eval_i64(int(img_num_nodes), int(pcd_num_nodes), pi.shape[0], ptr(pi) if pi.shape[0] else None,
                                       ptr(pp) if pi.shape[0] else None, gi.shape[0], ptr(gi) if gi.shape[0] else None,
                                       ptr(gp) if gi.shape[0] else None, ptr(ov) if gi.shape[0] else None, float(acceptance_overlap), ptr(out),
                                       ptr(counts), ptr(ws), wsb, stream_of(out)))
    return out, counts


def corr_eval(pcd_corr_points, img_corr_points, transform, positive_radius, sel_indices=None, depth_mask=False):
    """-> (out [4] float64: inlier ratio, mean residual, overlap, EvalFunction's (depth-masked) IR; counts [4] int32: inliers, overlapping image
    points, kept by the mask, inliers among those)   (evaluate_correspondences, registration_utils.py:151-173; evaluate_fine_matching,
    EXP/loss.py:266-278).  sel_indices int64: the correspondences that take part (None = all)."""
    ensure_init()
    dev = pcd_corr_points.device
    n = pcd_corr_points.shape[0]
    pc, ic = _f32c(pcd_corr_points, (n, 3)), _f32c(img_corr_points, (n, 3))
    sel = None if sel_indices is None else _i64c(sel_indices, dev)
    m = n if sel is None else sel.shape[0]
    out = torch.empty(4, dtype=torch.float64, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    wsb = _lib.dr_corr_eval_workspace_bytes(m)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    if sel is not None and m == 0:                              # an empty selection is not "all of them"
        n, sel = 0, None
    check(_lib.dr_corr_eval_f32(n, ptr(pc) if n else None, ptr(ic) if n else None, ptr(_t44(transform, dev)), float(positive_radius), m if sel is not None else 0,
                                ptr(sel), 1 if depth_mask else 0, ptr(out), ptr(counts), ptr(ws), wsb, stream_of(out)))
    return out, counts


def registration_eval(pcd_points, gt_transform, est_transform, rmse_threshold):
    """-> (out [4] float64: eval.py's RMSE, EvalFunction's "rmse", RRE in degrees, RTE; recall [2] int32: either one < rmse_threshold)
    (registration_rmse / isotropic_registration_error, array_ops/metrics.py:25-121; EvalFunction.evaluate_registration, EXP/loss.py:280-294)"""
    ensure_init()
    dev = gt_transform.device if pcd_points is None else pcd_points.device
    N = 0 if pcd_points is None else pcd_points.shape[0]
    pts = None if N == 0 else _f32c(pcd_points, (N, 3))
    out = torch.empty(4, dtype=torch.float64, device=dev)
    recall = torch.empty(2, dtype=torch.int32, device=dev)
    wsb = _lib.dr_registration_eval_workspace_bytes(N)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_registration_eval_f64(N, ptr(pts), ptr(_t44(gt_transform, dev)), ptr(_t44(est_transform, dev)), float(rmse_threshold), ptr(out),
                                        ptr(recall), ptr(ws), wsb, stream_of(out)))
    return out, recall


# ------------------------------------------------------------------------------------------------
# geometry head and feature-layout glue of the 2D-3D forward (ABI 0.7.0, second set, csrc/front2d3d.hip): one image per call, asynchronous
# ------------------------------------------------------------------------------------------------
def _scalar_or_dev(x, dev):
    """a Python number stays on the host; a tensor is read by the kernel from device memory (no synchronisation)"""
    if torch.is_tensor(x):
        return 0.0, x.detach().to(device=dev, dtype=torch.float32).reshape(-1)[:1].contiguous()
    return float(x), None


def back_project_points(depth, intrinsics, mode=0, a=1000.0, b=0.0, depth_limit=None, pixels=False):
    """depth [H,W], intrinsics [3,3] -> (points [H*W,3] float32, mask [H*W] uint8, pixels [H*W,2] float32 or None)   (dr_back_project_f32:
    mode 0 vision3d.ops.back_project, z = depth / a; mode 1 MATR2D3D.back_project_depth, z = depth * a + b with a / b numbers or device tensors)"""
    ensure_init()
    if depth.dim() != 2:
        raise ValueError("back_project_points takes one depth image [H, W] (got %s)" % (tuple(depth.shape),))
    H, W = depth.shape
    dev = depth.device
    d, K = _f32c(depth, (H, W)), _f32c(intrinsics.to(dev), (3, 3))
    (ah, ad), (bh, bd) = _scalar_or_dev(a, dev), _scalar_or_dev(b, dev)
    pts = torch.empty(H * W, 3, device=dev)
    mask = torch.empty(H * W, dtype=torch.uint8, device=dev)
    pix = torch.empty(H * W, 2, device=dev) if pixels else None
    check(_lib.dr_back_project_f32(H, W, ptr(d) if H * W else None, ptr(K), int(mode), ah, bh, ptr(ad), ptr(bd), 0 if depth_limit is None else 1,
                                   0.0 if depth_limit is None else float(depth_limit), ptr(pts) if H * W else None,
                                   ptr(mask) if H * W else None, ptr(pix) if pixels and H * W else None, stream_of(pts)))
    return pts, mask, pix


def render_points(points, intrinsics, extrinsics=None, eps=1e-8, return_depth=False):
    """points [N,3], intrinsics [3,3], extrinsics [4,4] or None -> pixels [N,2] float32 (h, w), not rounded (+ depth [N])   (dr_render_f32)"""
    ensure_init()
    N = points.shape[0]
    dev = points.device
    p, K = _f32c(points, (N, 3)), _f32c(intrinsics.to(dev), (3, 3))
    T = None if extrinsics is None else _f32c(extrinsics.to(dev), (4, 4))
    pix = torch.empty(N, 2, device=dev)
    z = torch.empty(N, device=dev) if return_depth else None
    check(_lib.dr_render_f32(N, ptr(p) if N else None, ptr(K), ptr(T), float(eps), ptr(pix) if N else None, ptr(z) if N else None, stream_of(pix)))
    return (pix, z) if return_depth else pix


def resize_tokens(feats, size):
    """feats [C,Hs,Ws] -> [Hd*Wd, C]: bilinear, align_corners=True, written as token rows   (dr_resize_tokens_f32)"""
    ensure_init()
    C, Hs, Ws = feats.shape
    Hd, Wd = int(size[0]), int(size[1])
    x = _f32c(feats, (C, Hs, Ws))
    out = torch.empty(Hd * Wd, C, device=x.device)
    check(_lib.dr_resize_tokens_f32(C, Hs, Ws, Hd, Wd, ptr(x) if x.numel() else None, ptr(out) if out.numel() else None, stream_of(out)))
    return out


def resize_tokens_backward(grad_out, src_shape, size):
    """grad_out [Hd*Wd, C] -> grad of the [C,Hs,Ws] input; a gather, bit-identical between runs   (dr_resize_tokens_backward_f32)"""
    ensure_init()
    C, Hs, Ws = (int(v) for v in src_shape)
    Hd, Wd = int(size[0]), int(size[1])
    g = _f32c(grad_out, (Hd * Wd, C))
    gi = torch.empty(C, Hs, Ws, device=g.device)
    check(_lib.dr_resize_tokens_backward_f32(C, Hs, Ws, Hd, Wd, ptr(g) if g.numel() else None, ptr(gi) if gi.numel() else None, stream_of(gi)))
    return gi


def conv_out_size(n, k, stride=1, padding=0, dilation=1):
    """nn.Conv2d's output extent (conv_index.h: conv_out_size)"""
    span = n + 2 * padding - dilation * (k - 1) - 1
    return 0 if span < 0 else span // stride + 1


def pack_conv_weight(weight):
    """nn.Conv2d weight [Cout, Cin, k, k] -> the packed [Cout, k k Cin] (tap-major, ci-minor) dr_conv2d_rows_f32 reads"""
    Cout, Cin, kh, kw = weight.shape
    if kh != kw:
        raise NotImplementedError("libdiffreg_hip: conv2d_rows takes square kernels (got %d x %d)" % (kh, kw))
    return weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, kh * kw * Cin).contiguous()


def conv2d_rows(x, size, w_packed, k, bias=None, stride=1, padding=0, dilation=1, addend=None, out=None):
    """nn.Conv2d on token rows: x [Hi*Wi, Cin] (a row stride >= Cin is taken as the leading dimension), size = (Hi, Wi), w_packed from
    pack_conv_weight -> (out [Ho*Wo, Cout], (Ho, Wo)); addend [Ho*Wo, Cout] is added last   (dr_conv2d_rows_f32)"""
    ensure_init()
    Hi, Wi = int(size[0]), int(size[1])
    Cin, Cout = x.shape[1], w_packed.shape[0]
    if x.shape[0] != Hi * Wi or w_packed.shape[1] != k * k * Cin or (Cin > 1 and x.stride(1) != 1):
        raise ValueError("conv2d_rows: x %s / weight %s do not fit a %d x %d image and a %d x %d kernel" % (tuple(x.shape), tuple(w_packed.shape),
                                                                                                         Hi, Wi, k, k))
    Ho, Wo = conv_out_size(Hi, k, stride, padding, dilation), conv_out_size(Wi, k, stride, padding, dilation)
    if out is None:
        out = torch.empty(max(Ho * Wo, 0), Cout, device=x.device)
    rawp = lambda t_: None if t_ is None else c_void_p(t_.data_ptr())
    check(_lib.dr_conv2d_rows_f32(Hi, Wi, Cin, Cout, k, stride, padding, dilation, rawp(x), x.stride(0), ptr(w_packed), ptr(bias), rawp(addend),
                                  addend.stride(0) if addend is not None else 0, rawp(out), out.stride(0), stream_of(x)))
    return out, (Ho, Wo)


def resize_rows(x, src_size, size, addend=None, out=None):
    """x [Hs*Ws, C] rows -> [Hd*Wd, C] rows: bilinear, align_corners=True, out = addend + resample(x)   (dr_resize_rows_f32)"""
    ensure_init()
    Hs, Ws = int(src_size[0]), int(src_size[1])
    Hd, Wd = int(size[0]), int(size[1])
    C = x.shape[1]
    if x.shape[0] != Hs * Ws or (C > 1 and x.stride(1) != 1):
        raise ValueError("resize_rows: x %s is not a %d x %d image of rows" % (tuple(x.shape), Hs, Ws))
    if out is None:
        out = torch.empty(Hd * Wd, C, device=x.device)
    rawp = lambda t_: None if t_ is None else c_void_p(t_.data_ptr())
    check(_lib.dr_resize_rows_f32(C, Hs, Ws, Hd, Wd, rawp(x), x.stride(0), rawp(addend), addend.stride(0) if addend is not None else 0, rawp(out),
                                  out.stride(0), stream_of(x)))
    return out


CONV_RELU_IN, CONV_RELU_OUT = 1, 2          # DR_CONV_RELU_IN, DR_CONV_RELU_OUT


def _rows_ok(t_, n, C):
    return t_.dim() == 2 and t_.shape[0] == n and t_.shape[1] == C and (C == 1 or t_.stride(1) == 1)


def conv2d_rows_act(x, size, w_packed, k, bias=None, stride=1, padding=0, dilation=1, relu_in=False, relu_out=False, addend=None, addend2=None,
                    out=None):
    """conv2d_rows with the DPT head's epilogue: out = relu_out?(conv(relu_in?(x)) + bias) + addend + addend2 -> (out [Ho*Wo, Cout], (Ho, Wo)).
    relu_in leaves x itself untouched; relu_out comes after the bias and before the addends; out must not share memory with an input.
    Flags and addend2 need Cin % 4 == 0   (dr_conv2d_rows_act_f32)"""
    ensure_init()
    Hi, Wi = int(size[0]), int(size[1])
    Cin, Cout = x.shape[1], w_packed.shape[0]
    if x.shape[0] != Hi * Wi or w_packed.shape[1] != k * k * Cin or (Cin > 1 and x.stride(1) != 1):
        raise ValueError("conv2d_rows_act: x %s / weight %s do not fit a %d x %d image and a %d x %d kernel" % (tuple(x.shape), tuple(w_packed.shape),
                                                                                                             Hi, Wi, k, k))
    Ho, Wo = conv_out_size(Hi, k, stride, padding, dilation), conv_out_size(Wi, k, stride, padding, dilation)
    for name, a in (("addend", addend), ("addend2", addend2)):
        if a is not None and not _rows_ok(a, Ho * Wo, Cout):
            raise ValueError("conv2d_rows_act: %s %s is not [%d, %d] rows" % (name, tuple(a.shape), Ho * Wo, Cout))
    if out is None:
        out = torch.empty(max(Ho * Wo, 0), Cout, device=x.device)
    rawp = lambda t_: None if t_ is None else c_void_p(t_.data_ptr())
    flags = (CONV_RELU_IN if relu_in else 0) | (CONV_RELU_OUT if relu_out else 0)
    check(_lib.dr_conv2d_rows_act_f32(Hi, Wi, Cin, Cout, k, stride, padding, dilation, rawp(x), x.stride(0), ptr(w_packed), ptr(bias), flags,
                                      rawp(addend), addend.stride(0) if addend is not None else 0, rawp(addend2),
                                      addend2.stride(0) if addend2 is not None else 0, rawp(out), out.stride(0), stream_of(x)))
    return out, (Ho, Wo)


def pack_conv_transpose_weight(weight):
    """nn.ConvTranspose2d weight [Cin, Cout, s, s] -> the packed [s s Cout, Cin] ((i, j) major, co minor) dr_conv_transpose2d_rows_f32 reads"""
    Cin, Cout, kh, kw = weight.shape
    if kh != kw:
        raise NotImplementedError("libdiffreg_hip: conv_transpose2d_rows takes square kernels (got %d x %d)" % (kh, kw))
    return weight.detach().float().permute(2, 3, 1, 0).reshape(kh * kw * Cout, Cin).contiguous()


def conv_transpose2d_rows(x, size, w_packed, s, bias=None, out=None):
    """nn.ConvTranspose2d(kernel = stride = s, padding 0) on token rows: x [H*W, Cin], size = (H, W), w_packed from pack_conv_transpose_weight
    -> (out [H s * W s, Cout], (H s, W s)), every element written   (dr_conv_transpose2d_rows_f32)"""
    ensure_init()
    H, W, s = int(size[0]), int(size[1]), int(s)
    Cin = x.shape[1]
    if s < 1 or x.shape[0] != H * W or w_packed.shape[1] != Cin or w_packed.shape[0] % (s * s) != 0 or (Cin > 1 and x.stride(1) != 1):
        raise ValueError("conv_transpose2d_rows: x %s / weight %s do not fit a %d x %d image and stride %d" % (tuple(x.shape), tuple(w_packed.shape),
                                                                                                            H, W, s))
    Cout = w_packed.shape[0] // (s * s)
    if out is None:
        out = torch.empty(H * s * W * s, Cout, device=x.device)
    elif not _rows_ok(out, H * s * W * s, Cout):
        raise ValueError("conv_transpose2d_rows: out %s is not [%d, %d] rows" % (tuple(out.shape), H * s * W * s, Cout))
    check(_lib.dr_conv_transpose2d_rows_f32(H, W, Cin, Cout, s, c_void_p(x.data_ptr()), x.stride(0), ptr(w_packed), ptr(bias),
                                            c_void_p(out.data_ptr()), out.stride(0), stream_of(x)))
    return out, (H * s, W * s)


def conv2d_rows_project(x, size, w1_packed, k, b1, w2, b2=None, stride=1, padding=0, dilation=1, relu_out=True, out=None):
    """conv k x k (Cin -> Cmid <= 64, w1_packed from pack_conv_weight, + b1) -> ReLU -> w2 [Cmid] . (.) + b2 [1] -> ReLU if relu_out, in one
    launch: x [Hi*Wi, Cin] rows -> (out [Ho*Wo] or a strided view of that length, (Ho, Wo))   (dr_conv2d_rows_project_f32)"""
    ensure_init()
    Hi, Wi = int(size[0]), int(size[1])
    Cin, Cmid = x.shape[1], w1_packed.shape[0]
    if x.shape[0] != Hi * Wi or w1_packed.shape[1] != k * k * Cin or (Cin > 1 and x.stride(1) != 1) or w2.numel() != Cmid or \
            (b2 is not None and b2.numel() != 1):
        raise ValueError("conv2d_rows_project: x %s / w1 %s / w2 %s do not fit a %d x %d image and a %d x %d kernel"
                         % (tuple(x.shape), tuple(w1_packed.shape), tuple(w2.shape), Hi, Wi, k, k))
    Ho, Wo = conv_out_size(Hi, k, stride, padding, dilation), conv_out_size(Wi, k, stride, padding, dilation)
    if out is None:
        out = torch.empty(max(Ho * Wo, 0), device=x.device)
    elif out.dim() != 1 or out.shape[0] != Ho * Wo:
        raise ValueError("conv2d_rows_project: out %s is not [%d]" % (tuple(out.shape), Ho * Wo))
    check(_lib.dr_conv2d_rows_project_f32(Hi, Wi, Cin, Cmid, k, stride, padding, dilation, c_void_p(x.data_ptr()), x.stride(0), ptr(w1_packed),
                                          ptr(b1), ptr(w2), ptr(b2), 1 if relu_out else 0, c_void_p(out.data_ptr()),
                                          out.stride(0) if out.numel() > 1 else 1, stream_of(x)))
    return out, (Ho, Wo)


def pack_conv_weight_t(weight):
    """nn.Conv2d weight [Cout, Cin, k, k] -> the packed [Cin, k k Cout] (tap-major, co-minor) dr_conv2d_rows_backward_data_f32 reads"""
    Cout, Cin, kh, kw = weight.shape
    if kh != kw:
        raise NotImplementedError("libdiffreg_hip: conv2d_rows takes square kernels (got %d x %d)" % (kh, kw))
    return weight.detach().float().permute(1, 2, 3, 0).reshape(Cin, kh * kw * Cout).contiguous()


def conv_wgrad_slabs(M):
    """(S, L): the slabs of output pixels dr_conv2d_rows_backward_weight_f32 reduces over (conv_index.h: conv_wgrad_slabs) -- a function of
    M = Ho Wo alone: S0 = min(64, ceil(M / 2048)), L = ceil(M / S0) rounded up to 32, S = ceil(M / L)"""
    s0 = max(1, min(64, -(-M // 2048)))
    L = max(32, -(-(-(-M // s0)) // 32) * 32)
    return max(1, -(-M // L)), L


def conv_wgrad_workspace_bytes(M, Cout, K):
    """the workspace of dr_conv2d_rows_backward_weight_f32: float32 partials [S, Cout, K] rounded up to 8 bytes, double partials [S, Cout]"""
    S, _ = conv_wgrad_slabs(M)
    return (S * Cout * K * 4 + 7) // 8 * 8 + S * Cout * 8


def _rawp(t_):
    return None if t_ is None else c_void_p(t_.data_ptr())


def conv2d_rows_backward_data(grad_out, size, w_packed_t, k, stride=1, padding=0, dilation=1, addend=None, out=None):
    """grad_out [Ho*Wo, Cout] rows of the convolution of a size = (Hi, Wi) image, w_packed_t from pack_conv_weight_t -> grad_x [Hi*Wi, Cin]
    (+ addend), every element written   (dr_conv2d_rows_backward_data_f32)"""
    ensure_init()
    Hi, Wi = int(size[0]), int(size[1])
    Cout, Cin = grad_out.shape[1], w_packed_t.shape[0]
    Ho, Wo = conv_out_size(Hi, k, stride, padding, dilation), conv_out_size(Wi, k, stride, padding, dilation)
    if grad_out.shape[0] != Ho * Wo or w_packed_t.shape[1] != k * k * Cout or (Cout > 1 and grad_out.stride(1) != 1):
        raise ValueError("conv2d_rows_backward_data: grad_out %s / weight %s do not fit a %d x %d image and a %d x %d kernel"
                         % (tuple(grad_out.shape), tuple(w_packed_t.shape), Hi, Wi, k, k))
    if out is None:
        out = torch.empty(Hi * Wi, Cin, device=grad_out.device)
    check(_lib.dr_conv2d_rows_backward_data_f32(Hi, Wi, Cin, Cout, k, stride, padding, dilation, _rawp(grad_out), grad_out.stride(0), ptr(w_packed_t),
                                                _rawp(addend), addend.stride(0) if addend is not None else 0, _rawp(out), out.stride(0),
                                                stream_of(grad_out)))
    return out


def conv2d_rows_backward_weight(x, size, grad_out, k, stride=1, padding=0, dilation=1, need_weight=True, need_bias=True, packed=False):
    """x [Hi*Wi, Cin], grad_out [Ho*Wo, Cout] rows -> (grad_weight in the module's layout [Cout, Cin, k, k] -- or packed [Cout, k k Cin] with
    packed=True -- or None, grad_bias [Cout] or None)   (dr_conv2d_rows_backward_weight_f32)"""
    ensure_init()
    Hi, Wi = int(size[0]), int(size[1])
    Cin, Cout = x.shape[1], grad_out.shape[1]
    Ho, Wo = conv_out_size(Hi, k, stride, padding, dilation), conv_out_size(Wi, k, stride, padding, dilation)
    if x.shape[0] != Hi * Wi or grad_out.shape[0] != Ho * Wo or (Cin > 1 and x.stride(1) != 1) or (Cout > 1 and grad_out.stride(1) != 1):
        raise ValueError("conv2d_rows_backward_weight: x %s / grad_out %s do not fit a %d x %d image and a %d x %d kernel"
                         % (tuple(x.shape), tuple(grad_out.shape), Hi, Wi, k, k))
    dev = x.device
    gw = torch.empty(Cout, k * k * Cin, device=dev) if need_weight else None
    gb = torch.empty(Cout, device=dev) if need_bias else None
    wsb = _lib.dr_conv2d_rows_backward_weight_workspace_bytes(Hi, Wi, Cin, Cout, k, stride, padding, dilation)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_conv2d_rows_backward_weight_f32(Hi, Wi, Cin, Cout, k, stride, padding, dilation, _rawp(x), x.stride(0), _rawp(grad_out),
                                                  grad_out.stride(0), ptr(gw), ptr(gb), ptr(ws), wsb, stream_of(x)))
    if gw is not None and not packed:
        gw = gw.view(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
    return gw, gb


def resize_rows_backward(grad_out, src_size, size, out=None):
    """grad_out [Hd*Wd, C] rows -> the gradient [Hs*Ws, C] of resize_rows' input; a gather, every element written   (dr_resize_rows_backward_f32)"""
    ensure_init()
    Hs, Ws = int(src_size[0]), int(src_size[1])
    Hd, Wd = int(size[0]), int(size[1])
    C = grad_out.shape[1]
    if grad_out.shape[0] != Hd * Wd or (C > 1 and grad_out.stride(1) != 1):
        raise ValueError("resize_rows_backward: grad_out %s is not a %d x %d image of rows" % (tuple(grad_out.shape), Hd, Wd))
    if out is None:
        out = torch.empty(Hs * Ws, C, device=grad_out.device)
    check(_lib.dr_resize_rows_backward_f32(C, Hs, Ws, Hd, Wd, _rawp(grad_out), grad_out.stride(0), _rawp(out), out.stride(0), stream_of(grad_out)))
    return out


def rows_normalize_chw(feats):
    """feats [C,P] -> [P,C], rows divided by max(|row|_2, 1e-12)   (dr_rows_normalize_chw_f32; C <= 256)"""
    ensure_init()
    C, P = feats.shape
    x = _f32c(feats, (C, P))
    out = torch.empty(P, C, device=x.device)
    check(_lib.dr_rows_normalize_chw_f32(C, P, ptr(x) if x.numel() else None, ptr(out) if out.numel() else None, stream_of(out)))
    return out


def rows_normalize_chw_backward(feats, grad_out, rows=None):
    """feats [C,P] and the gradient of rows_normalize_chw's output -> the gradient of feats [C,P].  rows None: grad_out is dense [P,C]
    (dr_rows_normalize_chw_backward_f32); rows int64 [K]: grad_out is [K,C], the gradient of output rows `rows` (repeats accumulate), zero elsewhere
    (dr_rows_normalize_chw_backward_rows_f32; a row outside [0, P) is skipped and reported by device_status())"""
    ensure_init()
    C, P = feats.shape
    x = _f32c(feats, (C, P))
    gi = torch.empty(C, P, device=x.device)
    if rows is None:
        g = _f32c(grad_out, (P, C))
        check(_lib.dr_rows_normalize_chw_backward_f32(C, P, ptr(x) if x.numel() else None, ptr(g) if g.numel() else None,
                                                      ptr(gi) if gi.numel() else None, stream_of(gi)))
    else:
        r = _i64c(rows, x.device)
        K = r.shape[0]
        g = _f32c(grad_out, (K, C))
        check(_lib.dr_rows_normalize_chw_backward_rows_f32(C, P, K, ptr(x) if x.numel() else None, ptr(r) if K else None,
                                                           ptr(g) if g.numel() else None, ptr(gi) if gi.numel() else None, stream_of(gi)))
    return gi


# ------------------------------------------------------------------------------------------------
# collate-time ops: stacked clouds [n,3] float32 + lengths int32 [nb], all on the device
# ------------------------------------------------------------------------------------------------
def grid_subsample(points, lengths, dl, vision3d=False, open3d=False):
    """-> (sub_points [n,3] buffer, sub_lengths [nb] int32, total [1] int32, status [1] int32), asynchronous; the first
    total[0] rows of the buffer are valid (cpp_subsampling.subsample_batch, grid_subsampling.cpp:4-211; vision3d = True: the
    2D-3D loader's vision3d/csrc/cpu/grid_subsampling/grid_subsampling.cpp, whose grid origin is floor(min / dl) * dl; open3d = True:
    the origin of Open3D's voxel_down_sample, min - 0.5 * dl)"""
    points = points.to(torch.float32).contiguous()
    lengths = lengths.to(device=points.device, dtype=torch.int32).contiguous()
    n, nb = points.shape[0], lengths.shape[0]
    dev = points.device
    out = torch.empty(max(n, 1), 3, device=dev)
    ol = torch.empty(nb, dtype=torch.int32, device=dev)
    tot = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _lib.dr_grid_subsample_workspace_bytes(n, nb)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    entry = _lib.dr_grid_subsample_open3d_f32 if open3d else _lib.dr_grid_subsample_vision3d_f32 if vision3d else _lib.dr_grid_subsample_f32
    check(entry(n, nb, ptr(points), ptr(lengths), float(dl), ptr(out), ptr(ol), ptr(tot), ptr(status), ptr(ws), wsb, stream_of(points)))
    return out, ol, tot, status


def radius_neighbors(queries, supports, q_lengths, s_lengths, radius, limit):
    """-> (neighbors int64 [nq, limit], max_count [1] int32, status [1] int32), asynchronous
    (cpp_neighbors.batch_query + [:, :limit], neighbors.cpp:210-333)"""
    queries = queries.to(torch.float32).contiguous()
    supports = supports.to(torch.float32).contiguous()
    dev = queries.device
    ql = q_lengths.to(device=dev, dtype=torch.int32).contiguous()
    sl = s_lengths.to(device=dev, dtype=torch.int32).contiguous()
    nq, ns, nb = queries.shape[0], supports.shape[0], ql.shape[0]
    out = torch.empty(nq, limit, dtype=torch.int64, device=dev)
    mc = torch.empty(1, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _lib.dr_radius_neighbors_workspace_bytes(nq, ns, nb)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_radius_neighbors_f32(nq, ns, nb, ptr(queries), ptr(supports), ptr(ql), ptr(sl), float(radius), int(limit), ptr(out),
                                       ptr(mc), ptr(status), ptr(ws), wsb, stream_of(queries)))
    return out, mc, status


def radius_count_hist(queries, supports, q_lengths, s_lengths, radius, hist, counts=None):
    """hist int32 [hist_n] (device, accumulated in place): hist[c] += 1 for every query with c < hist_n supports of its own cloud at
    d^2 < radius^2; counts int32 [nq] (optional) receives every c.  -> status [1] int32, asynchronous.  The allocations are torch's
    caching allocator's: the call can be captured in a graph (calibrate_neighbors_pack_mode, vision3d/utils/dataloader.py:42-67)."""
    queries = queries.to(torch.float32).contiguous()
    supports = supports.to(torch.float32).contiguous()
    dev = queries.device
    ql = q_lengths.to(device=dev, dtype=torch.int32).contiguous()
    sl = s_lengths.to(device=dev, dtype=torch.int32).contiguous()
    nq, ns, nb = queries.shape[0], supports.shape[0], ql.shape[0]
    if hist.dtype != torch.int32 or hist.dim() != 1 or not hist.is_contiguous() or hist.device != dev:
        raise ValueError("radius_count_hist: hist must be a contiguous int32 vector on the queries' device")
    if counts is not None and (counts.dtype != torch.int32 or counts.shape != (nq,) or not counts.is_contiguous() or counts.device != dev):
        raise ValueError("radius_count_hist: counts must be a contiguous int32 [nq] vector on the queries' device")
    status = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _lib.dr_radius_count_hist_workspace_bytes(nq, ns, nb)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_radius_count_hist_f32(nq, ns, nb, ptr(queries), ptr(supports), ptr(ql), ptr(sl), float(radius), int(hist.shape[0]),
                                        ptr(hist), ptr(counts) if counts is not None else None, ptr(status), ptr(ws), wsb,
                                        stream_of(queries)))
    return status


def _offsets_i32(offsets, n_pairs, dev, name):
    o = offsets.to(device=dev, dtype=torch.int32).contiguous()
    if o.dim() != 1 or (n_pairs is not None and o.shape[0] != n_pairs + 1):
        raise ValueError("%s: offsets must be a vector of P + 1 entries" % name)
    return o


def blend_flow_knn3(query, q_offsets, reference, reference_flow, r_offsets):
    """-> (flow [nq, 3] float32, status [P] int32), asynchronous: blend_scene_flow(query, reference, reference_flow, knn=3) of
    3D/datasets/utils.py:43-59 for P pairs at once; pair p's queries / references are rows [offsets[p], offsets[p + 1]) of the stacked arrays
    (int32 device vectors of P + 1 entries).  status[p]: 0, 1 (fewer than 4 references: its rows of `flow` are zero) or 2 (bad offsets)."""
    ensure_init()
    query = query.to(torch.float32).contiguous()
    dev = query.device
    reference = reference.to(device=dev, dtype=torch.float32).contiguous()
    reference_flow = reference_flow.to(device=dev, dtype=torch.float32).contiguous()
    qo = _offsets_i32(q_offsets, None, dev, "blend_flow_knn3")
    P = qo.shape[0] - 1
    ro = _offsets_i32(r_offsets, P, dev, "blend_flow_knn3")
    nq, nr = query.shape[0], reference.shape[0]
    if query.shape != (nq, 3) or reference.shape != (nr, 3) or reference_flow.shape != (nr, 3):
        raise ValueError("blend_flow_knn3: query [nq, 3], reference and reference_flow [nr, 3]")
    out = torch.zeros(nq, 3, device=dev)
    status = torch.empty(max(P, 0), dtype=torch.int32, device=dev)
    check(_lib.dr_blend_flow_knn3_f32(P, nq, nr, ptr(query) if nq else None, ptr(qo), ptr(reference) if nr else None,
                                      ptr(reference_flow) if nr else None, ptr(ro), ptr(out) if nq else None, ptr(status) if P else None,
                                      stream_of(query)))
    return out, status


def coarse_gt_matches(src, s_offsets, tgt, t_offsets, rot, trn, radius, src_flow=None):
    """-> (out_src [ns] int64, out_tgt [ns] int64, counts [P] int32, status [P] int32), asynchronous: the `get match at coarse level` block of
    collate_fn_3dmatch / collate_fn_4dmatch (dataloader.py:253-257, 512-520) for P pairs at once.  src [ns, 3] / tgt [nt, 3] hold the pairs'
    coarse clouds stacked each on its own, rows [offsets[p], offsets[p + 1]); rot [P, 3, 3], trn [P, 3] (or [P, 3, 1]); src_flow [ns, 3] or None.
    Pair p's matches are out_*[s_offsets[p] : s_offsets[p] + counts[p]], pair-local indices in ascending source order.  status[p]: 0, 1 (a cloud
    of fewer than 2 points: count 0) or 2 (bad offsets)."""
    ensure_init()
    src = src.to(torch.float32).contiguous()
    dev = src.device
    tgt = tgt.to(device=dev, dtype=torch.float32).contiguous()
    so = _offsets_i32(s_offsets, None, dev, "coarse_gt_matches")
    P = so.shape[0] - 1
    to = _offsets_i32(t_offsets, P, dev, "coarse_gt_matches")
    ns, nt = src.shape[0], tgt.shape[0]
    rot = rot.to(device=dev, dtype=torch.float32).contiguous()
    trn = trn.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    if src.shape != (ns, 3) or tgt.shape != (nt, 3) or rot.shape != (P, 3, 3) or trn.shape != (P, 3):
        raise ValueError("coarse_gt_matches: src [ns, 3], tgt [nt, 3], rot [P, 3, 3], trn [P, 3]")
    flow = None
    if src_flow is not None:
        flow = src_flow.to(device=dev, dtype=torch.float32).contiguous()
        if flow.shape != (ns, 3):
            raise ValueError("coarse_gt_matches: src_flow must be [ns, 3]")
    out_src = torch.empty(ns, dtype=torch.int64, device=dev)
    out_tgt = torch.empty(ns, dtype=torch.int64, device=dev)
    counts = torch.empty(max(P, 0), dtype=torch.int32, device=dev)
    status = torch.empty(max(P, 0), dtype=torch.int32, device=dev)
    wsb = _lib.dr_coarse_gt_matches_workspace_bytes(ns, nt)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_coarse_gt_matches_f32(P, ns, nt, ptr(src) if ns else None, ptr(so), ptr(tgt) if nt else None, ptr(to),
                                        ptr(flow) if (flow is not None and ns) else None, ptr(rot) if P else None, ptr(trn) if P else None,
                                        float(radius), ptr(out_src) if ns else None, ptr(out_tgt) if ns else None, ptr(counts) if P else None,
                                        ptr(status) if P else None, ptr(ws), wsb, stream_of(src)))
    return out_src, out_tgt, counts, status


def item3d_prepare(src_raw, s_raw_offsets, tgt_raw, t_raw_offsets, rot, trans, *, s_offsets=None, t_offsets=None, src_sel=None, tgt_sel=None,
                   flow_raw=None, recompute_flow=False, rot_ab=None, coin=None, src_jitter=None, tgt_jitter=None, noise=0.0):
    """dr_item3d_prepare_f32, asynchronous -> dict(src, tgt [n, 3] float32, flow [n_src_raw, 3] or None, rot [P, 3, 3], trans [P, 3],
    tsfm [P, 3, 4] float32, status [P] int32).  The clouds are stacked float32 device tensors with int32 offsets of P + 1 entries; a selection is
    a contiguous int64 device vector of pair-local raw rows, one per output row, with the outputs' offsets next to it; rot_ab [P, 3, 3], coin [P]
    and the jitter draws are float64."""
    ensure_init()
    dev = src_raw.device
    for name, t in (("src_raw", src_raw), ("tgt_raw", tgt_raw), ("flow_raw", flow_raw)):
        if t is not None and (t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous()):
            raise ValueError("item3d_prepare: %s must be a contiguous float32 [n, 3] tensor" % name)
    for name, t in (("src_sel", src_sel), ("tgt_sel", tgt_sel)):
        if t is not None and (t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous()):
            raise ValueError("item3d_prepare: %s must be a contiguous int64 vector" % name)
    sro = _offsets_i32(s_raw_offsets, None, dev, "item3d_prepare")
    P = sro.shape[0] - 1
    tro = _offsets_i32(t_raw_offsets, P, dev, "item3d_prepare")
    so = sro if src_sel is None else _offsets_i32(s_offsets, P, dev, "item3d_prepare")
    to = tro if tgt_sel is None else _offsets_i32(t_offsets, P, dev, "item3d_prepare")
    n_sr, n_tr = src_raw.shape[0], tgt_raw.shape[0]
    n_s = n_sr if src_sel is None else src_sel.shape[0]
    n_t = n_tr if tgt_sel is None else tgt_sel.shape[0]
    if flow_raw is not None and flow_raw.shape[0] != n_sr:
        raise ValueError("item3d_prepare: flow_raw has one row per raw source point")
    if flow_raw is not None and recompute_flow and n_s != n_sr:
        raise ValueError("item3d_prepare: a selection shorter than the cloud leaves no flow to recompute (the reference raises on "
                         "`src_pcd_deformed - src_pcd`)")
    f64 = lambda t, shape, name: None if t is None else _shaped(t.to(device=dev, dtype=torch.float64).contiguous(), shape, name)
    rot = f64(rot, (P, 3, 3), "rot")
    trans = f64(trans.reshape(P, 3), (P, 3), "trans")
    rot_ab = f64(rot_ab, (P, 3, 3), "rot_ab")
    coin = f64(coin, (P,), "coin")
    if rot_ab is not None and coin is None:
        raise ValueError("item3d_prepare: rot_ab needs coin")
    src_jitter, tgt_jitter = f64(src_jitter, (n_s, 3), "src_jitter"), f64(tgt_jitter, (n_t, 3), "tgt_jitter")
    out = dict(src=torch.empty(n_s, 3, device=dev), tgt=torch.empty(n_t, 3, device=dev),
               flow=None if flow_raw is None else torch.empty(n_sr, 3, device=dev), rot=torch.empty(P, 3, 3, device=dev),
               trans=torch.empty(P, 3, device=dev), tsfm=torch.empty(P, 3, 4, device=dev),
               status=torch.empty(P, dtype=torch.int32, device=dev))
    opt = lambda t, n=1: ptr(t) if (t is not None and n) else None
    a = Item3dArgs(P, n_sr, n_tr, n_s, n_t, opt(src_raw, n_sr), ptr(sro), opt(tgt_raw, n_tr), ptr(tro), opt(flow_raw, n_sr), opt(src_sel, n_s),
                   opt(tgt_sel, n_t), ptr(so), ptr(to), opt(rot_ab, P), opt(coin, P), opt(src_jitter, n_s), opt(tgt_jitter, n_t), float(noise),
                   1 if recompute_flow else 0, opt(rot, P), opt(trans, P), opt(out["src"], n_s), opt(out["tgt"], n_t), opt(out["flow"], n_sr),
                   opt(out["rot"], P), opt(out["trans"], P), opt(out["tsfm"], P), opt(out["status"], P))
    check(_lib.dr_item3d_prepare_f32(ctypes.byref(a), stream_of(src_raw)))
    return out


def _shaped(t, shape, name):
    if tuple(t.shape) != tuple(shape):
        raise ValueError("item3d: %s must have shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))
    return t


def radius_pairs_ragged(src, s_offsets, tgt, t_offsets, transforms, radius, c_offsets=None, capacity=0):
    """dr_radius_pairs_ragged_f32, asynchronous -> (out_src, out_tgt int64 [capacity], counts int32 [P, 2] = (written, found), status int32 [P]).
    src [ns, 3] / tgt [nt, 3] contiguous float32, stacked by int32 offsets of P + 1 entries; transforms [P, 3, 4] float32 or None; c_offsets int64
    [P + 1] on the device: pair p's room in the list.  capacity = 0 counts only."""
    ensure_init()
    dev = src.device
    for name, t in (("src", src), ("tgt", tgt)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3 or not t.is_contiguous():
            raise ValueError("radius_pairs_ragged: %s must be a contiguous float32 [n, 3] tensor" % name)
    so = _offsets_i32(s_offsets, None, dev, "radius_pairs_ragged")
    P = so.shape[0] - 1
    to = _offsets_i32(t_offsets, P, dev, "radius_pairs_ragged")
    ns, nt = src.shape[0], tgt.shape[0]
    T = None if transforms is None else _shaped(transforms.to(device=dev, dtype=torch.float32).contiguous(), (P, 3, 4), "transforms")
    capacity = int(capacity)
    co = None
    if capacity > 0:
        co = c_offsets.to(device=dev, dtype=torch.int64).contiguous()
        if co.shape != (P + 1,):
            raise ValueError("radius_pairs_ragged: c_offsets must be a vector of P + 1 entries")
    out_src = torch.empty(capacity, dtype=torch.int64, device=dev)
    out_tgt = torch.empty(capacity, dtype=torch.int64, device=dev)
    counts = torch.zeros(P, 2, dtype=torch.int32, device=dev)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    wsb = _lib.dr_radius_pairs_ragged_workspace_bytes(P, ns, nt)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    check(_lib.dr_radius_pairs_ragged_f32(P, ns, nt, ptr(src) if ns else None, ptr(so), ptr(tgt) if nt else None, ptr(to), ptr(T) if P else None,
                                          float(radius), ptr(co), capacity, ptr(out_src) if capacity else None,
                                          ptr(out_tgt) if capacity else None, ptr(counts) if P else None, ptr(status) if P else None, ptr(ws),
                                          wsb, stream_of(src)))
    return out_src, out_tgt, counts, status


def _item_inputs(name, depth, points, intrinsics, transform):
    """the common operands of the thirteenth set on depth's device: depth float32 [H, W], points float32 / float64 [N, 3] (float64 is kept),
    intrinsics float64 [9], transform float64 [16]"""
    ensure_init()
    dev = depth.device
    depth = depth.to(torch.float32).contiguous()
    points = points.to(device=dev, dtype=torch.float64 if points.dtype == torch.float64 else torch.float32).contiguous()
    K = torch.as_tensor(intrinsics).to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
    T = torch.as_tensor(transform).to(device=dev, dtype=torch.float64).contiguous().reshape(-1)
    if depth.dim() != 2 or points.dim() != 2 or points.shape[1] != 3 or K.numel() != 9 or T.numel() != 16:
        raise ValueError("%s: depth [H, W], points [N, 3], intrinsics [3, 3], transform [4, 4]" % name)
    return depth, points, K, T


def _item_call(fn, size_fn, depth, points, K, T, scaling_factor, depth_limit, radius_2d, radius_3d, caps, outs, counts):
    H, W = depth.shape
    N = points.shape[0]
    wsb = size_fn(H, W, N)
    ws = torch.empty(max(wsb, 32), dtype=torch.uint8, device=depth.device)
    check(fn(H, W, N, ptr(depth) if H * W else None, float(scaling_factor), float("inf") if depth_limit is None else float(depth_limit), ptr(K),
             ptr(points) if N else None, 1 if points.dtype == torch.float64 else 0, ptr(T), float(radius_2d), float(radius_3d), *caps,
             *[ptr(o) if o.numel() else None for o in outs], ptr(counts), ptr(ws), wsb, stream_of(depth)))


def corr_2d3d(depth, points, intrinsics, transform, radius_2d, radius_3d, depth_limit=6.0, scaling_factor=1000.0, method="mutual_nearest",
              cap=None):
    """-> (img_corr_pixels [cap, 2] int64, pcd_corr_indices [cap] int64, counts [2] int32 = (written, found)), asynchronous:
    get_2d3d_correspondences_mutual / _radius of vision3d/array_ops/registration_utils.py:30-89 on dr_corr_2d3d_mutual_f64 /
    dr_corr_2d3d_radius_f64.  cap: rows of the outputs (mutual: min(H W, N) by default, which always suffices; radius: required)."""
    depth, points, K, T = _item_inputs("corr_2d3d", depth, points, intrinsics, transform)
    if method not in ("mutual_nearest", "radius"):
        raise ValueError("corr_2d3d: method is 'mutual_nearest' or 'radius'")
    mutual = method == "mutual_nearest"
    if cap is None:
        if not mutual:
            raise ValueError("corr_2d3d: the radius variant needs cap (count first with cap=0)")
        cap = min(depth.numel(), points.shape[0])
    dev = depth.device
    pix = torch.empty(cap, 2, dtype=torch.int64, device=dev)
    idx = torch.empty(cap, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    fn, size_fn = ((_lib.dr_corr_2d3d_mutual_f64, _lib.dr_corr_2d3d_mutual_workspace_bytes) if mutual else
                   (_lib.dr_corr_2d3d_radius_f64, _lib.dr_corr_2d3d_radius_workspace_bytes))
    _item_call(fn, size_fn, depth, points, K, T, scaling_factor, depth_limit, radius_2d, radius_3d, [int(cap)], [pix, idx], counts)
    return pix, idx, counts


def overlap_2d3d(depth, points, intrinsics, transform, radius_2d, radius_3d, depth_limit=6.0, scaling_factor=1000.0):
    """-> (img_overlap_indices [H W] int64, pcd_overlap_indices [N] int64, counts [4] int32 = (written, found) of either), asynchronous: the
    sorted distinct pixel indices h W + w and point indices of the radius variant's pairs (sevenscenes_hard.py:184-196) on dr_overlap_2d3d_f64;
    the first counts[1] / counts[3] rows are the lists."""
    depth, points, K, T = _item_inputs("overlap_2d3d", depth, points, intrinsics, transform)
    dev = depth.device
    img = torch.empty(depth.numel(), dtype=torch.int64, device=dev)
    pcd = torch.empty(points.shape[0], dtype=torch.int64, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    _item_call(_lib.dr_overlap_2d3d_f64, _lib.dr_overlap_2d3d_workspace_bytes, depth, points, K, T, scaling_factor, depth_limit, radius_2d,
               radius_3d, [img.numel(), pcd.numel()], [img, pcd], counts)
    return img, pcd, counts


def column_mean_seq(x):
    """-> [3] float32: x.mean(axis=0) of a float32 [n, 3] array in numpy's order of additions (row after row), asynchronous"""
    ensure_init()
    x = x.to(torch.float32).contiguous()
    if x.dim() != 2 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError("column_mean_seq: x [n, 3] with n >= 1")
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    check(_lib.dr_column_mean_seq_f32(x.shape[0], ptr(x), ptr(out), stream_of(x)))
    return out


def batch_mutual_topk_select(score_mat, k, row_masks=None, col_masks=None, largest=True, threshold=None, mutual=True):
    """-> (batch_indices, row_indices, col_indices, scores) like vision3d.ops.batch_mutual_topk_select(..., reduce_result=True)
    (Diff-Reg-2d3d/vision3d/ops/mutual_topk_select.py:63-134); a 2-D score_mat is one batch element (mutual_topk_select :7-60,
    returns (row_indices, col_indices, scores)).  One host sync for the number of correspondences."""
    two_d = score_mat.dim() == 2
    s = (score_mat[None] if two_d else score_mat).to(torch.float32).contiguous()
    B, N, M = s.shape
    if k > N or k > M:
        raise RuntimeError("selected index k out of range")      # what torch.topk says in the reference (mutual_topk_select.py:27-28)
    dev = s.device
    cap = B * (min(N, M) if mutual else (N + M)) * k
    idx = torch.empty(max(cap, 1), 3, dtype=torch.int64, device=dev)
    sc = torch.empty(max(cap, 1), device=dev)
    tot = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _lib.dr_mutual_topk_workspace_bytes(B, N, M)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    check(_lib.dr_mutual_topk_select_f32(B, N, M, ptr(s), int(k), 1 if largest else 0, 0 if threshold is None else 1,
                                         0.0 if threshold is None else float(threshold), 1 if mutual else 0, ptr(mask_u8(row_masks)),
                                         ptr(mask_u8(col_masks)), ptr(idx), ptr(sc), cap, ptr(tot), ptr(ws), wsb, stream_of(s)))
    n = int(tot.item())
    assert n <= cap
    idx, sc = idx[:n], sc[:n]
    if two_d:
        return idx[:, 1], idx[:, 2], sc
    return idx[:, 0], idx[:, 1], idx[:, 2], sc


def pnp_ransac(points, pixels, intrinsics, num_iterations=50000, distance_tolerance=8.0, seed=0, transposed=True):
    """PnP-RANSAC on device tensors -> dict(transform [4,4] float64 device, n_inlier, best_iter) (None with fewer than 4 correspondences)"""
    ensure_init()
    n = points.shape[0]
    if n < 4:
        return None
    points, pixels = points.contiguous().float(), pixels.contiguous().float()
    K = (ctypes.c_double * 9)(*[float(x) for x in torch.as_tensor(intrinsics, dtype=torch.float64).reshape(-1).tolist()])
    T = torch.empty(4, 4, dtype=torch.float64, device=points.device)
    ni = torch.zeros(1, dtype=torch.int32, device=points.device)
    bi = torch.zeros(1, dtype=torch.int32, device=points.device)
    wsb = _lib.dr_pnp_ransac_workspace_bytes(n, int(num_iterations))
    ws = torch.empty(wsb, dtype=torch.uint8, device=points.device)
    check(_lib.dr_pnp_ransac_f64(n, ptr(points), ptr(pixels), 1 if transposed else 0, K, int(num_iterations), float(distance_tolerance), int(seed), ptr(T),
                                 ptr(ni), ptr(bi), ptr(ws), wsb, stream_of(points)))
    return dict(transform=T, n_inlier=ni, best_iter=bi)


def patch_similarity(img_feats, img_knn_indices, pcd_feats, pcd_knn_indices):
    """[P,Ki,Kc] similarity of the image / point patches of P node correspondences (EXP/model.py:726-738); an index equal to
    pcd_feats.shape[0] addresses the zero row the reference appends"""
    ensure_init()
    img_feats, pcd_feats = img_feats.contiguous().float(), pcd_feats.contiguous().float()
    ii, pj = img_knn_indices.to(torch.int64).contiguous(), pcd_knn_indices.to(torch.int64).contiguous()
    P, Ki = ii.shape
    Kc = pj.shape[1]
    out = torch.empty(P, Ki, Kc, device=img_feats.device)
    check(_lib.dr_patch_similarity_f32(P, Ki, Kc, img_feats.shape[1], ptr(img_feats), ptr(ii), ptr(pcd_feats), ptr(pj), pcd_feats.shape[0], ptr(out),
                                       stream_of(out)))
    return out


def unique_pairs(first, second, multiplier):
    """sorted distinct first * multiplier + second (torch.unique of EXP/model.py:760-761) -> (keys [n] int64, count [1] int32) without a host sync"""
    ensure_init()
    a, b = first.to(torch.int64).contiguous(), second.to(torch.int64).contiguous()
    n = a.numel()
    keys = torch.empty(max(n, 1), dtype=torch.int64, device=a.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=a.device)
    wsb = _lib.dr_unique_pairs_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=a.device)
    check(_lib.dr_unique_pairs_i64(n, ptr(a), ptr(b), int(multiplier), ptr(keys), ptr(cnt), ptr(ws), wsb, stream_of(a)))
    return keys, cnt


def corr_gather(keys, count, num_points_f, img_points_f, img_pixels_f, pcd_points_f, pcd_pixels_f, img_feats_f, pcd_feats_f):
    """EXP/model.py:761-774 -> dict with the reference's output names (one host read of the count to size the views)"""
    ensure_init()
    f = lambda x, w: x.contiguous().float().view(-1, w)
    ip, ix, pp, px = f(img_points_f, 3), f(img_pixels_f, 2), f(pcd_points_f, 3), f(pcd_pixels_f, 2)
    fi, fp = img_feats_f.contiguous().float(), pcd_feats_f.contiguous().float()
    cap = keys.numel()
    dev = keys.device
    o = dict(img_corr_indices=torch.empty(cap, dtype=torch.int64, device=dev), pcd_corr_indices=torch.empty(cap, dtype=torch.int64, device=dev),
             img_corr_points=torch.empty(cap, 3, device=dev), img_corr_pixels=torch.empty(cap, 2, device=dev),
             pcd_corr_points=torch.empty(cap, 3, device=dev), pcd_corr_pixels=torch.empty(cap, 2, device=dev), corr_scores=torch.empty(cap, device=dev))
    check(_lib.dr_corr_gather_f32(cap, ptr(count), ptr(keys), int(num_points_f), fi.shape[1], ptr(ip), ptr(ix), ptr(pp), ptr(px), ptr(fi), ptr(fp),
                                  ptr(o["img_corr_indices"]), ptr(o["pcd_corr_indices"]), ptr(o["img_corr_points"]), ptr(o["img_corr_pixels"]),
                                  ptr(o["pcd_corr_points"]), ptr(o["pcd_corr_pixels"]), ptr(o["corr_scores"]), stream_of(keys)))
    n = int(count.item())
    return {k: v[:n] for k, v in o.items()}


PROF_KINDS = ("gemm", "attention", "layernorm", "position_code", "sinkhorn", "procrustes", "state", "gemm_split")


def prof_enable(on=True):
    _lib.dr_prof_enable(1 if on else 0)


def prof_collect():
    """-> {family: (calls, total_ms, work)}; synchronises the device."""
    n = len(PROF_KINDS)
    calls = (ctypes.c_int * n)(); ms = (ctypes.c_double * n)(); work = (ctypes.c_double * n)()
    check(_lib.dr_prof_collect(calls, ms, work))
    return {k: (calls[i], ms[i], work[i]) for i, k in enumerate(PROF_KINDS)}
