"""Loader and ctypes bindings for ``libpointnet_refine_hip.so`` (C ABI declared in
``include/pointnet_refine_hip.h``).

The product path has NO CPU fallback: ``lib()`` raises if the library is missing, and
every op in ``ops.py`` raises on non-GPU tensors.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
# PRH_LIB_PATH: load an alternative build of the same library (kernel-tuning experiments)
LIB_PATH = os.environ.get("PRH_LIB_PATH") or os.path.join(_HERE, "libpointnet_refine_hip.so")
_CSRC = os.path.join(_HERE, "csrc")
# every file of csrc/ counts for staleness (prh_lib.hip is the one translation unit; it includes the rest)
_SOURCES = [os.path.join(_CSRC, "prh_lib.hip")] + (sorted(
    os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hpp", ".h", ".hip")) and f != "prh_lib.hip")
    if os.path.isdir(_CSRC) else [])      # a binary-only install has no csrc/: nothing can be stale
_HEADER = os.path.join(_ROOT, "include", "pointnet_refine_hip.h")

PRH_MAX_LAYERS = 8


class BnLayer(C.Structure):
    _fields_ = [("w", C.c_void_p), ("b", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("num_batches_tracked", C.c_void_p), ("cin", C.c_int), ("cout", C.c_int)]


class BnLayerGrad(C.Structure):
    _fields_ = [("dw", C.c_void_p), ("db", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p)]


class EncoderParams(C.Structure):
    _fields_ = [("in_channel", C.c_int), ("out_dim", C.c_int), ("conv", BnLayer * 5),
                ("fusion", BnLayer), ("gate_w1", C.c_void_p), ("gate_b1", C.c_void_p),
                ("gate_w2", C.c_void_p), ("gate_b2", C.c_void_p)]


class EncoderGrads(C.Structure):
    _fields_ = [("conv", BnLayerGrad * 5), ("fusion", BnLayerGrad), ("d_gate_w1", C.c_void_p),
                ("d_gate_b1", C.c_void_p), ("d_gate_w2", C.c_void_p), ("d_gate_b2", C.c_void_p)]


class EncoderSaved(C.Structure):
    _fields_ = [("z_cat", C.c_void_p), ("z_fus", C.c_void_p), ("gate", C.c_void_p),
                ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("bn_mean", C.c_void_p),
                ("bn_rstd", C.c_void_p), ("argmax", C.c_void_p), ("op_amax", C.c_void_p),
                ("gate_recompute", C.c_int)]      # trailing, 0 by default: the stored-gate backward


class EncoderSavedBf16(C.Structure):
    _fields_ = [("z_cat", C.c_void_p), ("z_fus", C.c_void_p), ("gate", C.c_void_p),
                ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("bn_mean", C.c_void_p),
                ("bn_rstd", C.c_void_p), ("argmax", C.c_void_p)]


EXPORTS = [
    "prh_encoder_workspace_bytes", "prh_encoder_gate_recompute", "prh_encoder_forward", "prh_encoder_backward",
    "prh_encoder_bf16_workspace_bytes", "prh_encoder_forward_bf16", "prh_encoder_backward_bf16",
    "prh_linear_bf16_workspace_bytes", "prh_linear_forward_bf16", "prh_linear_backward_bf16",
    "prh_linear_forward_out16", "prh_linear_backward_dy16", "prh_attn_forward_kv16", "prh_attn_backward_kv16",
    "prh_encoder_fused_image_bytes", "prh_encoder_fused_prepare", "prh_encoder_fused_workspace_bytes",
    "prh_encoder_fused_forward",
    "prh_linear_forward_workspace_bytes", "prh_linear_forward", "prh_linear_forward_ex",
    "prh_linear_forward_full", "prh_linear_forward_amax", "prh_operand_absmax_workspace_bytes", "prh_operand_absmax",
    "prh_linear_uses_operand_maxima", "prh_linear_backward_full", "prh_linear_backward_amax", "prh_pos_hidden_forward",
    "prh_pos_hidden_forward_workspace_bytes", "prh_pos_hidden_forward_amax", "prh_pos_hidden_backward_workspace_bytes",
    "prh_pos_hidden_backward", "prh_linear_small_forward", "prh_linear_small_backward_workspace_bytes",
    "prh_linear_small_backward",
    "prh_linear_backward_workspace_bytes", "prh_linear_backward", "prh_linear_backward_ex",
    "prh_mlp_stack_workspace_bytes", "prh_mlp_stack_forward", "prh_mlp_stack_backward",
    "prh_test_gemm_nt", "prh_test_gemm_tn_workspace_bytes", "prh_test_gemm_tn",
    "prh_test_gate_backward_workspace_bytes", "prh_test_gate_backward",
    "prh_test_gemm_tn_side_workspace_bytes", "prh_test_gemm_tn_side", "prh_test_gemm_tn_side_ex", "prh_test_xcc_map",
    "prh_test_reduce_depth", "prh_test_reduce_slabs", "prh_test_reduce_bn_stage1", "prh_test_reduce_partials",
    "prh_test_reduce_ln_param_grad", "prh_test_reduce_pos_hidden_final", "prh_test_reduce_partial_rows_final",
    "prh_test_reduce_act_amax_workspace_bytes", "prh_test_reduce_act_amax",
    "prh_profile_enable", "prh_profile_count", "prh_profile_reset", "prh_profile_read",
    "prh_attn_forward", "prh_attn_backward", "prh_attn_backward_ex",
    "prh_context_workspace_bytes", "prh_context_build",
    "prh_context_ragged_workspace_bytes", "prh_context_ragged_count", "prh_context_ragged_select",
    "prh_line_metrics", "prh_shift_sweep_workspace_bytes", "prh_shift_sweep",
    "prh_shift_sweep_ragged_workspace_bytes", "prh_shift_sweep_ragged",
    "prh_drive_slice_workspace_bytes", "prh_drive_slice_count", "prh_drive_slice_write",
    "prh_drive_clip_workspace_bytes", "prh_drive_clip_count", "prh_drive_clip_write",
    "prh_drive_noise_workspace_bytes", "prh_drive_noise",
    "prh_match_clip_workspace_bytes", "prh_match_clip_count", "prh_match_clip_write",
    "prh_match_costs_workspace_bytes", "prh_match_costs", "prh_match_max_side", "prh_match_assign",
    "prh_bev_bounds_workspace_bytes", "prh_bev_bounds", "prh_bev_raster", "prh_bev_select_workspace_bytes",
    "prh_bev_select", "prh_bev_tone", "prh_bev_colorize", "prh_bev_crop", "prh_bev_tile", "prh_bev_draw_count",
    "prh_bev_draw_workspace_bytes", "prh_bev_draw",
    "prh_view_bounds_workspace_bytes", "prh_view_bounds", "prh_view_clear", "prh_view_max_views", "prh_view_splat",
    "prh_view_lines", "prh_view_resolve",
    "prh_fuse_max_points", "prh_fuse_tile", "prh_fuse_project_workspace_bytes", "prh_fuse_project",
    "prh_fuse_gather_workspace_bytes", "prh_fuse_gather",
    "prh_link_tile", "prh_link_pairs_per_block", "prh_link_pairs_workspace_bytes", "prh_link_pairs_count",
    "prh_link_pairs_write", "prh_link_stats",
    "prh_link_cum", "prh_link_edges_blocks", "prh_link_edges", "prh_link_edges_compact", "prh_link_label_round",
    "prh_link_tree_init", "prh_link_tree_level",
    "prh_support_max_cells", "prh_support_accumulate",
    "prh_ground_max_bins", "prh_ground_bin_workspace_bytes", "prh_ground_bin_count", "prh_ground_bin_write",
    "prh_ground_query",
    "prh_align_tile", "prh_align_max_shifts", "prh_align_select_workspace_bytes", "prh_align_select_count",
    "prh_align_select_write", "prh_align_score",
    "prh_align_max_poses", "prh_align_select_cells_workspace_bytes", "prh_align_select_cells_count",
    "prh_align_select_cells_write", "prh_align_score_rigid",
    "prh_trace_max_nms", "prh_trace_workspace_bytes", "prh_trace_hist", "prh_trace_hist_surface", "prh_trace_peaks_count",
    "prh_trace_peaks_write", "prh_trace_link",
    "prh_floor_max_bins", "prh_floor_hist", "prh_test_floor_hist", "prh_floor_otsu",
    "prh_pcd_group_rows", "prh_pcd_format_workspace_bytes", "prh_pcd_format_count", "prh_pcd_format_write",
    "prh_pcd_index_blocks", "prh_pcd_index_count", "prh_pcd_index_write", "prh_pcd_parse_workspace_bytes",
    "prh_pcd_parse", "prh_pcd_unpack14",
    "prh_l1_loss_workspace_bytes", "prh_l1_loss", "prh_adam_step",
    "prh_add_dropout_layernorm_forward", "prh_add_dropout_layernorm_workspace_bytes",
    "prh_add_dropout_layernorm_backward",
    "prh_relu_mask_absmax", "prh_cast_perm_bf16", "prh_posmem_images", "prh_attn_fold_forward", "prh_set_gemm_mode", "prh_get_gemm_mode", "prh_set_dropout_seed_source",
    "prh_last_error", "prh_version",
]

_lock = threading.Lock()
_lib = None


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in _SOURCES + [_HEADER])


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree with hipcc (cross-compiles without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
           "-o", LIB_PATH, _SOURCES[0]]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


def _bind(lib):
    vp, i, f, sz, lg = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_long
    lib.prh_last_error.restype = C.c_char_p
    lib.prh_version.restype = C.c_char_p
    lib.prh_encoder_workspace_bytes.restype = sz
    lib.prh_encoder_workspace_bytes.argtypes = [i, i, i, i, i]
    lib.prh_encoder_gate_recompute.restype = i
    lib.prh_encoder_gate_recompute.argtypes = [i, i, i, i, i]
    lib.prh_encoder_forward.restype = i
    lib.prh_encoder_forward.argtypes = [C.POINTER(EncoderParams), vp, i, i, i, f, f, vp, vp,
                                        C.POINTER(EncoderSaved), vp, sz, i, vp]
    lib.prh_encoder_backward.restype = i
    lib.prh_encoder_backward.argtypes = [C.POINTER(EncoderParams), vp, i, i, i, vp, vp, i,
                                         C.POINTER(EncoderSaved), C.POINTER(EncoderGrads), vp, vp,
                                         sz, i, vp]
    lib.prh_encoder_bf16_workspace_bytes.restype = sz
    lib.prh_encoder_bf16_workspace_bytes.argtypes = [i, i, i, i, i]
    lib.prh_encoder_forward_bf16.restype = i
    lib.prh_encoder_forward_bf16.argtypes = [C.POINTER(EncoderParams), vp, i, i, i, f, f, vp, vp,
                                             C.POINTER(EncoderSavedBf16), vp, sz, i, vp]
    lib.prh_encoder_backward_bf16.restype = i
    lib.prh_encoder_backward_bf16.argtypes = [C.POINTER(EncoderParams), vp, i, i, i, vp, vp,
                                              C.POINTER(EncoderSavedBf16), C.POINTER(EncoderGrads), vp, vp,
                                              sz, i, vp]
    lib.prh_linear_bf16_workspace_bytes.restype = sz
    lib.prh_linear_bf16_workspace_bytes.argtypes = [i, i, i, i]
    lib.prh_linear_forward_bf16.restype = i
    lib.prh_linear_forward_bf16.argtypes = [vp, lg, vp, vp, vp, i, i, i, i, vp, sz, i, vp]
    lib.prh_linear_backward_bf16.restype = i
    lib.prh_linear_backward_bf16.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_linear_forward_out16.restype = i
    lib.prh_linear_forward_out16.argtypes = [vp, lg, vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_linear_backward_dy16.restype = i
    lib.prh_linear_backward_dy16.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_attn_forward_kv16.restype = i
    lib.prh_attn_forward_kv16.argtypes = [vp, lg, vp, lg, vp, lg, vp, lg, vp, i, i, i, i, f, f, C.c_uint, i, vp]
    lib.prh_attn_backward_kv16.restype = i
    lib.prh_attn_backward_kv16.argtypes = [vp, lg, vp, lg, vp, lg, vp, lg, vp, vp, lg, vp, lg, vp, lg, vp, lg,
                                           i, i, i, i, f, f, C.c_uint, i, vp]
    lib.prh_encoder_fused_image_bytes.restype = sz
    lib.prh_encoder_fused_image_bytes.argtypes = [i, i]
    lib.prh_encoder_fused_prepare.restype = i
    lib.prh_encoder_fused_prepare.argtypes = [C.POINTER(EncoderParams), f, vp, vp, i, vp, sz, i, vp]
    lib.prh_encoder_fused_workspace_bytes.restype = sz
    lib.prh_encoder_fused_workspace_bytes.argtypes = [i, i, i]
    lib.prh_encoder_fused_forward.restype = i
    lib.prh_encoder_fused_forward.argtypes = [vp, i, i, i, vp, i, i, vp, vp, vp, vp, vp, sz, i, vp]
    lib.prh_linear_forward.restype = i
    lib.prh_linear_forward.argtypes = [vp, lg, vp, vp, vp, i, i, i, i, vp, sz, i, vp]
    lib.prh_linear_forward_ex.restype = i
    lib.prh_linear_forward_ex.argtypes = [vp, lg, vp, vp, vp, i, i, i, i, vp, vp, sz, i, vp]
    lib.prh_linear_forward_full.restype = i
    lib.prh_linear_forward_full.argtypes = [vp, lg, vp, vp, vp, lg, vp, i, i, i, i, vp, vp, f, C.c_uint, vp, sz, i, vp]
    lib.prh_linear_forward_amax.restype = i
    lib.prh_linear_forward_amax.argtypes = [vp, lg, vp, vp, vp, lg, vp, i, i, i, i, vp, vp, f, C.c_uint, vp, vp, sz, i, vp]
    lib.prh_linear_backward_amax.restype = i
    lib.prh_linear_backward_amax.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, i, vp, vp, sz, i, vp]
    lib.prh_pos_hidden_forward_workspace_bytes.restype = sz
    lib.prh_pos_hidden_forward_workspace_bytes.argtypes = []
    lib.prh_pos_hidden_forward_amax.restype = i
    lib.prh_pos_hidden_forward_amax.argtypes = [vp, lg, vp, vp, vp, lg, i, vp, vp, sz, i, vp]
    lib.prh_operand_absmax_workspace_bytes.restype = sz
    lib.prh_operand_absmax_workspace_bytes.argtypes = []
    lib.prh_operand_absmax.restype = i
    lib.prh_operand_absmax.argtypes = [vp, lg, lg, i, vp, vp, sz, i, vp]
    lib.prh_linear_uses_operand_maxima.restype = i
    lib.prh_linear_uses_operand_maxima.argtypes = [i, i, i]
    lib.prh_linear_backward_full.restype = i
    lib.prh_linear_backward_full.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, i, vp]
    lib.prh_pos_hidden_forward.restype = i
    lib.prh_pos_hidden_forward.argtypes = [vp, lg, vp, vp, vp, lg, i, i, vp]
    lib.prh_pos_hidden_backward_workspace_bytes.restype = sz
    lib.prh_pos_hidden_backward_workspace_bytes.argtypes = [lg, i]
    lib.prh_pos_hidden_backward.restype = i
    lib.prh_pos_hidden_backward.argtypes = [vp, lg, vp, vp, vp, vp, vp, vp, lg, i, vp, sz, i, vp]
    lib.prh_linear_small_forward.restype = i
    lib.prh_linear_small_forward.argtypes = [vp, vp, vp, vp, lg, i, i, i, vp]
    lib.prh_linear_small_backward_workspace_bytes.restype = sz
    lib.prh_linear_small_backward_workspace_bytes.argtypes = [lg, i, i]
    lib.prh_linear_small_backward.restype = i
    lib.prh_linear_small_backward.argtypes = [vp, vp, vp, vp, vp, vp, lg, i, i, vp, sz, i, vp]
    lib.prh_linear_backward_ex.restype = i
    lib.prh_linear_backward_ex.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, sz, i, vp]
    lib.prh_linear_forward_workspace_bytes.restype = sz
    lib.prh_linear_forward_workspace_bytes.argtypes = [i, i, i]
    lib.prh_linear_backward_workspace_bytes.restype = sz
    lib.prh_linear_backward_workspace_bytes.argtypes = [i, i, i]
    lib.prh_linear_backward.restype = i
    lib.prh_linear_backward.argtypes = [vp, lg, vp, vp, vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_mlp_stack_workspace_bytes.restype = sz
    lib.prh_mlp_stack_workspace_bytes.argtypes = [i, i, C.POINTER(BnLayer)]
    lib.prh_mlp_stack_forward.restype = i
    lib.prh_mlp_stack_forward.argtypes = [C.POINTER(BnLayer), i, i, vp, i, i, f, f, vp, vp, vp, vp,
                                          vp, vp, vp, sz, i, vp]
    lib.prh_mlp_stack_backward.restype = i
    lib.prh_mlp_stack_backward.argtypes = [C.POINTER(BnLayer), i, i, vp, i, i, vp, vp, vp, vp, vp,
                                           vp, C.POINTER(BnLayerGrad), vp, vp, sz, i, vp]
    lib.prh_attn_forward.restype = i
    lib.prh_attn_forward.argtypes = [vp, lg, vp, lg, vp, lg, vp, lg, vp, i, i, i, i, f, f, C.c_uint, i, vp]
    lib.prh_attn_backward.restype = i
    lib.prh_attn_backward.argtypes = [vp, lg, vp, lg, vp, lg, vp, lg, vp, vp, lg, vp, lg, vp, lg, vp, lg,
                                      i, i, i, i, f, f, C.c_uint, i, vp]
    lib.prh_context_workspace_bytes.restype = C.c_size_t
    lib.prh_context_workspace_bytes.argtypes = [i, i, i]
    lib.prh_context_build.restype = i
    lib.prh_context_build.argtypes = [vp, i, vp, i, vp, i, i, f, f, i, i, C.c_ulonglong, vp, vp, vp, vp,
                                      C.c_size_t, i, vp]
    lib.prh_context_ragged_workspace_bytes.restype = sz
    lib.prh_context_ragged_workspace_bytes.argtypes = [i, C.c_longlong]
    lib.prh_context_ragged_count.restype = i
    lib.prh_context_ragged_count.argtypes = [vp, vp, i, vp, i, vp, vp, i, f, vp, vp, vp, sz, i, vp]
    lib.prh_context_ragged_select.restype = i
    lib.prh_context_ragged_select.argtypes = [vp, vp, i, vp, i, vp, i, vp, i, f, f, i, vp, vp, i, i, vp, vp,
                                              C.c_longlong, vp, vp, sz, i, vp]
    lib.prh_line_metrics.restype = i
    lib.prh_line_metrics.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, vp, vp, i, vp]
    lib.prh_shift_sweep_workspace_bytes.restype = sz
    lib.prh_shift_sweep_workspace_bytes.argtypes = [i, i, i]
    lib.prh_shift_sweep.restype = i
    lib.prh_shift_sweep.argtypes = [vp, i, vp, i, vp, i, vp, vp, sz, i, vp]
    lib.prh_shift_sweep_ragged_workspace_bytes.restype = sz
    lib.prh_shift_sweep_ragged_workspace_bytes.argtypes = [vp, vp, i]
    lib.prh_shift_sweep_ragged.restype = i
    lib.prh_shift_sweep_ragged.argtypes = [vp, vp, vp, vp, i, vp, vp, vp, i, vp, vp, sz, i, vp]
    ll, dbl = C.c_longlong, C.c_double
    lib.prh_drive_slice_workspace_bytes.restype = sz
    lib.prh_drive_slice_workspace_bytes.argtypes = [i, i]
    lib.prh_drive_slice_count.restype = i
    lib.prh_drive_slice_count.argtypes = [vp, i, vp, i, dbl, dbl, vp, vp, sz, i, vp]
    lib.prh_drive_slice_write.restype = i
    lib.prh_drive_slice_write.argtypes = [vp, i, vp, i, dbl, dbl, vp, vp, vp, ll, vp, sz, i, vp]
    lib.prh_drive_clip_workspace_bytes.restype = sz
    lib.prh_drive_clip_workspace_bytes.argtypes = [i]
    lib.prh_drive_clip_count.restype = i
    lib.prh_drive_clip_count.argtypes = [vp, vp, i, vp, i, dbl, vp, vp, sz, i, vp]
    lib.prh_drive_clip_write.restype = i
    lib.prh_drive_clip_write.argtypes = [vp, vp, i, vp, i, dbl, vp, vp, vp, sz, i, vp]
    lib.prh_drive_noise_workspace_bytes.restype = sz
    lib.prh_drive_noise_workspace_bytes.argtypes = [i]
    lib.prh_drive_noise.restype = i
    lib.prh_drive_noise.argtypes = [vp, vp, vp, ll, i, vp, C.POINTER(dbl), i, C.c_ulonglong, i, vp, vp, vp, vp, sz,
                                    i, vp]
    lib.prh_match_clip_workspace_bytes.restype = sz
    lib.prh_match_clip_workspace_bytes.argtypes = [i]
    lib.prh_match_clip_count.restype = i
    lib.prh_match_clip_count.argtypes = [vp, vp, i, vp, i, dbl, vp, vp, sz, i, vp]
    lib.prh_match_clip_write.restype = i
    lib.prh_match_clip_write.argtypes = [vp, vp, i, vp, i, dbl, vp, vp, vp, sz, i, vp]
    lib.prh_match_costs_workspace_bytes.restype = sz
    lib.prh_match_costs_workspace_bytes.argtypes = [ll]
    lib.prh_match_costs.restype = i
    lib.prh_match_costs.argtypes = [vp, vp, vp, ll, vp, vp, vp, i, vp, vp, vp, sz, i, vp]
    lib.prh_match_max_side.restype = i
    lib.prh_match_max_side.argtypes = []
    lib.prh_match_assign.restype = i
    lib.prh_match_assign.argtypes = [vp, vp, vp, vp, vp, i, ll, dbl, i, vp, vp, vp, vp, vp, i, vp]
    lib.prh_bev_bounds_workspace_bytes.restype = sz
    lib.prh_bev_bounds_workspace_bytes.argtypes = []
    lib.prh_bev_bounds.restype = i
    lib.prh_bev_bounds.argtypes = [vp, ll, i, vp, vp, sz, i, vp]
    lib.prh_bev_raster.restype = i
    lib.prh_bev_raster.argtypes = [vp, vp, i, ll, i, dbl, dbl, dbl, i, i, vp, vp, i, vp]
    lib.prh_bev_select_workspace_bytes.restype = sz
    lib.prh_bev_select_workspace_bytes.argtypes = [i]
    lib.prh_bev_select.restype = i
    lib.prh_bev_select.argtypes = [vp, i, ll, f, vp, vp, sz, i, vp]
    lib.prh_bev_tone.restype = i
    lib.prh_bev_tone.argtypes = [vp, i, ll, vp, f, vp, i, vp]
    lib.prh_bev_colorize.restype = i
    lib.prh_bev_colorize.argtypes = [vp, vp, ll, vp, vp, i, vp]
    lib.prh_bev_crop.restype = i
    lib.prh_bev_crop.argtypes = [vp, i, i, vp, vp, i, ll, vp, i, vp]
    lib.prh_bev_tile.restype = i
    lib.prh_bev_tile.argtypes = []
    lib.prh_bev_draw_count.restype = i
    lib.prh_bev_draw_count.argtypes = [vp, vp, i, vp, vp, vp, vp, ll, vp, i, vp]
    lib.prh_bev_draw_workspace_bytes.restype = sz
    lib.prh_bev_draw_workspace_bytes.argtypes = [ll, ll]
    lib.prh_bev_draw.restype = i
    lib.prh_bev_draw.argtypes = [vp, vp, i, vp, vp, vp, vp, vp, vp, vp, ll, ll, vp, vp, sz, i, vp]
    lib.prh_view_bounds_workspace_bytes.restype = sz
    lib.prh_view_bounds_workspace_bytes.argtypes = []
    lib.prh_view_bounds.restype = i
    lib.prh_view_bounds.argtypes = [vp, ll, i, vp, vp, sz, i, vp]
    lib.prh_view_clear.restype = i
    lib.prh_view_clear.argtypes = [vp, i, i, i, i, vp]
    lib.prh_view_max_views.restype = i
    lib.prh_view_max_views.argtypes = []
    lib.prh_view_splat.restype = i
    lib.prh_view_splat.argtypes = [vp, ll, i, vp, i, vp, i, vp, i, dbl, dbl, i, i, vp, vp, i, vp]
    lib.prh_view_lines.restype = i
    lib.prh_view_lines.argtypes = [vp, vp, i, vp, i, vp, i, i, i, vp, i, vp]
    lib.prh_view_resolve.restype = i
    lib.prh_view_resolve.argtypes = [vp, ll, vp, vp, i, C.c_uint, vp, vp, i, vp]
    lib.prh_fuse_max_points.restype = i
    lib.prh_fuse_max_points.argtypes = []
    lib.prh_fuse_tile.restype = i
    lib.prh_fuse_tile.argtypes = []
    lib.prh_fuse_project_workspace_bytes.restype = sz
    lib.prh_fuse_project_workspace_bytes.argtypes = [i]
    lib.prh_fuse_project.restype = i
    lib.prh_fuse_project.argtypes = [vp, ll, i, vp, vp, vp, i, vp, vp, vp, i, vp, vp, vp, vp, vp, sz, i, vp]
    lib.prh_fuse_gather_workspace_bytes.restype = sz
    lib.prh_fuse_gather_workspace_bytes.argtypes = [ll]
    lib.prh_fuse_gather.restype = i
    lib.prh_fuse_gather.argtypes = [vp, vp, ll, i, vp, i, vp, ll, dbl, vp, vp, vp, vp, vp, sz, i, vp]
    lib.prh_link_tile.restype = i
    lib.prh_link_tile.argtypes = []
    lib.prh_link_pairs_per_block.restype = i
    lib.prh_link_pairs_per_block.argtypes = []
    lib.prh_link_pairs_workspace_bytes.restype = sz
    lib.prh_link_pairs_workspace_bytes.argtypes = [ll]
    lib.prh_link_pairs_count.restype = i
    lib.prh_link_pairs_count.argtypes = [vp, ll, i, vp, dbl, vp, vp, sz, i, vp]
    lib.prh_link_pairs_write.restype = i
    lib.prh_link_pairs_write.argtypes = [vp, ll, i, vp, dbl, vp, vp, vp, sz, i, vp]
    lib.prh_link_stats.restype = i
    lib.prh_link_stats.argtypes = [vp, vp, ll, i, vp, vp, ll, dbl, vp, vp, i, vp]
    lib.prh_link_cum.restype = i
    lib.prh_link_cum.argtypes = [vp, ll, i, vp, i, vp]
    lib.prh_link_edges_blocks.restype = ll
    lib.prh_link_edges_blocks.argtypes = [ll]
    lib.prh_link_edges.restype = i
    lib.prh_link_edges.argtypes = [vp, ll, vp, vp, ll, ll, ll, vp, vp, vp, vp, vp, i, vp]
    lib.prh_link_edges_compact.restype = i
    lib.prh_link_edges_compact.argtypes = [vp, vp, vp, vp, vp, vp, ll, vp, ll, vp, vp, vp, i, vp]
    lib.prh_link_label_round.restype = i
    lib.prh_link_label_round.argtypes = [vp, ll, ll, vp, vp, i, vp]
    lib.prh_link_tree_init.restype = i
    lib.prh_link_tree_init.argtypes = [vp, ll, vp, vp, vp, vp, vp, i, vp]
    lib.prh_link_tree_level.restype = i
    lib.prh_link_tree_level.argtypes = [vp, vp, vp, ll, ll, i, vp, vp, vp, vp, vp, vp, i, vp]
    lib.prh_support_max_cells.restype = i
    lib.prh_support_max_cells.argtypes = []
    lib.prh_support_accumulate.restype = i
    lib.prh_support_accumulate.argtypes = [vp, ll, dbl, dbl, dbl, dbl, dbl, dbl, i, i, vp, vp, ll, vp, vp, vp, i, vp, ll,
                                           dbl, dbl, dbl, vp, i, vp]
    lib.prh_pcd_group_rows.restype = i
    lib.prh_pcd_group_rows.argtypes = []
    lib.prh_pcd_format_workspace_bytes.restype = sz
    lib.prh_pcd_format_workspace_bytes.argtypes = [ll]
    lib.prh_pcd_format_count.restype = i
    lib.prh_pcd_format_count.argtypes = [vp, i, ll, vp, vp, vp, vp, sz, i, vp]
    lib.prh_pcd_format_write.restype = i
    lib.prh_pcd_format_write.argtypes = [vp, i, ll, vp, vp, vp, i, vp, ll, vp, i, vp]
    lib.prh_pcd_index_blocks.restype = ll
    lib.prh_pcd_index_blocks.argtypes = [vp, ll]
    lib.prh_pcd_index_count.restype = i
    lib.prh_pcd_index_count.argtypes = [vp, ll, vp, i, vp]
    lib.prh_pcd_index_write.restype = i
    lib.prh_pcd_index_write.argtypes = [vp, ll, vp, vp, ll, i, vp]
    lib.prh_pcd_parse_workspace_bytes.restype = sz
    lib.prh_pcd_parse_workspace_bytes.argtypes = [ll]
    lib.prh_pcd_parse.restype = i
    lib.prh_pcd_parse.argtypes = [vp, ll, vp, ll, i, vp, vp, vp, sz, i, vp]
    lib.prh_pcd_unpack14.restype = i
    lib.prh_pcd_unpack14.argtypes = [vp, ll, vp, i, vp]
    lib.prh_add_dropout_layernorm_forward.restype = i
    lib.prh_add_dropout_layernorm_forward.argtypes = [vp, vp, vp, vp, lg, i, f, f, C.c_uint, vp, vp, vp, i, vp]
    lib.prh_add_dropout_layernorm_workspace_bytes.restype = C.c_size_t
    lib.prh_add_dropout_layernorm_workspace_bytes.argtypes = []
    lib.prh_add_dropout_layernorm_backward.restype = i
    lib.prh_add_dropout_layernorm_backward.argtypes = [vp, vp, vp, vp, vp, vp, lg, i, f, C.c_uint, vp, vp, vp, vp,
                                                       vp, C.c_size_t, i, vp]
    lib.prh_l1_loss_workspace_bytes.restype = C.c_size_t
    lib.prh_l1_loss_workspace_bytes.argtypes = []
    lib.prh_l1_loss.restype = i
    lib.prh_l1_loss.argtypes = [vp, vp, i, lg, C.c_double, i, vp, vp, vp, C.c_double, vp, C.c_size_t, i, vp]
    lib.prh_adam_step.restype = i
    lib.prh_adam_step.argtypes = [vp, vp, vp, vp, lg, f, f, f, f, f, i, i, vp]
    lib.prh_cast_perm_bf16.restype = i
    lib.prh_cast_perm_bf16.argtypes = [vp, lg, vp, lg, i, vp]
    lib.prh_posmem_images.restype = i
    lib.prh_posmem_images.argtypes = [vp, lg, vp, vp, vp, vp, vp, lg, lg, vp, vp, i, vp]
    lib.prh_attn_fold_forward.restype = i
    lib.prh_attn_fold_forward.argtypes = [vp, lg, vp, vp, vp, lg, vp, lg, vp, vp, lg, i, i, i, i, C.c_float, i, vp]
    lib.prh_relu_mask_absmax.restype = i
    lib.prh_relu_mask_absmax.argtypes = [vp, vp, vp, lg, f, vp, vp, sz, i, vp]
    lib.prh_set_gemm_mode.restype = i
    lib.prh_set_gemm_mode.argtypes = [i]
    lib.prh_attn_backward_ex.restype = i
    lib.prh_attn_backward_ex.argtypes = [vp, lg, vp, lg, vp, lg, vp, lg, vp, vp, lg, vp, lg, vp, lg, vp, lg,
                                         i, i, i, i, f, f, C.c_uint, vp, i, vp]
    lib.prh_set_dropout_seed_source.restype = i
    lib.prh_set_dropout_seed_source.argtypes = [vp]
    lib.prh_get_gemm_mode.restype = i
    lib.prh_profile_enable.restype = i
    lib.prh_profile_enable.argtypes = [i]
    lib.prh_profile_count.restype = i
    lib.prh_profile_reset.restype = i
    lib.prh_profile_read.restype = i
    lib.prh_profile_read.argtypes = [i, C.c_char_p, i, C.POINTER(C.c_float), C.POINTER(C.c_double),
                                     C.POINTER(C.c_double)]
    lib.prh_test_gemm_nt.restype = i
    lib.prh_test_gemm_nt.argtypes = [vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_test_gate_backward_workspace_bytes.restype = sz
    lib.prh_test_gate_backward_workspace_bytes.argtypes = [i]
    lib.prh_test_gate_backward.restype = i
    lib.prh_test_gate_backward.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, sz, i, vp]
    lib.prh_test_gemm_tn_workspace_bytes.restype = sz
    lib.prh_test_gemm_tn_workspace_bytes.argtypes = [i, i, i]
    lib.prh_test_gemm_tn.restype = i
    lib.prh_test_gemm_tn.argtypes = [vp, vp, vp, vp, i, i, i, vp, sz, i, vp]
    lib.prh_test_gemm_tn_side_workspace_bytes.restype = sz
    lib.prh_test_gemm_tn_side_workspace_bytes.argtypes = [i, i, i]
    lib.prh_test_gemm_tn_side.restype = i
    lib.prh_test_gemm_tn_side.argtypes = [vp, vp, vp, vp, i, i, i, vp, lg, vp, lg, vp, vp, vp, lg, i, i, vp, vp, sz, i, vp]
    lib.prh_test_gemm_tn_side_ex.restype = i
    lib.prh_test_gemm_tn_side_ex.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp, vp, lg, vp, lg, vp, vp, vp, lg, i, i, i,
                                             C.POINTER(i), vp, vp, sz, i, vp]
    lib.prh_test_xcc_map.restype = i
    lib.prh_test_xcc_map.argtypes = [i, i, vp, i, vp]
    if not hasattr(lib, "prh_test_reduce_depth"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no raw reduction entries
    lib.prh_test_reduce_depth.restype = i
    lib.prh_test_reduce_depth.argtypes = [i]
    lib.prh_test_reduce_slabs.restype = i
    lib.prh_test_reduce_slabs.argtypes = [vp, i, i, i, vp, lg, vp, i, vp, i, vp]
    lib.prh_test_reduce_bn_stage1.restype = i
    lib.prh_test_reduce_bn_stage1.argtypes = [vp, vp, i, lg, i, i, i, i, vp, i, vp]
    lib.prh_test_reduce_partials.restype = i
    lib.prh_test_reduce_partials.argtypes = [vp, vp, i, i, vp, vp, i, vp]
    lib.prh_test_reduce_ln_param_grad.restype = i
    lib.prh_test_reduce_ln_param_grad.argtypes = [vp, vp, i, vp, vp, i, vp]
    lib.prh_test_reduce_pos_hidden_final.restype = i
    lib.prh_test_reduce_pos_hidden_final.argtypes = [vp, i, i, vp, vp, i, vp]
    lib.prh_test_reduce_partial_rows_final.restype = i
    lib.prh_test_reduce_partial_rows_final.argtypes = [vp, i, i, vp, i, vp, i, vp]
    lib.prh_test_reduce_act_amax_workspace_bytes.restype = sz
    lib.prh_test_reduce_act_amax_workspace_bytes.argtypes = []
    lib.prh_test_reduce_act_amax.restype = i
    lib.prh_test_reduce_act_amax.argtypes = [vp, vp, i, lg, i, vp, vp, vp, vp, sz, i, vp]
    if not hasattr(lib, "prh_ground_query"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no ground lift
    lib.prh_ground_max_bins.restype = i
    lib.prh_ground_max_bins.argtypes = []
    lib.prh_ground_bin_workspace_bytes.restype = sz
    lib.prh_ground_bin_workspace_bytes.argtypes = [ll]
    lib.prh_ground_bin_count.restype = i
    lib.prh_ground_bin_count.argtypes = [vp, i, vp, i, ll, vp, vp, vp, ll, dbl, vp, i, vp]
    lib.prh_ground_bin_write.restype = i
    lib.prh_ground_bin_write.argtypes = [vp, i, vp, i, ll, vp, vp, vp, ll, dbl, vp, vp, ll, vp, sz, i, vp]
    lib.prh_ground_query.restype = i
    lib.prh_ground_query.argtypes = [vp, i, vp, i, ll, vp, vp, ll, vp, vp, vp, ll, dbl, vp, vp, ll, dbl, dbl, dbl, dbl, i, i,
                                     i, i, vp, vp, vp, vp, i, vp]
    if not hasattr(lib, "prh_align_score"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no paint alignment
    lib.prh_align_tile.restype = i
    lib.prh_align_tile.argtypes = []
    lib.prh_align_max_shifts.restype = i
    lib.prh_align_max_shifts.argtypes = []
    lib.prh_align_select_workspace_bytes.restype = sz
    lib.prh_align_select_workspace_bytes.argtypes = [i]
    lib.prh_align_select_count.restype = i
    lib.prh_align_select_count.argtypes = [vp, i, vp, i, ll, vp, vp, vp, vp, ll, dbl, dbl, vp, i, vp]
    lib.prh_align_select_write.restype = i
    lib.prh_align_select_write.argtypes = [vp, i, vp, i, ll, vp, vp, vp, vp, ll, dbl, dbl, vp, vp, ll, vp, sz, i, vp]
    lib.prh_align_score.restype = i
    lib.prh_align_score.argtypes = [vp, vp, ll, vp, ll, vp, i, vp, vp, vp, ll, vp, i, vp, ll, dbl, vp, i, vp]
    if not hasattr(lib, "prh_align_score_rigid"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no rigid paint alignment
    lib.prh_align_max_poses.restype = i
    lib.prh_align_max_poses.argtypes = []
    lib.prh_align_select_cells_workspace_bytes.restype = sz
    lib.prh_align_select_cells_workspace_bytes.argtypes = [ll]
    lib.prh_align_select_cells_count.restype = i
    lib.prh_align_select_cells_count.argtypes = [vp, i, vp, i, ll, vp, vp, vp, vp, ll, dbl, dbl, vp, i, vp]
    lib.prh_align_select_cells_write.restype = i
    lib.prh_align_select_cells_write.argtypes = [vp, i, vp, i, ll, vp, vp, vp, vp, ll, dbl, dbl, vp, vp, ll, vp, sz, i, vp]
    lib.prh_align_score_rigid.restype = i
    lib.prh_align_score_rigid.argtypes = [vp, vp, ll, vp, ll, vp, i, vp, vp, vp, ll, vp, vp, i, vp, ll, dbl, vp, i, vp]
    if not hasattr(lib, "prh_trace_link"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no paint tracing
    lib.prh_trace_max_nms.restype = i
    lib.prh_trace_max_nms.argtypes = []
    lib.prh_trace_workspace_bytes.restype = sz
    lib.prh_trace_workspace_bytes.argtypes = [i, i, i]
    lib.prh_trace_hist.restype = i
    lib.prh_trace_hist.argtypes = [vp, i, vp, i, ll, ll, dbl, dbl, i, dbl, dbl, i, dbl, vp, sz, i, vp]
    lib.prh_trace_peaks_count.restype = i
    lib.prh_trace_peaks_count.argtypes = [vp, sz, i, i, i, i, i, ll, vp, i, vp]
    lib.prh_trace_peaks_write.restype = i
    lib.prh_trace_peaks_write.argtypes = [vp, sz, i, i, i, i, i, ll, vp, ll, i, vp, vp, vp, vp, vp, i, vp]
    lib.prh_trace_link.restype = i
    lib.prh_trace_link.argtypes = [vp, ll, i, vp, vp, ll, i, i, i, vp, vp, i, vp]
    if not hasattr(lib, "prh_floor_otsu"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no paint floor
    lib.prh_floor_max_bins.restype = i
    lib.prh_floor_max_bins.argtypes = []
    lib.prh_floor_hist.restype = i
    lib.prh_floor_hist.argtypes = [vp, i, vp, i, ll, dbl, dbl, dbl, i, i, vp, dbl, dbl, i, vp, i, vp]
    lib.prh_test_floor_hist.restype = i
    lib.prh_test_floor_hist.argtypes = [i] + lib.prh_floor_hist.argtypes
    lib.prh_floor_otsu.restype = i
    lib.prh_floor_otsu.argtypes = [vp, i, i, ll, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i, vp]
    if not hasattr(lib, "prh_trace_hist_surface"):
        return lib      # an older build under PRH_LIB_PATH (A/B runs): it has no surface gate
    lib.prh_trace_hist_surface.restype = i
    lib.prh_trace_hist_surface.argtypes = lib.prh_trace_hist.argtypes[:-2] + [dbl, dbl, dbl, i, i, vp, dbl, vp, i, vp]
    return lib


def lib():
    """The loaded library; raises RuntimeError if it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                        "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
                _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().prh_last_error().decode(errors="replace")
        if rc == -1:
            raise RuntimeError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (code {rc}): {msg}")
