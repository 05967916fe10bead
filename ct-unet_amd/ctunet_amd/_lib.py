"""ctypes binding of libctunet_hip.so (the C ABI declared in include/ctunet_hip.h).

There is no fallback: if the library is missing or a symbol cannot be resolved the import of
the product path fails with a clear message.  Build with ``python __graft_entry__.py`` or
``make -C ct-unet_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# CTUNET_HIP_LIB: load a differently built libctunet_hip.so (development A/B runs); there is no other fallback
LIB_PATH = os.environ.get("CTUNET_HIP_LIB") or os.path.join(_HERE, "libctunet_hip.so")

P = C.c_void_p          # device pointer / stream
I = C.c_int
L = C.c_int64
F = C.c_float
D = C.c_double
Z = C.c_size_t
U = C.c_uint64

class PackJob(C.Structure):
    """ctu_pack_job of include/ctunet_hip.h."""
    _fields_ = [("w", C.c_void_p), ("wp", C.c_void_p), ("cinv", C.c_void_p), ("kind", C.c_int), ("Co", C.c_int),
                ("Ci", C.c_int), ("k", C.c_int), ("rin_p", C.c_int), ("nout_p", C.c_int), ("mode", C.c_int),
                ("layout", C.c_int)]


class BnTail(C.Structure):
    """ctu_bn_tail of include/ctunet_hip.h."""
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("scale", C.c_void_p), ("shift", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p),
                ("num_batches_tracked", C.c_void_p), ("counter", C.c_void_p), ("count", C.c_double),
                ("momentum", C.c_float), ("eps", C.c_float), ("C", C.c_int), ("n_updates", C.c_int)]


class BnBwdTail(C.Structure):
    """ctu_bn_bwd_tail of include/ctunet_hip.h."""
    _fields_ = [("gamma", C.c_void_p), ("invstd", C.c_void_p), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("coef", C.c_void_p), ("mean", C.c_void_p), ("running_mean", C.c_void_p), ("running_var", C.c_void_p),
                ("num_batches_tracked", C.c_void_p), ("counter", C.c_void_p), ("count", C.c_double),
                ("momentum", C.c_float), ("eps", C.c_float), ("C", C.c_int)]


class WgradJob(C.Structure):
    """ctu_wgrad_job of include/ctunet_hip.h."""
    _fields_ = [("ws", C.c_void_p), ("dw", C.c_void_p), ("db", C.c_void_p), ("cinv", C.c_void_p), ("kind", C.c_int),
                ("Co", C.c_int), ("Ci", C.c_int), ("cin_p", C.c_int), ("n_ci_g", C.c_int), ("gx", C.c_int),
                ("pairs", C.c_int), ("nmf", C.c_int)]


class SegLossCfg(C.Structure):
    """ctu_seg_loss_cfg of include/ctunet_hip.h."""
    _fields_ = [("ce_lambda", C.c_float), ("dice_lambda", C.c_float), ("tversky_lambda", C.c_float),
                ("boundary_lambda", C.c_float), ("w0", C.c_float), ("w1", C.c_float), ("focal_gamma", C.c_float),
                ("tversky_alpha", C.c_float), ("tversky_beta", C.c_float), ("dice_softmax", C.c_int)]


WGRAD_JOBS_MAX = 4       # CTU_WGRAD_JOBS_MAX

# name -> (restype, argtypes); mirrors include/ctunet_hip.h one to one
SIGNATURES = {
    "ctu_last_error": (C.c_char_p, []),
    "ctu_abi_version": (I, []),
    "ctu_arch": (C.c_char_p, []),
    "ctu_ncdhw_to_ndhwc": (I, [P, P, I, I, I, I, I, I, I, P]),
    "ctu_ndhwc_to_ncdhw": (I, [P, P, I, I, I, I, I, I, P]),
    "ctu_conv3d_layout": (I, [I, I, I]),
    "ctu_conv3d_fwd_kernel_name": (C.c_char_p, [I, I, I, I, I, I, I]),
    "ctu_conv3d_wgrad_kernel_name": (C.c_char_p, [I, I, I, I]),
    "ctu_conv3d_packed_floats": (Z, [I, I, I, I]),
    "ctu_conv3d_num_blocks": (I, [I, I, I, I, I, I, I]),
    "ctu_pack_conv3d_weight": (I, [P, P, I, I, I, P, I, I, I, I, P]),
    "ctu_pack_batch": (I, [P, I, P]),
    "ctu_conv3d_fwd": (I, [P, I, I, P, P, I, P, P, I, P, I, I, P, I, I, I, I, I, I, P, P]),
    "ctu_conv3d_wgrad_ws_floats": (Z, [I, I, I, I, I, I, I]),
    "ctu_conv3d_wgrad": (I, [P, I, I, P, P, I, P, I, I, P, P, I, I, P, P, I, I, I, I, I, P]),
    "ctu_conv3d_wgrad_bn_supported": (I, [I, I, I, I, I, I, I]),
    "ctu_conv3d_wgrad_bn": (I, [P, I, I, P, P, I, P, I, I, P, P, P, P, P, P, I, I, P, P, I, I, I, I, I, P]),
    "ctu_conv3d_first_supported": (I, [I, I, I, I]),
    "ctu_conv3d_first_num_blocks": (I, [I, I, I, I]),
    "ctu_conv3d_first_fwd": (I, [P, I, P, P, I, P, I, I, P, I, I, I, I, P, P]),
    "ctu_conv3d_first_bwd_data": (I, [P, I, P, I, I, P, I, I, I, I, P]),
    "ctu_conv3d_first_wgrad_ws_floats": (Z, [I, I, I, I, I]),
    "ctu_conv3d_first_wgrad": (I, [P, I, P, I, P, I, P, I, I, I, I, P]),
    "ctu_conv3d_first_wgrad_bn": (I, [P, I, P, I, P, P, P, P, P, P, I, P, I, I, I, I, P]),
    "ctu_bn_finalize": (I, [P, I, I, I, D, P, P, P, P, F, F, I, P, P, P, P, P, P]),
    "ctu_bn_eval_affine": (I, [P, P, P, P, F, I, I, P, P, P]),
    "ctu_bn_bwd_num_blocks": (I, [L]),
    "ctu_bn_relu_bwd_reduce": (I, [P, I, P, I, I, P, P, P, P, L, P, P, P]),
    "ctu_bn_bwd_finalize": (I, [P, I, I, I, D, P, P, P, P, P, P, P, P, F, F, P, P]),
    "ctu_bn_relu_bwd_apply": (I, [P, I, P, I, I, P, P, P, P, P, L, P]),
    "ctu_conv3d_wgrad_slabs": (I, [P, I, I, P, P, I, P, I, I, P, P, I, I, P, P, I, I, I, I, I, P, P]),
    "ctu_conv3d_wgrad_bn_slabs": (I, [P, I, I, P, P, I, P, I, I, P, P, P, P, P, P, I, I, P, P, I, I, I, I, I, P, P]),
    "ctu_conv3d_first_wgrad_slabs": (I, [P, I, P, I, P, I, P, I, I, I, I, P, P]),
    "ctu_conv3d_first_wgrad_bn_slabs": (I, [P, I, P, I, P, P, P, P, P, P, I, P, I, I, I, I, P, P]),
    "ctu_convt2_wgrad_slabs": (I, [P, I, I, P, P, I, P, I, I, P, P, I, I, P, P, I, I, I, I, P, P]),
    "ctu_bn_bwd_finalize_jobs": (I, [P, I, I, I, D, P, P, P, P, P, P, P, P, F, F, P, P, I, P]),
    "ctu_wgrad_reduce_jobs": (I, [P, I, P]),
    "ctu_maxpool2_fwd": (I, [P, I, I, P, P, I, P, I, I, I, I, I, P]),
    "ctu_maxpool2_bwd": (I, [P, I, I, P, P, I, P, I, P, I, I, I, I, I, I, P]),
    "ctu_maxpool2_bwd_bn_num_blocks": (I, [I, I, I, I, I]),
    "ctu_maxpool2_bwd_bn": (I, [P, I, I, P, P, P, P, P, I, P, I, I, I, I, I, I, P, P, P]),
    "ctu_convt_packed_floats": (Z, [I, I]),
    "ctu_pack_convt_weight": (I, [P, P, I, I, P, I, I, I, P]),
    "ctu_convt2_fwd": (I, [P, I, I, P, P, I, P, P, I, P, I, I, I, I, I, I, P]),
    "ctu_convt2_bwd_data": (I, [P, I, I, P, P, I, I, I, I, I, I, P]),
    "ctu_convt2_wgrad_ws_floats": (Z, [I, I, I, I, I, I]),
    "ctu_convt2_wgrad": (I, [P, I, I, P, P, I, P, I, I, P, P, I, I, P, P, I, I, I, I, P]),
    "ctu_convt2_plan": (C.c_char_p, [I, I, I, I, I, I, I, P]),
    "ctu_convt2_wgrad_plan": (C.c_char_p, [I, I, I, I, I, I, P]),
    "ctu_head_fwd": (I, [P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, I, L, P]),
    "ctu_head_bwd_ws_floats": (Z, [I, L, I, I]),
    "ctu_head_bwd": (I, [P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, P, P, I, L, P]),
    "ctu_head_bwd_num_blocks": (I, [I, L]),
    "ctu_head_bwd_bn": (I, [P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, P, P, I, L, P, P, I, P, P, P]),
    "ctu_head_fwd_seg2": (I, [P, I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, I, L, P]),
    "ctu_head_bwd_bn_seg2": (I, [P, I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, I, P, P, P, I, L, P, P, I, P, P, P]),
    "ctu_loss_ws_floats": (Z, [I, L]),
    "ctu_loss_fwd": (I, [P, P, I, L, F, F, I, P, P, P]),
    "ctu_loss_bwd": (I, [P, P, I, L, F, F, I, P, P, P, P, I, P]),
    "ctu_seg_loss_ws_floats": (Z, [I, L]),
    "ctu_seg_loss_fwd": (I, [P, P, P, I, L, P, P, P, P]),
    "ctu_seg_loss_bwd": (I, [P, P, P, I, L, P, P, P, P, P, P, P, I, P]),
    "ctu_skip_add": (I, [P, I, P, P, I, P, I, P, P, I, P, I, I, L, P]),
    "ctu_upconv_fused_supported": (I, [I, I, I, I, I, I]),
    "ctu_upconv_fused_packed_floats": (Z, [I, I]),
    "ctu_upconv_fused_num_blocks": (I, [I, I, I, I, I]),
    "ctu_upconv_fused_pack_ws_floats": (Z, [I, I]),
    "ctu_upconv_fused_pack": (I, [P, P, P, I, I, P, I, I, P, P, P, P]),
    "ctu_upconv_fused_pack_all": (I, [P, P, P, I, I, P, I, I, P, P, P, P, P]),
    "ctu_upconv_fused_fwd": (I, [P, I, I, P, P, I, P, P, P, I, I, P, I, I, I, I, P, P]),
    "ctu_upconv_fused_wgrad_ws_floats": (Z, [I, I, I, I, I, I]),
    "ctu_upconv_fused_wgrad": (I, [P, I, I, P, P, I, P, I, I, P, P, I, I, I, I, P]),
    "ctu_upconv_fused_wgrad_bn_supported": (I, [I, I, I, I, I, I]),
    "ctu_upconv_fused_wgrad_bn": (I, [P, I, I, P, P, I, P, I, I, P, P, P, P, P, P, P, I, I, I, I, P]),
    "ctu_upconv_fused_project_ws_floats": (Z, [I, L]),
    "ctu_upconv_fused_project": (I, [P, P, I, I, I, I, I, I, P, P, P, I, I, I, P, P, P, P, P]),
    "ctu_upconv_fused_bwd_packed_floats": (Z, [I, I]),
    "ctu_upconv_fused_pack_bwd": (I, [P, I, I, P, P]),
    "ctu_upconv_fused_bwd_data": (I, [P, I, I, P, P, I, I, I, I, I, I, P]),
    "ctu_upconv_fused_seg2_supported": (I, [I, I, I, I, I, I, I]),
    "ctu_upconv_fused_fwd_seg2": (I, [P, P, I, I, I, P, P, I, P, P, P, I, I, P, I, I, I, I, P, P]),
    "ctu_upconv_fused_wgrad_seg2": (I, [P, P, I, I, I, P, P, I, P, I, I, P, P, I, I, I, I, P]),
    "ctu_upconv_fused_wgrad_bn_seg2": (I, [P, P, I, I, I, P, P, I, P, I, I, P, P, P, P, P, P, P, I, I, I, I, P]),
    "ctu_upconv_fused_bwd_data_seg2": (I, [P, I, I, P, P, P, I, I, I, I, I, I, I, P]),
    "ctu_hard_segm": (I, [P, I, I, L, P, P]),
    "ctu_one_hot": (I, [P, I, I, L, P, P]),
    "ctu_hard_dice_ws_doubles": (Z, [I]),
    "ctu_hard_dice_counts": (I, [P, P, I, I, L, P, P, P]),
    "ctu_hausdorff_ws_bytes": (Z, [I, I, I, I, I]),
    "ctu_hausdorff": (I, [P, P, I, I, I, I, I, P, P, P]),
    "ctu_surface_ws_bytes": (Z, [I, I, I, I, I]),
    "ctu_surface_metrics": (I, [P, I, I, P, I, I, I, I, I, I, I, I, I, P, P, D, P, P, P]),
    "ctu_components_ws_bytes": (Z, [I, I, I, I]),
    "ctu_label_components": (I, [P, I, I, I, I, I, I, P, I, P, P, P, P]),
    "ctu_filter_components": (I, [P, I, I, I, I, I, I, P, I, I, I, P, P, P]),
    "ctu_region_moments_ws_bytes": (Z, [I, I]),
    "ctu_region_moments": (I, [P, I, I, I, I, I, I, P, P, P, P, P]),
    "ctu_region_derive": (I, [P, I, I, P, P, P, P, P, P]),
    "ctu_morphology_ws_bytes": (Z, [I, I, I, I, I]),
    "ctu_binary_morphology": (I, [P, I, I, I, I, I, I, C.c_uint32, I, I, I, L, P, P, P]),
    "ctu_fill_holes": (I, [P, I, I, I, I, I, I, I, L, P, P, P]),
    "ctu_implant_mask": (I, [P, I, P, I, I, I, I, I, C.c_uint32, I, I, I, I, P, P, P]),
    "ctu_distance_ws_bytes": (Z, [I, I, I, I, I, I]),
    "ctu_distance_transform": (I, [P, I, I, I, I, I, I, L, I, I, P, I, P, P, F, P, P]),
    "ctu_thickness_ws_bytes": (Z, [I, I, I, I, I]),
    "ctu_local_thickness": (I, [P, I, I, I, I, I, P, P, P, P]),
    "ctu_thickness_summary_ws_bytes": (Z, [I, L]),
    "ctu_thickness_summary": (I, [P, I, L, F, P, P, P]),
    "ctu_resample": (I, [P, I, I, I, L, I, I, I, I, I, I, P, P, P, P, P]),
    "ctu_affine_resample": (I, [P, I, I, I, L, I, I, I, I, I, I, P, P, P, P, P, D, P, P]),
    "ctu_registration_ws_bytes": (Z, [L]),
    "ctu_registration_init": (I, [P, L, P, P, P]),
    "ctu_registration_accumulate": (I, [P, L, P, I, I, I, P, P, D, P, P]),
    "ctu_registration_update": (I, [L, I, P, P, P, I, P, P]),
    "ctu_similarity_ws_bytes": (Z, [L, L]),
    "ctu_similarity_init": (I, [P, L, P, P, P]),
    "ctu_similarity_accumulate": (I, [I, P, L, P, I, I, I, P, P, P, L, P, I, I, I, P, P, D, P, P]),
    "ctu_similarity_update": (I, [I, L, L, I, P, P, P, I, P, P]),
    "ctu_ffd_ws_bytes": (Z, [P, L]),
    "ctu_ffd_cells": (I, [P, L, P, P, P, P, P, P]),
    "ctu_ffd_init": (I, [P, L, P, D, P, P, P]),
    "ctu_ffd_accumulate": (I, [P, L, P, P, I, I, I, P, P, P, P, P, D, P, P, P, P, L, P, P]),
    "ctu_ffd_update": (I, [L, P, P, P, P, L, I, P, P, I, P, P]),
    "ctu_ffd_transform_points": (I, [P, L, P, P, P, P, P, P, P, P]),
    "ctu_ffd_resample": (I, [P, I, I, I, L, I, I, I, I, I, I, P, P, P, P, P, P, P, P, P, D, P, P]),
    "ctu_mesh_ws_bytes": (Z, [I, I, I]),
    "ctu_mesh_count": (I, [P, I, I, I, I, I, L, F, P, P]),
    "ctu_mesh_emit": (I, [P, I, I, I, I, F, F, P, P, L, L, P, P, P, P]),
    "ctu_mesh_measure": (I, [P, L, P, L, P, P, P, P]),
    "ctu_mesh_adjacency_ws_bytes": (Z, [L, L]),
    "ctu_mesh_adjacency_build": (I, [P, L, L, P, P, P]),
    "ctu_mesh_adjacency_emit": (I, [L, L, L, P, P, P, P]),
    "ctu_mesh_smooth_ws_bytes": (Z, [L]),
    "ctu_mesh_smooth": (I, [P, L, P, P, L, P, I, F, I, F, P, P, P]),
    "ctu_mesh_voxelize_ws_bytes": (Z, [I, I, I]),
    "ctu_mesh_voxelize": (I, [P, L, P, L, I, I, I, P, P, I, P, P, P]),
    "ctu_mesh_grid_ws_bytes": (Z, [L, L]),
    "ctu_mesh_grid_build": (I, [P, L, P, L, F, L, P, P, P]),
    "ctu_mesh_grid_emit": (I, [P, L, L, L, L, P, P, P, P]),
    "ctu_mesh_distance": (I, [P, L, P, P, L, P, I, I, I, P, L, I, I, I, P, P, F, F, P, P, P, P]),
    "ctu_mesh_decimate_ws_bytes": (Z, [L, L, L]),
    "ctu_mesh_decimate_bounds": (I, [P, L, P, L, P, P]),
    "ctu_mesh_decimate_build": (I, [P, L, P, L, P, P, P, L, I, P, P]),
    "ctu_mesh_decimate_emit": (I, [P, L, L, L, L, P, P, P, P, P, P, P]),
    "ctu_gaussian_ws_bytes": (Z, [L, I, I, I, I]),
    "ctu_gaussian_filter": (I, [P, I, L, I, I, I, P, P, I, F, P, P, P]),
    "ctu_minmax_ws_bytes": (Z, [L]),
    "ctu_finite_minmax": (I, [P, I, L, P, P, P]),
    "ctu_histogram": (I, [P, I, L, I, P, D, D, P, P]),
    "ctu_threshold_otsu": (I, [P, I, P, D, D, P, P, P]),
    "ctu_binarize": (I, [P, I, L, P, D, P, D, P, P]),
    "ctu_rank_filter_ws_bytes": (Z, [L, I, I, I, P]),
    "ctu_rank_filter": (I, [P, I, L, I, I, I, P, I, I, D, P, P, P]),
    "ctu_extract_patches": (I, [P, P, I, I, I, I, I, I, I, I, P, P]),
    "ctu_stitch_patches": (I, [P, P, I, I, I, I, I, I, I, I, P, P]),
    "ctu_window_accumulate": (I, [P, P, P, P, I, I, I, I, I, I, I, I, P, P, P, F, I, I, I, P, P, P]),
    "ctu_window_finalize": (I, [P, P, I, L, P, P, P]),
    "ctu_extract_patches_flip": (I, [P, P, P, I, I, I, I, I, I, I, I, P, P]),
    "ctu_window_accumulate_flip": (I, [P, P, P, P, P, I, I, I, I, I, I, I, I, P, P, P, F, I, I, I, P, P, P, P, P]),
    "ctu_window_finalize_stats": (I, [P, P, P, P, I, L, P, P, P, P, P, P]),
    "ctu_flap_count": (I, [P, I, I, L, P, P]),
    "ctu_flap_draw": (I, [P, I, I, I, I, I, P, I, P, U, F, I, I, I, P, P, U, F, F, I, P, P]),
    "ctu_flap_apply": (I, [P, I, P, I, I, I, I, P, I, P, P, P, U, I, P, I, P, P, P]),
    "ctu_patch_index": (I, [P, I, L, I, P, P, P]),
    "ctu_patch_draw": (I, [P, P, I, I, I, I, I, P, P, I, P, U, P, P, P, P, P, P]),
    "ctu_patch_crop": (I, [P, I, I, I, I, I, I, P, I, I, I, I, D, P, I, I, I, P]),
    "ctu_spatial_draw": (I, [I, I, I, I, P, P, U, I, D, D, D, P, I, I, I, I, P, P, P]),
    "ctu_spatial_warp": (I, [P, I, I, I, I, I, I, P, I, I, I, P, P, P, P, P]),
    "ctu_defect_draw": (I, [P, I, I, I, I, I, P, P, P, U, D, P, I, I, I, I, I, P, P, P]),
    "ctu_defect_apply": (I, [P, I, P, I, I, I, I, P, P, P, I, I, I, D, D, P, I, P, P, P, U, I, P, I, P, P, P]),
    "ctu_random_dilate": (I, [P, I, I, I, I, I, I, P, U, D, P, P]),
    "ctu_lp_upconv_fused_supported": (I, [I, I, I, I, I, I]),
    "ctu_lp_upconv_fused_packed_elems": (Z, [I]),
    "ctu_lp_upconv_fused_num_blocks": (I, [I, I, I, I]),
    "ctu_lp_upconv_fused_pack": (I, [I, P, I, P, P]),
    "ctu_lp_upconv_fused_fwd": (I, [I, P, I, I, P, P, I, P, P, P, I, P, I, I, I, I, P]),
    "ctu_lp_upconv_fused_wgrad_ws_floats": (Z, [I, I, I, I, I]),
    "ctu_lp_upconv_fused_wgrad": (I, [I, P, I, I, P, P, I, P, I, P, P, I, I, I, I, P]),
    "ctu_lp_upconv_fused_wgrad_bn_supported": (I, [I, I, I, I, I]),
    "ctu_lp_upconv_fused_wgrad_bn": (I, [I, P, I, I, P, P, I, P, I, P, P, P, P, P, P, P, I, I, I, I, P]),
    "ctu_lp_conv3d_wgrad_bn_supported": (I, [I, I, I, I, I, I, I]),
    "ctu_lp_conv3d_wgrad_bn": (I, [I, P, I, I, P, P, I, P, I, I, P, P, P, P, P, P, I, I, P, P, I, I, I, I, I, P]),
    "ctu_lp_upconv_fused_project": (I, [I, P, P, I, I, I, I, I, I, P, P, P, I, I, I, P, P, P, P, P]),
    "ctu_lp_upconv_fused_bwd_data": (I, [I, P, I, P, P, I, I, I, I, I, I, P]),
    "ctu_lp_conv3d_layout": (I, [I, I, I, I]),
    "ctu_lp_conv3d_packed_elems": (Z, [I, I, I]),
    "ctu_lp_conv3d_num_blocks": (I, [I, I, I, I, I, I, I, I]),
    "ctu_lp_pack_conv3d_weight": (I, [I, P, P, I, I, I, P, I, I, I, I, P]),
    "ctu_lp_pack_batch": (I, [I, P, I, P]),
    "ctu_lp_conv3d_fwd": (I, [I, P, I, I, P, P, I, P, P, I, P, I, I, P, I, I, I, I, I, I, P, P]),
    "ctu_lp_conv3d_wgrad_ws_floats": (Z, [I, I, I, I, I, I, I]),
    "ctu_lp_conv3d_wgrad": (I, [I, P, I, I, P, P, I, P, I, I, P, I, I, P, P, I, I, I, I, I, P]),
    "ctu_lp_conv3d_first_fwd": (I, [I, P, I, P, P, I, P, I, I, P, I, I, I, I, P, P]),
    "ctu_lp_conv3d_first_bwd_data": (I, [I, P, I, P, I, I, P, I, I, I, I, P]),
    "ctu_lp_conv3d_first_bwd_data_pair_supported": (I, [I, I]),
    "ctu_lp_conv3d_fwd_kernel_name": (C.c_char_p, [I, I, I, I, I, I, I, I]),
    "ctu_lp_conv3d_wgrad_kernel_name": (C.c_char_p, [I, I, I, I, I, I]),
    "ctu_lp_conv3d_first_bwd_data_pair": (I, [I, P, I, P, I, P, I, I, I, I, P]),
    "ctu_lp_conv3d_first_wgrad": (I, [I, P, I, P, I, P, I, P, I, I, I, I, P]),
    "ctu_lp_convt_packed_elems": (Z, [I, I, I]),
    "ctu_lp_pack_convt_weight": (I, [I, P, P, I, I, P, I, I, I, P]),
    "ctu_lp_convt2_fwd": (I, [I, P, I, I, P, P, I, P, P, I, P, I, I, I, I, I, I, P]),
    "ctu_lp_convt2_bwd_data": (I, [I, P, I, I, P, P, I, I, I, I, I, I, P]),
    "ctu_lp_convt2_wgrad_ws_floats": (Z, [I, I, I, I, I, I]),
    "ctu_lp_convt2_wgrad": (I, [I, P, I, I, P, P, I, P, I, I, P, I, I, P, P, I, I, I, I, P]),
    "ctu_lp_convt2_plan": (C.c_char_p, [I, I, I, I, I, I, I, P]),
    "ctu_lp_convt2_wgrad_plan": (C.c_char_p, [I, I, I, I, I, I, P]),
    "ctu_lp_ncdhw_to_ndhwc": (I, [I, P, P, I, I, I, I, I, I, I, P]),
    "ctu_lp_ndhwc_to_ncdhw": (I, [I, P, P, I, I, I, I, I, I, P]),
    "ctu_lp_bn_relu_bwd_reduce": (I, [I, P, I, P, I, I, P, P, P, P, L, P, P, P]),
    "ctu_lp_bn_relu_bwd_apply": (I, [I, P, I, P, I, I, P, P, P, P, P, L, P]),
    "ctu_lp_maxpool2_fwd": (I, [I, P, I, I, P, P, I, P, I, I, I, I, I, P]),
    "ctu_lp_maxpool2_bwd": (I, [I, P, I, I, P, P, I, P, I, P, I, I, I, I, I, I, P]),
    "ctu_lp_maxpool2_bwd_bn": (I, [I, P, I, I, P, P, P, P, P, I, P, I, I, I, I, I, I, P, P, P]),
    "ctu_lp_skip_add": (I, [I, P, I, P, P, I, P, I, P, P, I, P, I, I, L, P]),
    "ctu_lp_channel_sum": (I, [I, P, I, I, L, P, P, I, P]),
    "ctu_lp_head_fwd": (I, [I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, I, L, P]),
    "ctu_lp_head_bwd_bn": (I, [I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, P, P, I, L, P, P, I, P, P, F, P]),
    "ctu_lp_head_bwd_bn_dscale": (I, [I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, P, P, I, L, P, P, I, P, P, P, P]),
    "ctu_lp_head_fwd_seg2": (I, [I, P, I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, I, L, P]),
    "ctu_lp_head_bwd_bn_seg2": (I, [I, P, I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, I, P, P, P, I, L, P, P, I, P, P, F, P]),
    "ctu_lp_head_bwd_bn_dscale_seg2": (I, [I, P, I, P, I, I, P, P, I, P, P, P, I, I, I, I, P, P, P, I, P, I, P, P, P, I, L, P, P, I, P, P, P, P]),
    "ctu_scale_tensors": (I, [P, P, I, F, P, P]),
    "ctu_unscale_tensors": (I, [P, P, I, P, P, P]),
    "ctu_loss_scale_update": (I, [P, P, P, P, F, F, I, P]),
    "ctu_comm_available": (I, []),
    "ctu_comm_unique_id": (I, [P]),
    "ctu_comm_init": (I, [C.POINTER(C.c_void_p), I, I, P]),
    "ctu_comm_allreduce_f32": (I, [P, P, P, Z, I, P]),
    "ctu_comm_destroy": (I, [P]),
    "ctu_channel_sum_num_blocks": (I, [L]),
    "ctu_channel_sum": (I, [P, I, I, L, P, P, I, P]),
    "ctu_adam_amsgrad": (I, [P, P, I, P, D, D, D, D, D, I, P, P]),
    "ctu_adam_amsgrad_dev": (I, [P, P, I, P, P, D, D, D, D, I, P, P, P]),
    "ctu_grad_norm_num_blocks": (I, [P, I]),
    "ctu_grad_clip_coef": (I, [P, P, I, F, P, P, P, P]),
    "ctu_plateau_update": (I, [P, P, P, P, I, I, D, I, D, I, D, D, P]),
    "ctu_sgd": (I, [P, P, I, P, P, D, D, D, D, I, I, P, P, P]),
    "ctu_rmsprop": (I, [P, P, I, P, P, D, D, D, D, D, I, I, P, P, P]),
}

_lib = None
ABI_VERSION = 8          # CTU_ABI_VERSION of the csrc/ this file mirrors (bumped on any signature change)


class CtuError(RuntimeError):
    """A libctunet_hip.so entry point returned a non-zero status."""


def load() -> C.CDLL:
    """Load the shared library once and attach the prototypes.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the MI355X kernels are not built. Run `python __graft_entry__.py` "
            "(or `make -C ct-unet_amd/csrc`). There is no CPU fallback for this path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}; rebuild the library") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ctu_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} is ABI v{lib.ctu_abi_version()}, this package binds v{ABI_VERSION}: "
                          "a stale build -- run `python __graft_entry__.py` (or `make -C ct-unet_amd/csrc`)")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().ctu_last_error().decode("utf-8", "replace")
        raise CtuError(f"{what} failed (status {status}): {msg}")


# ---- what every wrapper of a volume entry point does around its call
# CTU_F32 / CTU_U8 / CTU_I64 / CTU_I16 / CTU_I32 of include/ctunet_hip.h; bool travels as uint8 (as_bytes)
DTYPE_CODE = {torch.float32: 0, torch.uint8: 3, torch.bool: 3, torch.int64: 4, torch.int16: 5, torch.int32: 6}


class on(torch.cuda.device):
    """``with on(device) as run: run("ctu_x", *args)``: enters the device, reads its current stream once, and ``run`` calls
    the entry point with that stream as the last argument and checks the status under the label ``x`` (or ``what=``).
    Several launches of one wrapper, and the host reads between them, stay inside one ``with``."""

    def __init__(self, device: torch.device):
        super().__init__(device.index)          # the index spares torch the parsing of a device: 1.3 us of a 10 us call

    def __enter__(self):
        super().__enter__()
        self._stream = torch.cuda.current_stream().cuda_stream
        return self._run

    def _run(self, name: str, *args, what: str = None) -> None:
        status = getattr(_lib or load(), name)(*args, self._stream)
        if status:
            check(status, what or name[4:])


def check_device(message: str, *tensors) -> None:
    """Refuse, in the caller's words, tensors that do not live on the GPU."""
    for t in tensors:
        if not t.is_cuda:
            raise ValueError(message)


def as_bytes(t):
    """The contiguous tensor a kernel reads: bool viewed as uint8, every other dtype as it is."""
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def array(ctype, values):
    """A host array for a ``const ctype*`` argument (None stays None: the entry point's default)."""
    if values is None:
        return None
    values = list(values)
    return (ctype * len(values))(*values)


def float_array(values):
    return array(C.c_float, values)


def double_array(values):
    return array(C.c_double, values)
