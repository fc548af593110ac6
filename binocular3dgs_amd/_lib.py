"""ctypes binding of the C ABI declared in include/b3gs_raster.h.

There is no fallback: if libb3gs_raster.so is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("B3GS_LIB") or os.path.join(_HERE, "libb3gs_raster.so")   # B3GS_LIB: A/B builds of the kernels

ABI_VERSION = 18
OK = 0
ERR_NAMES = {-1: "B3GS_ERR_ARG", -2: "B3GS_ERR_ALLOC", -3: "B3GS_ERR_HIP", -4: "B3GS_ERR_CAPACITY",
             -5: "B3GS_ERR_NO_DEVICE"}

c_float_p = C.c_void_p  # device pointers travel as plain integers

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class B3gsScene(C.Structure):
    _fields_ = [("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
                ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("scale_modifier", C.c_float),
                ("prefiltered", C.c_int32), ("debug", C.c_int32),
                ("background", C.c_void_p), ("means3D", C.c_void_p), ("shs", C.c_void_p),
                ("colors_precomp", C.c_void_p), ("opacities", C.c_void_p), ("scales", C.c_void_p),
                ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("viewmatrix", C.c_void_p),
                ("projmatrix", C.c_void_p), ("campos", C.c_void_p)]


class B3gsRawParams(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("features_dc", C.c_void_p), ("features_rest", C.c_void_p),
                ("scaling", C.c_void_p), ("rotation", C.c_void_p), ("opacity", C.c_void_p)]


class B3gsRawGrads(C.Structure):
    _fields_ = B3gsRawParams._fields_ + [("touched_rows", C.c_void_p)]


class B3gsFusedView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("radii", C.c_void_p), ("geometry", C.c_void_p),
                ("scratch", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("densify_stats", C.c_int32)]


class B3gsBlendView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p),
                ("image", C.c_void_p), ("out_color", C.c_void_p), ("out_depth", C.c_void_p),
                ("out_alpha", C.c_void_p), ("dL_dcolor", C.c_void_p), ("dL_ddepth", C.c_void_p),
                ("dL_dalpha", C.c_void_p), ("scratch", C.c_void_p), ("binning_capacity", C.c_int64)]


class B3gsForwardView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p),
                ("binning_capacity", C.c_int64), ("image", C.c_void_p), ("out_color", C.c_void_p),
                ("out_depth", C.c_void_p), ("out_alpha", C.c_void_p), ("radii", C.c_void_p),
                ("device_num_rendered", C.c_void_p), ("depth_order_from", C.c_int32), ("seg1_fraction", C.c_float),
                ("high_water", C.c_void_p), ("overflow_flag", C.c_void_p), ("depth_key_bits", C.c_int32),
                ("fresh_image", C.c_int32), ("depth_order_hint", C.c_void_p), ("hint_mismatch", C.c_void_p),
                ("hint_trusted", C.c_int32), ("visible", C.c_void_p), ("reference_binning", C.c_int32)]


class B3gsLossIO(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("image", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p),
                ("gt_image", C.c_void_p), ("shifted_image", C.c_void_p), ("alpha_weight", C.c_void_p),
                ("focal_x", C.c_float), ("trans_dist", C.c_float), ("lambda_dssim", C.c_float),
                ("lambda_smooth", C.c_float), ("grad_scale", C.c_float), ("dL_dimage", C.c_void_p),
                ("dL_ddepth", C.c_void_p), ("dL_dalpha", C.c_void_p), ("dL_dshifted", C.c_void_p),
                ("parts", C.c_void_p), ("workspace", C.c_void_p), ("trans_dist_dev", C.c_void_p)]


class B3gsDensifyIO(C.Structure):
    _fields_ = [("P", C.c_int32), ("M", C.c_int32), ("param", C.c_void_p * 6), ("exp_avg", C.c_void_p * 6),
                ("exp_avg_sq", C.c_void_p * 6), ("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p),
                ("grad_threshold", C.c_float), ("min_opacity", C.c_float), ("extent", C.c_float),
                ("percent_dense", C.c_float), ("max_screen_size", C.c_float)]


class B3gsAdamSegment(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("count", C.c_int64), ("lr", C.c_float), ("row_len", C.c_int32), ("first_row", C.c_int32),
                ("lr_dev", C.c_void_p)]


class B3gsDensifyStats(C.Structure):
    _fields_ = [("xyz_gradient_accum", C.c_void_p), ("denom", C.c_void_p), ("max_radii2D", C.c_void_p),
                ("skip_if_nonzero", C.c_void_p)]


class B3gsDebugViews(C.Structure):
    _fields_ = [("tiles_touched", C.c_void_p), ("depths", C.c_void_p), ("records", C.c_void_p),
                ("point_list", C.c_void_p), ("tile_ids", C.c_void_p), ("ranges", C.c_void_p),
                ("final_T", C.c_void_p), ("n_contrib", C.c_void_p), ("packed_idx_bits", C.c_int32),
                ("counts", C.c_void_p), ("point_list2", C.c_void_p), ("ranges2", C.c_void_p)]


class B3gsMetricView(C.Structure):
    _fields_ = [("image", C.c_void_p), ("gt", C.c_void_p), ("mask", C.c_void_p), ("mask_channels", C.c_int32),
                ("prepared_image", C.c_void_p), ("prepared_gt", C.c_void_p)]


class B3gsFrameView(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p), ("rgb_out", C.c_void_p),
                ("gray_out", C.c_void_p), ("cmap_out", C.c_void_p)]


class B3gsGtView(C.Structure):
    _fields_ = [("src", C.c_void_p), ("Hs", C.c_int32), ("Ws", C.c_int32), ("C", C.c_int32), ("tab_x", C.c_void_p),
                ("tab_y", C.c_void_p), ("ks_x", C.c_int32), ("ks_y", C.c_int32), ("image", C.c_void_p),
                ("alpha", C.c_void_p), ("bg_mask", C.c_void_p)]


class B3gsCloudGrow(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("W", "H", "n_views", "ref", "src", "n_seeds", "n_samples", "n_start", "h_patch_size", "init")]
                + [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "alpha", "ssim_threshold")]
                + [(n, C.c_void_p) for n in ("images", "w2c", "window", "seed_idx", "noise", "points", "colors")]
                + [("capacity", C.c_int32)]
                + [(n, C.c_void_p) for n in ("length", "overflow", "grids", "workspace", "debug_ssim", "debug_mask")])


class B3gsSweepPair(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("W", "H", "D", "stride", "radius")]
                + [(n, C.c_float) for n in ("near", "far", "inv_far", "step", "min_score", "margin", "min_var", "cyc_steps")]
                + [(n, C.c_void_p) for n in ("image_a", "image_b", "homographies", "proj", "kp_source", "kp_target", "score", "count",
                                             "node_invd", "node_score", "node_k", "workspace")])


class B3gsTsdfVolume(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3), ("voxel", C.c_float),
                ("tsdf", C.c_void_p), ("weight", C.c_void_p), ("rgb", C.c_void_p)]


class B3gsTsdfView(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("alpha", C.c_void_p), ("colour", C.c_void_p), ("rot", C.c_float * 9),
                ("trans", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float)]


class B3gsLpipsWeights(C.Structure):
    _fields_ = [("conv_w", C.c_void_p * 13), ("conv_b", C.c_void_p * 13), ("lin", C.c_void_p * 5), ("shift", C.c_float * 3),
                ("scale", C.c_float * 3)]


class B3gsContribView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("pixel_mask", C.c_void_p)]


class B3gsPixelMapView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("median_depth", C.c_void_p), ("depth_m1", C.c_void_p), ("depth_m2", C.c_void_p), ("dominant", C.c_void_p),
                ("count", C.c_void_p)]


class B3gsLabelVoteView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("labels", C.c_void_p)]


class B3gsLabelRenderView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("label", C.c_void_p), ("weight", C.c_void_p)]


class B3gsFeatureRenderView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("out", C.c_void_p)]


class B3gsFeatureLiftView(C.Structure):
    _fields_ = [("view", C.POINTER(B3gsScene)), ("geometry", C.c_void_p), ("binning", C.c_void_p), ("image", C.c_void_p),
                ("maps", C.c_void_p), ("pixel_mask", C.c_void_p)]


class B3gsContribOut(C.Structure):
    _fields_ = [("weight_q32", C.c_void_p), ("hits", C.c_void_p), ("wmax_bits", C.c_void_p), ("dominant", C.c_void_p)]


class B3gsCameraModel(C.Structure):
    _fields_ = [("model", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_params", C.c_int32), ("params", C.c_double * 12)]


class B3gsSimilarity(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("s", C.c_double), ("ln_s", C.c_double), ("q", C.c_double * 4),
                ("D1", C.c_double * 9), ("D2", C.c_double * 25), ("D3", C.c_double * 49)]


class B3gsSelect(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("flags", "nviews", "min_views", "mask_h", "mask_w")]
                + [("logit_min", C.c_float), ("log_max_scale", C.c_float), ("box", C.c_double * 12), ("half", C.c_double * 3),
                   ("centre", C.c_double * 3), ("r2", C.c_double), ("cameras", C.c_void_p), ("masks", C.c_void_p)])


class B3gsMcmcIO(C.Structure):
    _fields_ = [("P", C.c_int32), ("P_old", C.c_int32), ("K", C.c_int32), ("n_max", C.c_int32), ("min_opacity", C.c_float),
                ("offset", C.c_uint32), ("seed", C.c_uint64), ("param", C.c_void_p * 6), ("exp_avg", C.c_void_p * 6),
                ("exp_avg_sq", C.c_void_p * 6), ("draws", C.c_void_p)]


class B3gsMcmcViews(C.Structure):
    _fields_ = [("src", C.c_void_p), ("count", C.c_void_p), ("rank", C.c_void_p), ("weight_scan", C.c_void_p), ("head", C.c_void_p)]


class B3gsDepthPriorIO(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("depth", C.c_void_p), ("alpha", C.c_void_p), ("prior", C.c_void_p),
                ("mask", C.c_void_p), ("mode", C.c_int32), ("patch", C.c_int32), ("min_valid", C.c_int32), ("alpha_min", C.c_float),
                ("w_global", C.c_double), ("w_local", C.c_double), ("offset_dev", C.c_void_p), ("dL_ddepth", C.c_void_p),
                ("parts", C.c_void_p), ("workspace", C.c_void_p)]


class B3gsDepthResizeIO(C.Structure):
    _fields_ = [("Wsrc", C.c_int32), ("Hsrc", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("src", C.c_void_p),
                ("src_mask", C.c_void_p), ("prior", C.c_void_p), ("mask", C.c_void_p)]


class B3gsExposurePlane(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("in_", C.c_void_p), ("g_out", C.c_void_p), ("out", C.c_void_p), ("A", C.c_void_p),
                ("row_dev", C.c_void_p), ("V", C.c_int32), ("G", C.c_void_p), ("workspace", C.c_void_p)]


class B3gsExposureFitIO(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("render", C.c_void_p), ("gt", C.c_void_p), ("mask", C.c_void_p), ("A", C.c_void_p),
                ("sums", C.c_void_p), ("flag", C.c_void_p), ("workspace", C.c_void_p)]


class B3gsNormalPriorIO(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("depth", C.c_void_p), ("alpha", C.c_void_p), ("target", C.c_void_p),
                ("mask", C.c_void_p), ("alpha_min", C.c_float), ("tanfovx", C.c_double), ("tanfovy", C.c_double),
                ("w_cos", C.c_double), ("w_l1", C.c_double), ("dL_ddepth", C.c_void_p), ("dL_dalpha", C.c_void_p),
                ("normals", C.c_void_p), ("valid", C.c_void_p), ("parts", C.c_void_p), ("workspace", C.c_void_p)]


class B3gsDepthNormalsIO(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("depth", C.c_void_p), ("alpha", C.c_void_p), ("mask", C.c_void_p),
                ("alpha_min", C.c_float), ("tanfovx", C.c_double), ("tanfovy", C.c_double), ("normals", C.c_void_p),
                ("valid", C.c_void_p)]


class B3gsNormalResizeIO(C.Structure):
    _fields_ = [("Wsrc", C.c_int32), ("Hsrc", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("src", C.c_void_p),
                ("src_mask", C.c_void_p), ("normals", C.c_void_p), ("mask", C.c_void_p)]


class B3gsKernelTimes(C.Structure):
    _fields_ = [("preprocess_ms", C.c_double), ("sort_ms", C.c_double), ("render_fwd_ms", C.c_double),
                ("render_bwd_ms", C.c_double), ("preprocess_bwd_ms", C.c_double), ("calls", C.c_int64)]


# every symbol include/b3gs_raster.h declares (tests/test_abi.py checks the .so exports all of them)
EXPORTS = ("b3gs_abi_version", "b3gs_last_error", "b3gs_set_timing", "b3gs_timing_collect", "b3gs_geometry_bytes", "b3gs_image_bytes",
           "b3gs_binning_bytes", "b3gs_forward", "b3gs_forward_capacity", "b3gs_backward", "b3gs_mark_visible",
           "b3gs_debug_views", "b3gs_forward_raw", "b3gs_backward_raw", "b3gs_backward_scratch_floats",
           "b3gs_backward_raw_accumulate", "b3gs_blend_forward_batch", "b3gs_blend_backward_batch",
           "b3gs_adam_step", "b3gs_forward_raw_batch", "b3gs_loss_workspace_floats", "b3gs_binocular_loss",
           "b3gs_densify_classify", "b3gs_densify_scatter", "b3gs_knn_workspace_bytes", "b3gs_knn_mean_dist2",
           "b3gs_backward_raw_accumulate_range", "b3gs_binocular_loss_batch",
           # ABI 9: the training loop's statements one by one
           "b3gs_lossfn_workspace_floats", "b3gs_l1_loss_forward", "b3gs_l1_loss_backward", "b3gs_inverse_warp_forward",
           "b3gs_inverse_warp_backward", "b3gs_smooth_loss_forward", "b3gs_smooth_loss_backward", "b3gs_ssim_forward",
           "b3gs_ssim_backward", "b3gs_opacity_decay", "b3gs_add_densification_stats", "b3gs_adam_step_at", "b3gs_debug_activations",
           "b3gs_apply_staged_densify_stats",
           # ABI 11: image metrics of held-out views
           "b3gs_image_metrics_workspace_bytes", "b3gs_image_metrics_batch",
           # ABI 12: frames of a rendered path
           "b3gs_frames_workspace_bytes", "b3gs_encode_frames_batch",
           # ABI 13: ground-truth preparation of dataset images
           "b3gs_gt_workspace_bytes", "b3gs_prepare_gt_batch",
           # ABI 14: the matcher cloud
           "b3gs_cloud_workspace_bytes", "b3gs_triangulate_matches", "b3gs_background_sheet", "b3gs_cloud_grow_round",
           # ABI 15: the plane-sweep stereo matcher
           "b3gs_sweep_workspace_bytes", "b3gs_sweep_match_pair",
           # ABI 16: baseline JPEG of rendered frames
           "b3gs_jpeg_workspace_bytes", "b3gs_jpeg_encode_batch",
           # ABI 17: TSDF fusion and marching tetrahedra
           "b3gs_tsdf_integrate_batch", "b3gs_mesh_workspace_bytes", "b3gs_mesh_count", "b3gs_mesh_emit",
           # ABI 18: cleaning and scoring an extracted mesh
           "b3gs_mesh_components", "b3gs_mesh_clean_workspace_bytes", "b3gs_mesh_clean_count", "b3gs_mesh_clean_emit",
           "b3gs_mesh_sample_workspace_bytes", "b3gs_mesh_sample_count", "b3gs_mesh_sample_emit",
           "b3gs_nearest_workspace_bytes", "b3gs_nearest_grid", "b3gs_nearest_query",
           "b3gs_cloud_score_workspace_bytes", "b3gs_cloud_score",
           # added to ABI 18: simplifying an extracted mesh
           "b3gs_mesh_simplify_workspace_bytes", "b3gs_mesh_simplify_count", "b3gs_mesh_simplify_emit",
           # added to ABI 18: rendering an extracted mesh
           "b3gs_mesh_raster_workspace_bytes", "b3gs_mesh_raster_batch", "b3gs_mesh_resolve_batch",
           # added to ABI 18: texturing an extracted mesh
           "b3gs_mesh_texture_atlas_height", "b3gs_mesh_texture_accumulate_batch", "b3gs_mesh_texture_finalize",
           "b3gs_mesh_resolve_textured_batch",
           # added to ABI 18: smoothing an extracted mesh
           "b3gs_mesh_adjacency_workspace_bytes", "b3gs_mesh_adjacency_layout", "b3gs_mesh_adjacency_build", "b3gs_mesh_smooth",
           "b3gs_mesh_vertex_normals", "b3gs_mesh_resolve_shaded_batch",
           # added to ABI 18: LPIPS (VGG) of held-out views
           "b3gs_lpips_workspace_bytes", "b3gs_lpips_batch", "b3gs_lpips_features",
           # added to ABI 18: per-Gaussian render contribution
           "b3gs_blend_contribution_batch",
           # added to ABI 18: per-pixel geometry maps
           "b3gs_blend_pixel_maps_batch",
           # added to ABI 18: segmentation from 2D label planes
           "b3gs_label_votes_batch", "b3gs_label_render_batch",
           # added to ABI 18: feature fields
           "b3gs_feature_render_batch", "b3gs_feature_lift_batch",
           # added to ABI 18: weighted k-means codebooks
           "b3gs_kmeans_workspace_bytes", "b3gs_kmeans_assign", "b3gs_kmeans",
           # added to ABI 18: undistorting a COLMAP dataset
           "b3gs_camera_points", "b3gs_undistort_map", "b3gs_remap_batch",
           # added to ABI 18: editing a trained model
           "b3gs_transform_points", "b3gs_transform_gaussians", "b3gs_select_gaussians", "b3gs_nearest_query_index",
           "b3gs_similarity_sums_workspace_bytes", "b3gs_similarity_sums",
           # added to ABI 18: the camera pose gradient
           "b3gs_pose_gradient_workspace_bytes", "b3gs_pose_gradient",
           # added to ABI 18: merging Gaussians into levels of detail
           "b3gs_gaussian_merge_workspace_bytes", "b3gs_gaussian_merge_count", "b3gs_gaussian_merge_emit",
           # added to ABI 18: screened Poisson surface reconstruction
           "b3gs_oriented_points_workspace_bytes", "b3gs_oriented_points_batch", "b3gs_oriented_points_emit",
           "b3gs_poisson_workspace_bytes", "b3gs_poisson_splat", "b3gs_poisson_apply", "b3gs_poisson_solve", "b3gs_poisson_volume",
           # added to ABI 18: fixed-budget training (MCMC relocation and position noise)
           "b3gs_mcmc_random", "b3gs_mcmc_noise", "b3gs_mcmc_workspace_bytes", "b3gs_mcmc_relocate", "b3gs_mcmc_views",
           # added to ABI 18: depth priors (Pearson depth loss, prior resize)
           "b3gs_depth_prior_workspace_bytes", "b3gs_depth_prior_loss_batch", "b3gs_resize_depth_batch",
           # added to ABI 18: per-image exposure compensation (apply, backward, fit, row-sparse Adam)
           "b3gs_exposure_workspace_bytes", "b3gs_exposure_apply", "b3gs_exposure_backward", "b3gs_exposure_fit", "b3gs_exposure_adam",
           # added to ABI 18: normal priors (depth-derived normals, their loss, prior resize)
           "b3gs_normal_prior_workspace_bytes", "b3gs_normal_prior_loss_batch", "b3gs_depth_normals_batch",
           "b3gs_resize_normals_batch")

_lib = None


class B3gsError(RuntimeError):
    pass


def lib():
    """Load (once) and type the shared library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise B3gsError(f"{LIB_PATH} not found: run `python -m binocular3dgs_amd.build` (hipcc, gfx950). "
                        "There is no CPU or PyTorch fallback for the rasterizer.")
    L = C.CDLL(LIB_PATH)
    L.b3gs_abi_version.restype = C.c_int
    L.b3gs_last_error.restype = C.c_char_p
    L.b3gs_set_timing.argtypes = [C.c_void_p]
    L.b3gs_set_timing.restype = None
    L.b3gs_timing_collect.restype = C.c_int
    L.b3gs_geometry_bytes.argtypes = [C.c_int32]
    L.b3gs_geometry_bytes.restype = C.c_size_t
    L.b3gs_image_bytes.argtypes = [C.c_int32, C.c_int32]
    L.b3gs_image_bytes.restype = C.c_size_t
    L.b3gs_binning_bytes.argtypes = [C.c_int32, C.c_int64]
    L.b3gs_binning_bytes.restype = C.c_size_t
    L.b3gs_forward.argtypes = [C.POINTER(B3gsScene), ALLOC_FN, C.c_void_p, ALLOC_FN, C.c_void_p, ALLOC_FN,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_int32), C.c_void_p]
    L.b3gs_forward.restype = C.c_int
    L.b3gs_forward_capacity.argtypes = [C.POINTER(B3gsScene), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.b3gs_forward_capacity.restype = C.c_int
    L.b3gs_backward.argtypes = [C.POINTER(B3gsScene), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 8 + [C.c_void_p]
    L.b3gs_backward.restype = C.c_int
    L.b3gs_forward_raw.argtypes = [C.POINTER(B3gsScene), C.POINTER(B3gsRawParams), C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p]
    L.b3gs_forward_raw.restype = C.c_int
    for fn in (L.b3gs_blend_forward_batch, L.b3gs_blend_backward_batch):
        fn.argtypes = [C.c_int32, C.POINTER(B3gsBlendView), C.c_void_p]
        fn.restype = C.c_int
    L.b3gs_backward_scratch_floats.argtypes = [C.c_int32]
    L.b3gs_backward_scratch_floats.restype = C.c_size_t
    L.b3gs_backward_raw.argtypes = [C.POINTER(B3gsScene), C.POINTER(B3gsRawParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(B3gsRawGrads), C.c_void_p, C.c_int, C.c_void_p]
    L.b3gs_backward_raw.restype = C.c_int
    L.b3gs_backward_raw_accumulate.argtypes = [C.c_int32, C.POINTER(B3gsFusedView), C.POINTER(B3gsRawParams),
                                               C.POINTER(B3gsRawGrads), C.c_int32, C.POINTER(B3gsDensifyStats),
                                               C.c_void_p]
    L.b3gs_backward_raw_accumulate.restype = C.c_int
    L.b3gs_backward_raw_accumulate_range.argtypes = [C.c_int32, C.POINTER(B3gsFusedView), C.POINTER(B3gsRawParams),
                                                     C.POINTER(B3gsRawGrads), C.c_int32, C.POINTER(B3gsDensifyStats),
                                                     C.c_int32, C.c_int32, C.c_void_p]
    L.b3gs_backward_raw_accumulate_range.restype = C.c_int
    L.b3gs_forward_raw_batch.argtypes = [C.c_int32, C.POINTER(B3gsForwardView), C.POINTER(B3gsRawParams), C.c_int,
                                         C.c_void_p]
    L.b3gs_forward_raw_batch.restype = C.c_int
    L.b3gs_loss_workspace_floats.argtypes = [C.c_int32, C.c_int32]
    L.b3gs_loss_workspace_floats.restype = C.c_size_t
    L.b3gs_binocular_loss.argtypes = [C.POINTER(B3gsLossIO), C.c_void_p]
    L.b3gs_binocular_loss.restype = C.c_int
    L.b3gs_binocular_loss_batch.argtypes = [C.c_int32, C.POINTER(B3gsLossIO), C.c_void_p]
    L.b3gs_binocular_loss_batch.restype = C.c_int
    L.b3gs_densify_classify.argtypes = [C.POINTER(B3gsDensifyIO), C.c_void_p, C.c_void_p]
    L.b3gs_densify_classify.restype = C.c_int
    L.b3gs_densify_scatter.argtypes = [C.POINTER(B3gsDensifyIO), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_void_p), C.c_void_p]
    L.b3gs_densify_scatter.restype = C.c_int
    L.b3gs_knn_workspace_bytes.argtypes = [C.c_int32]
    L.b3gs_knn_workspace_bytes.restype = C.c_size_t
    L.b3gs_knn_mean_dist2.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.b3gs_knn_mean_dist2.restype = C.c_int
    L.b3gs_adam_step.argtypes = [C.c_int32, C.POINTER(B3gsAdamSegment), C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.b3gs_adam_step.restype = C.c_int
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.b3gs_lossfn_workspace_floats.argtypes = [I64, I32, I32]
    L.b3gs_lossfn_workspace_floats.restype = C.c_size_t
    L.b3gs_l1_loss_forward.argtypes = [V, V, V, I64, I32, I64, V, V, V]
    L.b3gs_l1_loss_backward.argtypes = [V, V, V, I64, I32, I64, V, V, V, V, V]
    L.b3gs_inverse_warp_forward.argtypes = [V, V, I32, I32, I32, I32, V, V, V]
    L.b3gs_inverse_warp_backward.argtypes = [V, V, V, I32, I32, I32, I32, V, V, V]
    L.b3gs_smooth_loss_forward.argtypes = [V, V, I32, I32, I32, I32, V, V, V]
    L.b3gs_smooth_loss_backward.argtypes = [V, V, I32, I32, I32, I32, V, V, V, V]
    L.b3gs_ssim_forward.argtypes = [V, V, I32, I32, I32, I32, I32, V, I32, V, V, V]
    L.b3gs_ssim_backward.argtypes = [V, V, V, I32, I32, I32, I32, I32, V, V, V, V]
    L.b3gs_opacity_decay.argtypes = [V, I64, F, V]
    L.b3gs_add_densification_stats.argtypes = [I64, V, I64, V, V, V, V]
    L.b3gs_adam_step_at.argtypes = [I32, C.POINTER(B3gsAdamSegment), I32, F, F, F, V]
    for fn in (L.b3gs_l1_loss_forward, L.b3gs_l1_loss_backward, L.b3gs_inverse_warp_forward, L.b3gs_inverse_warp_backward,
               L.b3gs_smooth_loss_forward, L.b3gs_smooth_loss_backward, L.b3gs_ssim_forward, L.b3gs_ssim_backward,
               L.b3gs_opacity_decay, L.b3gs_add_densification_stats, L.b3gs_adam_step_at):
        fn.restype = C.c_int
    L.b3gs_apply_staged_densify_stats.argtypes = [I64] + [V] * 9
    L.b3gs_apply_staged_densify_stats.restype = C.c_int
    L.b3gs_debug_activations.argtypes = [I32, C.POINTER(B3gsRawParams), V, V, V, V]
    L.b3gs_debug_activations.restype = C.c_int
    L.b3gs_image_metrics_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.b3gs_image_metrics_workspace_bytes.restype = C.c_size_t
    L.b3gs_image_metrics_batch.argtypes = [I32, C.POINTER(B3gsMetricView), I32, I32, I32, I32, V, V, V]
    L.b3gs_image_metrics_batch.restype = C.c_int
    L.b3gs_frames_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_frames_workspace_bytes.restype = C.c_size_t
    L.b3gs_encode_frames_batch.argtypes = [I32, C.POINTER(B3gsFrameView), I32, I32, C.c_double, V, V, V, V]
    L.b3gs_encode_frames_batch.restype = C.c_int
    L.b3gs_gt_workspace_bytes.argtypes = [I32, C.POINTER(B3gsGtView), I32, I32]
    L.b3gs_gt_workspace_bytes.restype = C.c_size_t
    L.b3gs_prepare_gt_batch.argtypes = [I32, C.POINTER(B3gsGtView), I32, I32, I32, C.c_float, V, V]
    L.b3gs_prepare_gt_batch.restype = C.c_int
    L.b3gs_cloud_workspace_bytes.argtypes = [I64]
    L.b3gs_cloud_workspace_bytes.restype = C.c_size_t
    L.b3gs_triangulate_matches.argtypes = [I32] + [V] * 8 + [I32, I32, F, V, V, V, V, V]
    L.b3gs_triangulate_matches.restype = C.c_int
    L.b3gs_background_sheet.argtypes = [V, I32, I32, V, V, F, V, V, V, V, V]
    L.b3gs_background_sheet.restype = C.c_int
    L.b3gs_cloud_grow_round.argtypes = [C.POINTER(B3gsCloudGrow), V]
    L.b3gs_cloud_grow_round.restype = C.c_int
    L.b3gs_sweep_workspace_bytes.argtypes = [I32, I32, I32, I32]
    L.b3gs_sweep_workspace_bytes.restype = C.c_size_t
    L.b3gs_sweep_match_pair.argtypes = [C.POINTER(B3gsSweepPair), V]
    L.b3gs_sweep_match_pair.restype = C.c_int
    L.b3gs_jpeg_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_jpeg_workspace_bytes.restype = C.c_size_t
    L.b3gs_jpeg_encode_batch.argtypes = [I32, C.POINTER(C.c_void_p), I32, I32, V, V, I64, V, V, V]
    L.b3gs_jpeg_encode_batch.restype = C.c_int
    L.b3gs_tsdf_integrate_batch.argtypes = [C.POINTER(B3gsTsdfVolume), I32, C.POINTER(B3gsTsdfView), I32, I32, F, F, F, V]
    L.b3gs_tsdf_integrate_batch.restype = C.c_int
    L.b3gs_mesh_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_mesh_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_count.argtypes = [C.POINTER(B3gsTsdfVolume), F, V, V]
    L.b3gs_mesh_count.restype = C.c_int
    L.b3gs_mesh_emit.argtypes = [C.POINTER(B3gsTsdfVolume), V, I64, I64, V, V, V, V]
    L.b3gs_mesh_emit.restype = C.c_int
    L.b3gs_mesh_components.argtypes = [I32, I64, V, V, V, V]
    L.b3gs_mesh_components.restype = C.c_int
    L.b3gs_mesh_clean_workspace_bytes.argtypes = [I64, I64]
    L.b3gs_mesh_clean_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_clean_count.argtypes = [I32, I64, V, V, V, V, V, V]
    L.b3gs_mesh_clean_count.restype = C.c_int
    L.b3gs_mesh_clean_emit.argtypes = [I32, I64, V, V, V, V, V, V, V, I64, I64, V, V, V, V]
    L.b3gs_mesh_clean_emit.restype = C.c_int
    L.b3gs_mesh_sample_workspace_bytes.argtypes = [I64]
    L.b3gs_mesh_sample_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_sample_count.argtypes = [I32, I64, V, V, F, V, V]
    L.b3gs_mesh_sample_count.restype = C.c_int
    L.b3gs_mesh_sample_emit.argtypes = [I32, I64, V, V, F, V, I64, V, V]
    L.b3gs_mesh_sample_emit.restype = C.c_int
    L.b3gs_nearest_workspace_bytes.argtypes = [I64]
    L.b3gs_nearest_workspace_bytes.restype = C.c_size_t
    L.b3gs_nearest_grid.argtypes = [I64, V, F, V, V]
    L.b3gs_nearest_grid.restype = C.c_int
    L.b3gs_nearest_query.argtypes = [I64, V, I64, F, V, V, V]
    L.b3gs_nearest_query.restype = C.c_int
    L.b3gs_cloud_score_workspace_bytes.argtypes = [I64]
    L.b3gs_cloud_score_workspace_bytes.restype = C.c_size_t
    L.b3gs_cloud_score.argtypes = [I64, V, V, F, V, V, V]
    L.b3gs_cloud_score.restype = C.c_int
    L.b3gs_mesh_simplify_workspace_bytes.argtypes = [I64, I64]
    L.b3gs_mesh_simplify_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_simplify_count.argtypes = [I32, I64, V, V, F, V, V]
    L.b3gs_mesh_simplify_count.restype = C.c_int
    L.b3gs_mesh_simplify_emit.argtypes = [I32, I64, V, V, V, F, I32, V, I64, I64, V, V, V, V]
    L.b3gs_mesh_simplify_emit.restype = C.c_int
    L.b3gs_mesh_raster_workspace_bytes.argtypes = [I32, I64, I64, I32, I32]
    L.b3gs_mesh_raster_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_raster_batch.argtypes = [I32, V, I32, I32, I32, I64, V, V, I32, I32, I32, V, V, V]
    L.b3gs_mesh_raster_batch.restype = C.c_int
    L.b3gs_mesh_resolve_batch.argtypes = [I32, V, I32, I32, I32, I64, V, V, V, V, V, I32, V, V, V, V, V, V]
    L.b3gs_mesh_resolve_batch.restype = C.c_int
    L.b3gs_mesh_texture_atlas_height.argtypes = [I64, I32, I32]
    L.b3gs_mesh_texture_atlas_height.restype = I32
    L.b3gs_mesh_texture_accumulate_batch.argtypes = [I32, V, I32, I32, I32, I64, V, V, I32, I32, I32, V, V, V, C.c_float, I32, V, V, V]
    L.b3gs_mesh_texture_accumulate_batch.restype = C.c_int
    L.b3gs_mesh_texture_finalize.argtypes = [I32, I64, V, V, I32, I32, I32, V, V, V, V]
    L.b3gs_mesh_texture_finalize.restype = C.c_int
    L.b3gs_mesh_resolve_textured_batch.argtypes = [I32, V, I32, I32, I32, I64, V, V, V, V, V, I32, I32, I32, V, V, V, V, V, V]
    L.b3gs_mesh_resolve_textured_batch.restype = C.c_int
    L.b3gs_mesh_adjacency_workspace_bytes.argtypes = [I64, I64]
    L.b3gs_mesh_adjacency_workspace_bytes.restype = C.c_size_t
    L.b3gs_mesh_adjacency_layout.argtypes = [I64, I64, C.POINTER(C.c_size_t)]
    L.b3gs_mesh_adjacency_layout.restype = C.c_int
    L.b3gs_mesh_adjacency_build.argtypes = [I32, I64, V, V, V, V]
    L.b3gs_mesh_adjacency_build.restype = C.c_int
    L.b3gs_mesh_smooth.argtypes = [I32, I64, V, V, I32, C.c_double, C.c_double, I32, V, V]
    L.b3gs_mesh_smooth.restype = C.c_int
    L.b3gs_mesh_vertex_normals.argtypes = [I32, I64, V, V, V, V, V]
    L.b3gs_mesh_vertex_normals.restype = C.c_int
    L.b3gs_mesh_resolve_shaded_batch.argtypes = [I32, V, I32, I32, I32, I64, V, V, V, V, I32, V, V, V, V, V, V]
    L.b3gs_mesh_resolve_shaded_batch.restype = C.c_int
    L.b3gs_lpips_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_lpips_workspace_bytes.restype = C.c_size_t
    L.b3gs_lpips_batch.argtypes = [I32, V, V, I32, I32, C.POINTER(B3gsLpipsWeights), I32, V, V, V]
    L.b3gs_lpips_batch.restype = C.c_int
    L.b3gs_lpips_features.argtypes = [I32, V, I32, I32, C.POINTER(B3gsLpipsWeights), I32, C.POINTER(C.c_void_p), V, V]
    L.b3gs_lpips_features.restype = C.c_int
    L.b3gs_blend_contribution_batch.argtypes = [I32, C.POINTER(B3gsContribView), C.POINTER(B3gsContribOut), V]
    L.b3gs_blend_contribution_batch.restype = C.c_int
    L.b3gs_blend_pixel_maps_batch.argtypes = [I32, C.POINTER(B3gsPixelMapView), V]
    L.b3gs_blend_pixel_maps_batch.restype = C.c_int
    L.b3gs_label_votes_batch.argtypes = [I32, C.POINTER(B3gsLabelVoteView), I32, V, V]
    L.b3gs_label_votes_batch.restype = C.c_int
    L.b3gs_label_render_batch.argtypes = [I32, C.POINTER(B3gsLabelRenderView), I32, V, V]
    L.b3gs_label_render_batch.restype = C.c_int
    L.b3gs_feature_render_batch.argtypes = [I32, C.POINTER(B3gsFeatureRenderView), I32, V, V]
    L.b3gs_feature_render_batch.restype = C.c_int
    L.b3gs_feature_lift_batch.argtypes = [I32, C.POINTER(B3gsFeatureLiftView), I32, C.POINTER(C.c_float), V, V, V]
    L.b3gs_feature_lift_batch.restype = C.c_int
    L.b3gs_kmeans_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_kmeans_workspace_bytes.restype = C.c_size_t
    L.b3gs_kmeans_assign.argtypes = [I32, I32, I32, V, V, V, V, V]
    L.b3gs_kmeans_assign.restype = C.c_int
    L.b3gs_kmeans.argtypes = [I32, I32, I32, I32, V, V, V, V, V, V, V, V]
    L.b3gs_kmeans.restype = C.c_int
    L.b3gs_camera_points.argtypes = [C.POINTER(B3gsCameraModel), I32, I64, V, V, V, V]
    L.b3gs_camera_points.restype = C.c_int
    L.b3gs_undistort_map.argtypes = [C.POINTER(B3gsCameraModel), I32, I32, C.c_double, C.c_double, V, V]
    L.b3gs_undistort_map.restype = C.c_int
    L.b3gs_remap_batch.argtypes = [I32, C.POINTER(C.c_void_p), I32, I32, I32, V, I32, I32, C.POINTER(C.c_void_p), V, V]
    L.b3gs_remap_batch.restype = C.c_int
    L.b3gs_transform_points.argtypes = [I64, V, C.POINTER(B3gsSimilarity), V, V]
    L.b3gs_transform_points.restype = C.c_int
    L.b3gs_transform_gaussians.argtypes = [I32, I32, V, V, V, V, C.POINTER(B3gsSimilarity), V, V, V, V, V]
    L.b3gs_transform_gaussians.restype = C.c_int
    L.b3gs_select_gaussians.argtypes = [I32, V, V, V, C.POINTER(B3gsSelect), V, V, V]
    L.b3gs_select_gaussians.restype = C.c_int
    L.b3gs_nearest_query_index.argtypes = [I64, V, I64, F, V, V, V, V]
    L.b3gs_nearest_query_index.restype = C.c_int
    L.b3gs_similarity_sums_workspace_bytes.argtypes = [I64]
    L.b3gs_similarity_sums_workspace_bytes.restype = C.c_size_t
    L.b3gs_similarity_sums.argtypes = [I64, V, I64, V, V, V, F, V, C.POINTER(C.c_double), C.POINTER(C.c_double), V, V, V]
    L.b3gs_similarity_sums.restype = C.c_int
    L.b3gs_gaussian_merge_workspace_bytes.argtypes = [I64, I32]
    L.b3gs_gaussian_merge_workspace_bytes.restype = C.c_size_t
    L.b3gs_gaussian_merge_count.argtypes = [I32, I32, V, V, V, V, V, V, V, F, V, V]
    L.b3gs_gaussian_merge_count.restype = C.c_int
    L.b3gs_gaussian_merge_emit.argtypes = [I32, I32, V, V, V, V, V, V, V, F, V, C.POINTER(C.c_int64), V, V, V, V, V, V, V, V, V]
    L.b3gs_gaussian_merge_emit.restype = C.c_int
    L.b3gs_oriented_points_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_oriented_points_workspace_bytes.restype = C.c_size_t
    L.b3gs_oriented_points_batch.argtypes = [I32, C.POINTER(B3gsTsdfView), I32, I32, I32, F, F, F, I32, V, V]
    L.b3gs_oriented_points_batch.restype = C.c_int
    L.b3gs_oriented_points_emit.argtypes = [I32, C.POINTER(B3gsTsdfView), I32, I32, I32, F, F, F, I32, V, I64, V, V, V, V, V]
    L.b3gs_oriented_points_emit.restype = C.c_int
    L.b3gs_poisson_workspace_bytes.argtypes = [I32, I32, I32, I64]
    L.b3gs_poisson_workspace_bytes.restype = C.c_size_t
    L.b3gs_poisson_splat.argtypes = [C.POINTER(B3gsTsdfVolume), I64, V, V, V, V, V, V, V]
    L.b3gs_poisson_splat.restype = C.c_int
    L.b3gs_poisson_apply.argtypes = [C.POINTER(B3gsTsdfVolume), V, F, V, V, V]
    L.b3gs_poisson_apply.restype = C.c_int
    L.b3gs_poisson_solve.argtypes = [C.POINTER(B3gsTsdfVolume), V, V, F, I32, F, I32, V, V, V, V]
    L.b3gs_poisson_solve.restype = C.c_int
    L.b3gs_poisson_volume.argtypes = [C.POINTER(B3gsTsdfVolume), V, V, I32, V, V]
    L.b3gs_poisson_volume.restype = C.c_int
    L.b3gs_mcmc_random.argtypes = [I64, C.c_uint64, C.c_uint32, C.c_uint32, I32, V, V]
    L.b3gs_mcmc_random.restype = C.c_int
    L.b3gs_mcmc_noise.argtypes = [I32, V, V, V, V, V, C.c_uint64, C.c_uint32, F, F, V, V]
    L.b3gs_mcmc_noise.restype = C.c_int
    L.b3gs_mcmc_workspace_bytes.argtypes = [I32]
    L.b3gs_mcmc_workspace_bytes.restype = C.c_size_t
    L.b3gs_mcmc_relocate.argtypes = [C.POINTER(B3gsMcmcIO), V, V]
    L.b3gs_mcmc_relocate.restype = C.c_int
    L.b3gs_mcmc_views.argtypes = [I32, V, C.POINTER(B3gsMcmcViews)]
    L.b3gs_mcmc_views.restype = C.c_int
    L.b3gs_depth_prior_workspace_bytes.argtypes = [I32, I32, I32]
    L.b3gs_depth_prior_workspace_bytes.restype = C.c_size_t
    L.b3gs_depth_prior_loss_batch.argtypes = [I32, C.POINTER(B3gsDepthPriorIO), V]
    L.b3gs_depth_prior_loss_batch.restype = C.c_int
    L.b3gs_resize_depth_batch.argtypes = [I32, C.POINTER(B3gsDepthResizeIO), V]
    L.b3gs_resize_depth_batch.restype = C.c_int
    L.b3gs_exposure_workspace_bytes.argtypes = [I32, I32]
    L.b3gs_exposure_workspace_bytes.restype = C.c_size_t
    L.b3gs_exposure_apply.argtypes = [I32, C.POINTER(B3gsExposurePlane), V]
    L.b3gs_exposure_apply.restype = C.c_int
    L.b3gs_exposure_backward.argtypes = [I32, C.POINTER(B3gsExposurePlane), V]
    L.b3gs_exposure_backward.restype = C.c_int
    L.b3gs_exposure_fit.argtypes = [I32, C.POINTER(B3gsExposureFitIO), V]
    L.b3gs_exposure_fit.restype = C.c_int
    L.b3gs_exposure_adam.argtypes = [I32, V, V, V, V, V, V, V, V, C.c_double, C.c_double, C.c_double, V, V]
    L.b3gs_exposure_adam.restype = C.c_int
    L.b3gs_normal_prior_workspace_bytes.argtypes = [I32, I32]
    L.b3gs_normal_prior_workspace_bytes.restype = C.c_size_t
    L.b3gs_normal_prior_loss_batch.argtypes = [I32, C.POINTER(B3gsNormalPriorIO), V]
    L.b3gs_normal_prior_loss_batch.restype = C.c_int
    L.b3gs_depth_normals_batch.argtypes = [I32, C.POINTER(B3gsDepthNormalsIO), V]
    L.b3gs_depth_normals_batch.restype = C.c_int
    L.b3gs_resize_normals_batch.argtypes = [I32, C.POINTER(B3gsNormalResizeIO), V]
    L.b3gs_resize_normals_batch.restype = C.c_int
    L.b3gs_pose_gradient_workspace_bytes.argtypes = [I32, I32]
    L.b3gs_pose_gradient_workspace_bytes.restype = C.c_size_t
    L.b3gs_pose_gradient.argtypes = [I32, I32, I32, V, V, V, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_double), V, V, V]
    L.b3gs_pose_gradient.restype = C.c_int
    L.b3gs_mark_visible.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.b3gs_mark_visible.restype = C.c_int
    L.b3gs_debug_views.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(B3gsDebugViews)]
    L.b3gs_debug_views.restype = C.c_int
    if L.b3gs_abi_version() != ABI_VERSION:
        raise B3gsError(f"libb3gs_raster.so ABI {L.b3gs_abi_version()} != binding {ABI_VERSION}: rebuild")
    _lib = L
    return L


def check(rc: int, what: str) -> None:
    if rc != OK:
        msg = lib().b3gs_last_error().decode("utf-8", "replace")
        raise B3gsError(f"{what} failed: {ERR_NAMES.get(rc, rc)}: {msg}")
