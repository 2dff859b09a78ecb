"""ctypes binding of libnicer_slam_amd.so (the C ABI in include/nicer_slam_amd.h).

There is NO fallback: if the library is missing the import fails, so nothing above it can silently run
without the HIP kernels.
"""
import ctypes
import os

# PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7 -- the same
# SONAME as /opt/rocm's).  Whichever is loaded first serves the whole process, so torch must come first: our kernels
# then launch on the very runtime that owns torch's allocations and streams.  (Loading this library first made
# every launch fail on the GPU box.)
import torch  # noqa: F401  (must precede the CDLL below)

# NSA_LIB_TAG selects a side-by-side experiment build of the same library (nicer_slam_amd/build.py, NSA_BUILD_TAG);
# unset = the product library.  Either way it is the HIP library or nothing.
_TAG = os.environ.get("NSA_LIB_TAG", "")
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                         "libnicer_slam_amd" + ("_" + _TAG if _TAG else "") + ".so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"{_LIB_PATH} not found: the HIP extension has not been built.  Run "
        "`python -m nicer_slam_amd.build` (needs hipcc; cross-compiles gfx950 without a GPU).")

lib = ctypes.CDLL(_LIB_PATH)

_p, _u32, _f32, _i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_int

lib.nsa_strerror.restype = ctypes.c_char_p
lib.nsa_strerror.argtypes = [_i]
lib.nsa_version.restype = _i
lib.nsa_hash_encode_forward.restype = _i
lib.nsa_hash_encode_forward.argtypes = [_p, _p, _p, _p, _u32, _u32, _u32, _u32, _f32, _u32, _i, _p, _p]
lib.nsa_hash_encode_backward.restype = _i
lib.nsa_hash_encode_backward.argtypes = [_p, _p, _p, _p, _p, _u32, _u32, _u32, _u32, _f32, _u32, _i, _p, _p, _p]
lib.nsa_hash_encode_second_backward.restype = _i
lib.nsa_hash_encode_second_backward.argtypes = [_p, _p, _p, _p, _u32, _u32, _u32, _u32, _f32, _u32, _i, _p, _p,
                                                _p, _p, _p]

EXPORTS = ["nsa_strerror", "nsa_version", "nsa_hash_encode_forward", "nsa_hash_encode_backward",
           "nsa_hash_encode_second_backward"]


def check(rc):
    if rc != 0:
        raise RuntimeError(lib.nsa_strerror(rc).decode())


class GridDesc(ctypes.Structure):
    """nsa_grid_t"""
    _fields_ = [("table", _p), ("offsets_host", _p), ("L", _u32), ("C", _u32), ("S", _f32), ("H", _u32),
                ("divide_factor", _f32), ("n_hidden", _u32), ("precision", _u32), ("tile", _u32)]


_gp = ctypes.POINTER(GridDesc)
lib.nsa_sampler_sdf.restype = _i
lib.nsa_sampler_sdf.argtypes = [_p, _p, _u32, _u32, _p, _p, _f32, _f32, _f32, _gp, _gp, _p, _p, _p, _p, _p, _p]
lib.nsa_sample_rays.restype = _i
lib.nsa_sample_rays.argtypes = [_p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _u32, _p, _p, _u32, _f32, _p, _p, _p, _p]
EXPORTS += ["nsa_sampler_sdf", "nsa_sample_rays"]


class PointsDesc(ctypes.Structure):
    """nsa_points_t"""
    _fields_ = [("rays_o", _p), ("rays_d", _p), ("z_vals", _p), ("points", _p), ("P", _u32), ("S", _u32), ("order", _p)]


_pp = ctypes.POINTER(PointsDesc)
lib.nsa_sdfnet_forward.restype = _i
lib.nsa_sdfnet_forward.argtypes = [_pp, _gp, _p, _i, _p, _p, _p, _p]
lib.nsa_sdfnet_forward_pair.restype = _i
lib.nsa_sdfnet_forward_pair.argtypes = [_pp, _gp, _gp, _p, _p, _p, _p, _p, _p]
lib.nsa_sdfnet_backward.restype = _i
lib.nsa_sdfnet_backward.argtypes = [_pp, _gp, _p, _p, _p, _p, _i, _p, _p]
lib.nsa_colour_forward.restype = _i
lib.nsa_colour_forward.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _p]
lib.nsa_colour_backward.restype = _i
lib.nsa_colour_backward.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p]
lib.nsa_composite_forward.restype = _i
lib.nsa_composite_forward.argtypes = [_p, _p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _p, _p, _p, _p, _p, _p]
lib.nsa_composite_backward.restype = _i
lib.nsa_composite_backward.argtypes = [_p, _p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p]
lib.nsa_rays_backward.restype = _i
lib.nsa_rays_backward.argtypes = [_p, _p, _p, _u32, _u32, _p, _p, _p]
lib.nsa_sdfnet_backward_params.restype = _i
lib.nsa_sdfnet_backward_params.argtypes = [_pp, _gp, _p, _p, _p, _p, _i, _p, _p, _p, _u32, _p]
lib.nsa_colour_forward_composite.restype = _i
lib.nsa_colour_forward_composite.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _p, _p, _u32, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_colour_forward_composite"]
lib.nsa_colour_forward_track.restype = _i
lib.nsa_colour_forward_track.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _p, _p, _u32, _p, _u32, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_colour_forward_track"]
lib.nsa_colour_coarse_backward.restype = _i
lib.nsa_colour_coarse_backward.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _gp, _p, _p, _p]
EXPORTS += ["nsa_colour_coarse_backward"]
lib.nsa_colour_backward_params.restype = _i
lib.nsa_colour_backward_params.argtypes = [_pp, _gp, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _p, _u32, _p]
lib.nsa_sdfnet_emit_rows.restype = _i
lib.nsa_sdfnet_emit_rows.argtypes = []
lib.nsa_colour_emit_rows.restype = _i
lib.nsa_colour_emit_rows.argtypes = []
lib.nsa_sdfnet_emit_rows_nh.restype = _i
lib.nsa_sdfnet_emit_rows_nh.argtypes = [_u32]
lib.nsa_sdfnet_emit_rows_tile.restype = _i
lib.nsa_sdfnet_emit_rows_tile.argtypes = [_u32, _u32]
EXPORTS += ["nsa_sdfnet_backward_params", "nsa_colour_backward_params", "nsa_sdfnet_emit_rows", "nsa_colour_emit_rows",
            "nsa_sdfnet_emit_rows_nh", "nsa_sdfnet_emit_rows_tile"]
EXPORTS += ["nsa_sdfnet_forward", "nsa_sdfnet_forward_pair", "nsa_sdfnet_backward", "nsa_colour_forward", "nsa_colour_backward",
            "nsa_composite_forward", "nsa_composite_backward", "nsa_rays_backward"]

lib.nsa_rays_forward.restype = _i
lib.nsa_rays_forward.argtypes = [_p, _p, _p, _u32, _u32, _p, _p, _p, _p]
lib.nsa_rays_pose_backward.restype = _i
lib.nsa_rays_pose_backward.argtypes = [_p, _p, _p, _u32, _u32, _p, _p, _p, _p]
lib.nsa_rays_forward_draw.restype = _i
lib.nsa_rays_forward_draw.argtypes = [_p, _p, _p, _u32, _u32, _p, _p, _p, _p, ctypes.c_uint64, _p, _u32, _u32, _u32, _p, _p]
EXPORTS += ["nsa_rays_forward", "nsa_rays_forward_draw", "nsa_rays_pose_backward"]

lib.nsa_cam_to_pose.restype = _i
lib.nsa_cam_to_pose.argtypes = [_p, _u32, _p, _p]
lib.nsa_pose_grad_to_cam.restype = _i
lib.nsa_pose_grad_to_cam.argtypes = [_p, _p, _u32, _p, _p]
lib.nsa_l1_loss.restype = _i
lib.nsa_l1_loss.argtypes = [_p, _p, _u32, _p, _p, _p]
lib.nsa_adam_step.restype = _i
lib.nsa_adam_step.argtypes = [_p, _p, _p, _p, _p, _u32, _f32, _f32, _f32, _f32, _u32, _f32, _p]
EXPORTS += ["nsa_cam_to_pose", "nsa_pose_grad_to_cam", "nsa_l1_loss", "nsa_adam_step"]

lib.nsa_update_voxels.restype = _i
lib.nsa_update_voxels.argtypes = [_pp, _p, _u32, _p]
lib.nsa_adam_table_step.restype = _i
lib.nsa_adam_table_step.argtypes = [_p, _p, _p, _p, ctypes.c_uint64, _u32, _f32, _f32, _f32, _f32, _p]
lib.nsa_adam_table_step_clear.restype = _i
lib.nsa_adam_table_step_clear.argtypes = lib.nsa_adam_table_step.argtypes
lib.nsa_adam_table_step_zero_grad.restype = _i
lib.nsa_adam_table_step_zero_grad.argtypes = [_p, _p, _p, ctypes.c_uint64, _u32, _f32, _f32, _f32, _f32, _p]
EXPORTS += ["nsa_update_voxels", "nsa_adam_table_step", "nsa_adam_table_step_clear", "nsa_adam_table_step_zero_grad"]


class WnLayer(ctypes.Structure):
    """nsa_wn_layer_t"""
    _fields_ = [("weight_v", _p), ("weight_g", _p), ("bias", _p), ("rows", _u32), ("cols", _u32)]


lib.nsa_weight_norm_flat.restype = _i
lib.nsa_weight_norm_flat.argtypes = [ctypes.POINTER(WnLayer), _u32, _p, _p, _p]
lib.nsa_weight_norm_flat_backward.restype = _i
lib.nsa_weight_norm_flat_backward.argtypes = [ctypes.POINTER(WnLayer), _u32, _p, _p, _p, _p]
lib.nsa_emit_row.restype = _i
lib.nsa_emit_row.argtypes = [_p, _p, _p, _u32, ctypes.c_uint64, _f32, _p]
class AdamSeg(ctypes.Structure):
    """nsa_adam_seg_t"""
    _fields_ = [("param", _p), ("grad", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("n", _u32), ("step", _u32), ("lr", _f32)]


lib.nsa_adam_multi_step.restype = _i
lib.nsa_adam_multi_step.argtypes = [ctypes.POINTER(AdamSeg), _u32, _f32, _f32, _f32, _p]
EXPORTS += ["nsa_adam_multi_step"]
lib.nsa_fill_zero.restype = _i
lib.nsa_fill_zero.argtypes = [_p, ctypes.c_uint64, _p]
EXPORTS += ["nsa_weight_norm_flat", "nsa_weight_norm_flat_backward", "nsa_emit_row", "nsa_fill_zero"]

lib.nsa_emit_gemm.restype = _i
lib.nsa_emit_gemm.argtypes = [_p, ctypes.c_uint64, _u32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), _u32,
                              _u32, ctypes.c_int, _p, _p, _p]
lib.nsa_emit_gemm_workspace.restype = ctypes.c_uint64
lib.nsa_emit_gemm_workspace.argtypes = [ctypes.c_uint64, _u32, _u32, ctypes.c_int]
EXPORTS += ["nsa_emit_gemm", "nsa_emit_gemm_workspace"]
lib.nsa_pack_blocks.restype = _i
lib.nsa_pack_blocks.argtypes = [_p, _p, ctypes.c_uint64, _p, ctypes.c_uint64, _p, ctypes.c_uint64, _p, _p]
lib.nsa_operand_form.restype = _i
lib.nsa_operand_form.argtypes = []
EXPORTS += ["nsa_pack_blocks", "nsa_operand_form"]


class FeedField(ctypes.Structure):
    """nsa_feed_field_t"""
    _fields_ = [("store", _p), ("out", _p), ("channels", _u32)]


class CopySeg(ctypes.Structure):
    """nsa_copy_seg_t"""
    _fields_ = [("dst", _p), ("src", _p), ("n", _u32)]


lib.nsa_copy_segments.restype = _i
lib.nsa_copy_segments.argtypes = [ctypes.POINTER(CopySeg), _u32, _p]
EXPORTS += ["nsa_copy_segments"]
lib.nsa_feed_gather.restype = _i
lib.nsa_feed_gather.argtypes = [ctypes.POINTER(FeedField), _u32, _p, _u32, _p, _u32, ctypes.c_uint64, _u32, _p, _p]
EXPORTS += ["nsa_feed_gather"]

class LossDesc(ctypes.Structure):
    """nsa_loss_t"""
    _fields_ = ([("bs", _u32), ("n", _u32), ("S", _u32), ("E", _u32)]
                + [(k, _p) for k in ("rgb", "rgb_gt", "depth", "depth_mono", "depth_real", "depth_real_mask", "mask_gt", "sdf",
                                     "normal", "normal_gt", "grad_theta", "grad_theta_nei")]
                + [(k, _f32) for k in ("w_rgb", "w_eik", "w_smooth", "w_depth", "w_gtdepth", "w_nl1", "w_ncos")]
                + [("depth_whole_image", ctypes.c_int)]
                + [(k, _p) for k in ("g_rgb", "g_depth", "g_normal", "g_theta", "g_theta_nei", "terms")])


lib.nsa_slam_loss.restype = _i
lib.nsa_slam_loss.argtypes = [ctypes.POINTER(LossDesc), _p, _p]
lib.nsa_slam_loss_workspace.restype = ctypes.c_uint64
lib.nsa_slam_loss_workspace.argtypes = [_u32, _u32, _u32]
EXPORTS += ["nsa_slam_loss", "nsa_slam_loss_workspace"]

lib.nsa_sdf_points.restype = _i
lib.nsa_sdf_points.argtypes = [_p, ctypes.c_uint64, _gp, _gp, _p, _p, _p, _p]
EXPORTS += ["nsa_sdf_points"]

lib.nsa_draw_picks.restype = _i
lib.nsa_draw_picks.argtypes = [_p, _u32, _u32, _u32, _u32, _p, _p, _p]
lib.nsa_draw.restype = _i
lib.nsa_draw.argtypes = [_p, ctypes.c_uint64, _p, _u32, _u32, _u32, _u32, _p, _p, _p]
EXPORTS += ["nsa_draw_picks", "nsa_draw"]

lib.nsa_track_head.restype = _i
lib.nsa_track_head.argtypes = [_p, _p, _p, _u32, _p, _p, _p, _p, _p]
lib.nsa_track_tail.restype = _i
lib.nsa_track_tail.argtypes = [_p, _p, _p, _u32, _p, _p, _p, _i, _f32, _p, _p, _p, _f32, _f32, _f32, _f32, _u32, _f32, _p, _p,
                               _p]
EXPORTS += ["nsa_track_head", "nsa_track_tail"]
lib.nsa_track_begin.restype = _i
lib.nsa_track_begin.argtypes = [_p, _p, _p, _p, _p, _p, _u32, _p, _p, _p, _p, _p]
lib.nsa_composite_track.restype = _i
lib.nsa_composite_track.argtypes = [_p, _p, _p, _p, _p, _p, _u32, _u32, _u32, _p, _u32, _p, _p, _p, _p, _p, _p]
lib.nsa_track_finish.restype = _i
lib.nsa_track_finish.argtypes = [_p, _p, _p, _u32, _u32, _p, _p, _p, _p, _p, _i, _f32, _p, _p, _p, _f32, _f32, _f32, _f32, _u32,
                                 _f32, _p, _p, _p]
lib.nsa_track_finish_workspace.restype = ctypes.c_uint64
lib.nsa_track_finish_workspace.argtypes = [_u32]
lib.nsa_track_begin_draw.restype = _i
lib.nsa_track_begin_draw.argtypes = [_p, _p, _p, _p, _p, _p, _u32, _p, _p, _p, _p, _p, ctypes.c_uint64, _p, _u32, _u32, _u32, _p, _p]
EXPORTS += ["nsa_track_begin", "nsa_track_begin_draw", "nsa_composite_track", "nsa_track_finish", "nsa_track_finish_workspace"]

lib.nsa_morton_keys.restype = _i
lib.nsa_morton_keys.argtypes = [_pp, _p, _p]
lib.nsa_morton_order.restype = _i
lib.nsa_morton_order.argtypes = [_pp, _p, _p, _u32, _p]
lib.nsa_morton_order_workspace.restype = ctypes.c_uint64
lib.nsa_morton_order_workspace.argtypes = [_u32]
EXPORTS += ["nsa_morton_order", "nsa_morton_order_workspace"]
EXPORTS += ["nsa_morton_keys"]

lib.nsa_adam_step_scaled.restype = _i
lib.nsa_adam_step_scaled.argtypes = [_p, _p, _p, _p, _p, _p, _u32, _f32, _f32, _f32, _f32, _u32, _f32, _p, _p, _p]
EXPORTS += ["nsa_adam_step_scaled"]


class WarpDesc(ctypes.Structure):
    """nsa_warp_t"""
    _fields_ = ([("b", _u32), ("n", _u32), ("H", _u32), ("W", _u32)]
                + [(k, _p) for k in ("uv", "pose", "w2c", "K", "depth", "images", "depths", "frame_index")])


_wp, _u64 = ctypes.POINTER(WarpDesc), ctypes.c_uint64
lib.nsa_patch_warp_forward.restype = _i
lib.nsa_patch_warp_forward.argtypes = [_wp, _u32, _p, _p, _p, _p, _p]
lib.nsa_patch_warp_backward.restype = _i
lib.nsa_patch_warp_backward.argtypes = [_wp, _u32, _p, _p, _p, _p, _p, _p]
lib.nsa_patch_warp_workspace.restype = _u64
lib.nsa_patch_warp_workspace.argtypes = [_u32, _u32, _u32, _i]
lib.nsa_flow_forward.restype = _i
lib.nsa_flow_forward.argtypes = [_wp, _p, _p, _u32, _p, _p]
lib.nsa_flow_backward.restype = _i
lib.nsa_flow_backward.argtypes = [_wp, _p, _p, _u32, _p, _p, _p, _p, _p, _p]
lib.nsa_flow_workspace.restype = _u64
lib.nsa_flow_workspace.argtypes = [_u32, _u32, _u32, _i]
lib.nsa_masked_l1.restype = _i
lib.nsa_masked_l1.argtypes = [_p, _p, _p, _u64, _u32, _p, _p, _p, _p]
lib.nsa_masked_l1_workspace.restype = _u64
lib.nsa_masked_l1_workspace.argtypes = [_u64]
EXPORTS += ["nsa_patch_warp_forward", "nsa_patch_warp_backward", "nsa_patch_warp_workspace", "nsa_flow_forward",
            "nsa_flow_backward", "nsa_flow_workspace", "nsa_masked_l1", "nsa_masked_l1_workspace"]
lib.nsa_patch_ssim.restype = _i
lib.nsa_patch_ssim.argtypes = [_p, _p, _p, _u64, _u32, _p, _p, _p, _p]
lib.nsa_patch_ssim_workspace.restype = _u64
lib.nsa_patch_ssim_workspace.argtypes = [_u64]
EXPORTS += ["nsa_patch_ssim", "nsa_patch_ssim_workspace"]

lib.nsa_marching_cubes_workspace.restype = _u64
lib.nsa_marching_cubes_workspace.argtypes = [_u32, _u32, _u32]
lib.nsa_marching_cubes_count.restype = _i
lib.nsa_marching_cubes_count.argtypes = [_p, _u32, _u32, _u32, _f32, _p, _p, _p]
lib.nsa_marching_cubes_emit.restype = _i
lib.nsa_marching_cubes_emit.argtypes = [_p, _u32, _u32, _u32, _f32, ctypes.POINTER(_f32), ctypes.POINTER(_f32), _p, _u64, _u64, _p,
                                        _p, _p, _p]
EXPORTS += ["nsa_marching_cubes_workspace", "nsa_marching_cubes_count", "nsa_marching_cubes_emit"]

lib.nsa_nn_workspace.restype = _u64
lib.nsa_nn_workspace.argtypes = [_u32]
lib.nsa_nn_build.restype = _i
lib.nsa_nn_build.argtypes = [_p, _u32, _p, _p]
lib.nsa_nn_query.restype = _i
lib.nsa_nn_query.argtypes = [_p, _u32, _p, _u32, ctypes.c_double, _p, _p, _p]
lib.nsa_surface_sample_workspace.restype = _u64
lib.nsa_surface_sample_workspace.argtypes = [_u32]
lib.nsa_surface_sample.restype = _i
lib.nsa_surface_sample.argtypes = [_p, _u32, _p, _u32, _u32, _u64, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_nn_workspace", "nsa_nn_build", "nsa_nn_query", "nsa_surface_sample_workspace", "nsa_surface_sample"]

lib.nsa_image_metrics_workspace.restype = _u64
lib.nsa_image_metrics_workspace.argtypes = [_u32, _u32, _u32]
lib.nsa_image_metrics.restype = _i
lib.nsa_image_metrics.argtypes = [_p, _p, _u32, _u32, _u32, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_image_metrics_workspace", "nsa_image_metrics"]


class TsdfVolumeDesc(ctypes.Structure):
    """nsa_tsdf_volume_t"""
    _fields_ = [("tsdf", _p), ("weight", _p), ("colour", _p), ("nx", _u32), ("ny", _u32), ("nz", _u32), ("origin", _f32 * 3),
                ("voxel_length", _f32), ("sdf_trunc", _f32)]


_tp = ctypes.POINTER(TsdfVolumeDesc)
lib.nsa_tsdf_integrate.restype = _i
lib.nsa_tsdf_integrate.argtypes = [_tp, _p, _p, _p, _p, _i, _u32, _u32, _u32, _f32, _p, _p]
lib.nsa_tsdf_sample_colour.restype = _i
lib.nsa_tsdf_sample_colour.argtypes = [_tp, _p, _u64, _p, _p]
EXPORTS += ["nsa_tsdf_integrate", "nsa_tsdf_sample_colour"]

lib.nsa_mesh_components_workspace.restype = _u64
lib.nsa_mesh_components_workspace.argtypes = [_u32]
lib.nsa_mesh_components.restype = _i
lib.nsa_mesh_components.argtypes = [_p, _u32, _u32, _p, _p, _p, _p, _p]
lib.nsa_mesh_component_stats_workspace.restype = _u64
lib.nsa_mesh_component_stats_workspace.argtypes = [_u32, _u32, _u32]
lib.nsa_mesh_component_stats.restype = _i
lib.nsa_mesh_component_stats.argtypes = [_p, _u32, _p, _u32, _p, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_components_workspace", "nsa_mesh_components", "nsa_mesh_component_stats_workspace",
            "nsa_mesh_component_stats"]


class RasterViews(ctypes.Structure):
    """nsa_raster_views_t"""
    _fields_ = [("w2c", _p), ("K", _p), ("n", _u32), ("K_per_view", _i), ("H", _u32), ("W", _u32), ("near", _f32)]


_rv = ctypes.POINTER(RasterViews)
lib.nsa_mesh_raster_workspace.restype = _u64
lib.nsa_mesh_raster_workspace.argtypes = [_u32]
lib.nsa_mesh_raster.restype = _i
lib.nsa_mesh_raster.argtypes = [_p, _u32, _p, _u32, _p, _u32, _u32, _rv, _i, _i, _u32, _p, _u32, _p, _p, _p]
lib.nsa_mesh_raster_resolve.restype = _i
lib.nsa_mesh_raster_resolve.argtypes = [_p, _u32, _p, _u32, _p, _p, _u32, _p, _u32, _rv, _p, _i, _p, _p, _p, _p, _p, _p]
lib.nsa_mesh_visible.restype = _i
lib.nsa_mesh_visible.argtypes = [_p, _u32, _p, _u32, _rv, _p, _i, _f32, _p, _p]
EXPORTS += ["nsa_mesh_raster_workspace", "nsa_mesh_raster", "nsa_mesh_raster_resolve", "nsa_mesh_visible"]

_f64 = ctypes.c_double
lib.nsa_flowcue_induced.restype = _i
lib.nsa_flowcue_induced.argtypes = [_p, _u32, _u32, _u32, _p, _i, _p, _p, _p, _u32, _f64, _p, _p, _p]
lib.nsa_flowcue_consistency.restype = _i
lib.nsa_flowcue_consistency.argtypes = [_p, _p, _p, _p, _u32, _u32, _u32, _f64, _f64, _p, _p, _p]
lib.nsa_flowcue_select.restype = _i
lib.nsa_flowcue_select.argtypes = [_p, _p, _u32, _u64, _p, _u32, _u32, _p, _p, _p, _p]
EXPORTS += ["nsa_flowcue_induced", "nsa_flowcue_consistency", "nsa_flowcue_select"]

lib.nsa_tri_workspace.restype = _u64
lib.nsa_tri_workspace.argtypes = [_u32]
lib.nsa_tri_build.restype = _i
lib.nsa_tri_build.argtypes = [_p, _u32, _p, _u32, _p, _p, _p]
lib.nsa_tri_query.restype = _i
lib.nsa_tri_query.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, _p, _p, _p, _p]
lib.nsa_tri_query_counted.restype = _i
lib.nsa_tri_query_counted.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_tri_workspace", "nsa_tri_build", "nsa_tri_query", "nsa_tri_query_counted"]
lib.nsa_tri_adjacency_workspace.restype = _u64
lib.nsa_tri_adjacency_workspace.argtypes = [_u32, _u32]
lib.nsa_tri_adjacency_build.restype = _i
lib.nsa_tri_adjacency_build.argtypes = [_p, _u32, _p, _p, _u32, _p, _p]
lib.nsa_tri_signed_query.restype = _i
lib.nsa_tri_signed_query.argtypes = [_p, _p, _p, _u32, _p, _p, _u32, _p, _u32, ctypes.c_double, _i, _p, _p, _p, _p, _p, _p]
lib.nsa_tri_signed_query_counted.restype = _i
lib.nsa_tri_signed_query_counted.argtypes = [_p, _p, _p, _u32, _p, _p, _u32, _p, _u32, ctypes.c_double, _i, _p, _p, _p, _p, _p,
                                             _p, _p, _p, _p, _p]
lib.nsa_tri_query_bounded.restype = _i
lib.nsa_tri_query_bounded.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, ctypes.c_double, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_tri_adjacency_workspace", "nsa_tri_adjacency_build", "nsa_tri_signed_query", "nsa_tri_signed_query_counted",
            "nsa_tri_query_bounded"]
lib.nsa_tri_winding_workspace.restype = _u64
lib.nsa_tri_winding_workspace.argtypes = [_u32]
lib.nsa_tri_winding_build.restype = _i
lib.nsa_tri_winding_build.argtypes = [_p, _u32, _p, _u32, _p, _p, _p]
lib.nsa_tri_winding_query.restype = _i
lib.nsa_tri_winding_query.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, ctypes.c_double, _i, _p, _p, _p, _p]
EXPORTS += ["nsa_tri_winding_workspace", "nsa_tri_winding_build", "nsa_tri_winding_query"]
lib.nsa_tri_ray_workspace.restype = _u64
lib.nsa_tri_ray_workspace.argtypes = [_u32]
lib.nsa_tri_ray_build.restype = _i
lib.nsa_tri_ray_build.argtypes = [_p, _u32, _p, _u32, _p, _p, _p]
lib.nsa_tri_ray_cast.restype = _i
lib.nsa_tri_ray_cast.argtypes = [_p, _p, _u32, _p, _u32, _p, _p, _u32, ctypes.c_double, ctypes.c_double, _u32, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_tri_ray_workspace", "nsa_tri_ray_build", "nsa_tri_ray_cast"]
RAY_ANY_HIT, RAY_CULL_BACK, RAY_CULL_FRONT, RAY_BRUTE = 1, 2, 4, 8          # NSA_RAY_* of header Section 17
lib.nsa_mesh_edges_workspace.restype = _u64
lib.nsa_mesh_edges_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_edges.restype = _i
lib.nsa_mesh_edges.argtypes = [_p, _u32, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
lib.nsa_mesh_face_components_workspace.restype = _u64
lib.nsa_mesh_face_components_workspace.argtypes = [_u32]
lib.nsa_mesh_face_components.restype = _i
lib.nsa_mesh_face_components.argtypes = [_p, _p, _p, _u32, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_edges_workspace", "nsa_mesh_edges", "nsa_mesh_face_components_workspace", "nsa_mesh_face_components"]
lib.nsa_mesh_cluster_workspace.restype = _u64
lib.nsa_mesh_cluster_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_cluster.restype = _i
lib.nsa_mesh_cluster.argtypes = [_p, _u32, _p, _u32, ctypes.POINTER(_f64), _f64, _u32, _p, _p, _p, _p, _p, _p, _p, _p]
lib.nsa_mesh_cluster_place_workspace.restype = _u64
lib.nsa_mesh_cluster_place_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_cluster_place.restype = _i
lib.nsa_mesh_cluster_place.argtypes = [_p, _u32, _p, _u32, _p, _p, ctypes.POINTER(_f64), _f64, _f64, _i, _p, _p, _u32, _p, _p, _p,
                                       _p, _p, _p]
EXPORTS += ["nsa_mesh_cluster_workspace", "nsa_mesh_cluster", "nsa_mesh_cluster_place_workspace", "nsa_mesh_cluster_place"]
lib.nsa_mesh_orient_workspace.restype = _u64
lib.nsa_mesh_orient_workspace.argtypes = [_u32]
lib.nsa_mesh_orient.restype = _i
lib.nsa_mesh_orient.argtypes = [_p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
lib.nsa_mesh_orient_volume_workspace.restype = _u64
lib.nsa_mesh_orient_volume_workspace.argtypes = [_u32]
lib.nsa_mesh_orient_volume.restype = _i
lib.nsa_mesh_orient_volume.argtypes = [_p, _u32, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_orient_workspace", "nsa_mesh_orient", "nsa_mesh_orient_volume_workspace", "nsa_mesh_orient_volume"]
lib.nsa_mesh_ring_workspace.restype = _u64
lib.nsa_mesh_ring_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_ring.restype = _i
lib.nsa_mesh_ring.argtypes = [_p, _p, _u32, _u32, _p, _p, _p, _p, _p]
lib.nsa_mesh_smooth_workspace.restype = _u64
lib.nsa_mesh_smooth_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_smooth.restype = _i
lib.nsa_mesh_smooth.argtypes = [_p, _u32, _u32, _p, _p, _p, _p, _p, ctypes.POINTER(_f64), _u32, _i, _f64, _p, _p, _p, _p]
lib.nsa_mesh_vertex_normals_workspace.restype = _u64
lib.nsa_mesh_vertex_normals_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_vertex_normals.restype = _i
lib.nsa_mesh_vertex_normals.argtypes = [_p, _u32, _p, _u32, _i, _p, _p, _p]
EXPORTS += ["nsa_mesh_ring_workspace", "nsa_mesh_ring", "nsa_mesh_smooth_workspace", "nsa_mesh_smooth",
            "nsa_mesh_vertex_normals_workspace", "nsa_mesh_vertex_normals"]
SMOOTH_FREE, SMOOTH_FIXED, SMOOTH_CURVE = 0, 1, 2                           # NSA_SMOOTH_* of header Section 21
NORMALS_AREA, NORMALS_ANGLE = 0, 1                                          # NSA_NORMALS_*
lib.nsa_mesh_decimate_state_bytes.restype = _u64
lib.nsa_mesh_decimate_state_bytes.argtypes = [_u32]
lib.nsa_mesh_decimate_workspace.restype = _u64
lib.nsa_mesh_decimate_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_decimate_init.restype = _i
lib.nsa_mesh_decimate_init.argtypes = [_p, _p, _u32, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _i, _f64, _p, _p, _p]
lib.nsa_mesh_decimate_round.restype = _i
lib.nsa_mesh_decimate_round.argtypes = [_u32, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _u32, _i, _u64, _i, _f64, _f64, _f64, _i, _p, _p,
                                        _p, _u32, _p, _p]
lib.nsa_mesh_decimate_finish.restype = _i
lib.nsa_mesh_decimate_finish.argtypes = [_p, _p, _u32, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_decimate_state_bytes", "nsa_mesh_decimate_workspace", "nsa_mesh_decimate_init", "nsa_mesh_decimate_round",
            "nsa_mesh_decimate_finish"]
DECIMATE_BOUNDARY_QUADRIC, DECIMATE_BOUNDARY_FIXED = 0, 1                   # NSA_DECIMATE_BOUNDARY_* of header Section 22
lib.nsa_mesh_fill_workspace.restype = _u64
lib.nsa_mesh_fill_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_fill_loops.restype = _i
lib.nsa_mesh_fill_loops.argtypes = [_p, _p, _u32, _p, _p, _u32, _p, _p, _p, _p, _p, _p, _u32, _i, _u64, _i, _f64, _u32, _u32, _i, _p, _p, _p, _p,
                                    _p, _p, _p, _p, _p, _p, _p]
lib.nsa_mesh_fill_emit.restype = _i
lib.nsa_mesh_fill_emit.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, _p, _p, _p, _u64, _u64, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_fill_workspace", "nsa_mesh_fill_loops", "nsa_mesh_fill_emit"]
FILL_CLASSES = ("filled", "nonfinite", "pinched", "too_many_edges", "too_large", "folded")         # NSA_FILL_* of header Section 23
lib.nsa_mesh_fill_area_plan.restype = _i
lib.nsa_mesh_fill_area_plan.argtypes = [_p, _p, _u32, _u32, _u32, _u32, _p, _p, _p]
lib.nsa_mesh_fill_area_workspace.restype = _u64
lib.nsa_mesh_fill_area_workspace.argtypes = [_u64, _u64]
lib.nsa_mesh_fill_area_tables.restype = _i
lib.nsa_mesh_fill_area_tables.argtypes = [_p, _u32, _p, _p, _u32, _p, _p, _p, _u32, _p, _p, _p, _u64, _u64, _u32, _u64, _f64, _p, _p, _p, _p, _p]
lib.nsa_mesh_fill_area_roots.restype = _i
lib.nsa_mesh_fill_area_roots.argtypes = [_p, _u64, _p, _p]
EXPORTS += ["nsa_mesh_fill_area_plan", "nsa_mesh_fill_area_workspace", "nsa_mesh_fill_area_tables", "nsa_mesh_fill_area_roots"]
FILL_AREA_CLASSES = ("area_filled", "area_too_many_edges", "no_triangulation")                      # NSA_FILL_AREA_* of header Section 24
lib.nsa_tri_isect_workspace.restype = _u64
lib.nsa_tri_isect_workspace.argtypes = [_u32]
lib.nsa_tri_isect_count.restype = _i
lib.nsa_tri_isect_count.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, _p, _p, _p, _p]
lib.nsa_tri_isect_emit.restype = _i
lib.nsa_tri_isect_emit.argtypes = [_p, _p, _u32, _p, _u32, _p, _u32, _p, _p, _u64, _p, _p, _p]
EXPORTS += ["nsa_tri_isect_workspace", "nsa_tri_isect_count", "nsa_tri_isect_emit"]
lib.nsa_mesh_split_fans_workspace.restype = _u64
lib.nsa_mesh_split_fans_workspace.argtypes = [_u32, _u32]
lib.nsa_mesh_split_fans.restype = _i
lib.nsa_mesh_split_fans.argtypes = [_p, _u32, _u32, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]
EXPORTS += ["nsa_mesh_split_fans_workspace", "nsa_mesh_split_fans"]
SPLIT_CUT_INCONSISTENT = 1                                                  # NSA_SPLIT_* of header Section 26
lib.nsa_icp_transform.restype = _i
lib.nsa_icp_transform.argtypes = [_p, _u32, ctypes.POINTER(_f64), _p, _p]
lib.nsa_icp_plane_system_workspace.restype = _u64
lib.nsa_icp_plane_system_workspace.argtypes = [_u32]
lib.nsa_icp_plane_system.restype = _i
lib.nsa_icp_plane_system.argtypes = [_p, _u32, _i, _p, _p, _p, _p, _u32, _p, _p, _p, _u32, _p, _u32, _i, _f64, _p, _p, _p, _p]
EXPORTS += ["nsa_icp_transform", "nsa_icp_plane_system_workspace", "nsa_icp_plane_system"]
ICP_CLOUD, ICP_SURFACE = 0, 1                                               # NSA_ICP_* of header Section 27
ICP_KERNELS = ("l2", "huber", "tukey")                                      # NSA_ICP_KERNEL_*
lib.nsa_nn_query_k.restype = _i
lib.nsa_nn_query_k.argtypes = [_p, _u32, _p, _u32, _u32, _f64, _p, _p, _p, _p]
lib.nsa_cloud_normals.restype = _i
lib.nsa_cloud_normals.argtypes = [_p, _u32, _p, _p, _u32, _u32, _p, _p, _u32, _p, _p, _p, _p]
EXPORTS += ["nsa_nn_query_k", "nsa_cloud_normals"]
KNN_MAX_K = 64                                                              # header Section 28
