"""ctypes binding of libnerf_fl_amd.so (the C ABI in include/nerf_fl_amd.h).

There is no fallback: if the shared library is missing or does not export the
ABI this package was written against, importing a renderer entry point raises.

The mirror is written by hand and names itself: STRUCTS, SYMBOLS and CONSTANTS below list every struct, entry point and
constant repeated here, and tests/test_abi_cpu.py holds each of them to the header.  NFL_ABI_VERSION moves when an
existing struct or signature changes; a new symbol or struct alone does not move it (a library that lacks a symbol
already fails in lib(), which looks every SYMBOLS entry up).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NFL_LIB selects a diagnostic / variant build of the library (make diag, make variant) -- honoured only in a
# developer session (NERF_FL_AMD_DEV=1), so that a stray environment variable cannot swap the library under the product
LIB_PATH = ((os.environ.get("NFL_LIB") if os.environ.get("NERF_FL_AMD_DEV") == "1" else None)
            or os.path.join(_HERE, "libnerf_fl_amd.so"))

NFL_ABI_VERSION = 10
NFL_GMAX_SLOTS = 1024
NFL_PREC_F16X3 = 0
NFL_PREC_F16 = 1
NFL_PREC_F16W = 2      # backward only: one-product arithmetic, but the gradient chain reads hi + lo weight fragments
NFL_STATUS_NONFINITE = 1
NFL_STATUS_RANGE = 2
NFL_STATUS_POSE_ID = 4   # nfl_pose_rays: an image id (or its pose row) outside the pose table
NFL_NUM_LAYERS = 19

# layer slot -> state_dict prefix (reference models/nerf.py:121-151)
LAYER_NAMES = (
    [f"xyz_encoding_{i + 1}.0" for i in range(8)]
    + ["xyz_encoding_final", "dir_encoding.0", "static_sigma.0", "static_rgb.0"]
    + [f"transient_encoding.{j}" for j in (0, 2, 4, 6)]
    + ["transient_sigma.0", "transient_rgb.0", "transient_beta.0"]
)
assert len(LAYER_NAMES) == NFL_NUM_LAYERS


class FieldDesc(C.Structure):
    _fields_ = [
        ("n_emb_xyz", C.c_int32), ("n_emb_dir", C.c_int32),
        ("encode_appearance", C.c_int32), ("n_a", C.c_int32),
        ("encode_transient", C.c_int32), ("n_tau", C.c_int32),
        ("beta_min", C.c_float), ("reserved", C.c_int32),
    ]


class FieldParams(C.Structure):
    _fields_ = [("weight", C.c_void_p * NFL_NUM_LAYERS), ("bias", C.c_void_p * NFL_NUM_LAYERS)]


class PackJob(C.Structure):
    _fields_ = [("h_plan", C.c_void_p), ("d_plan", C.c_void_p), ("params", C.POINTER(FieldParams)), ("d_packed", C.c_void_p),
                ("packed_bytes", C.c_size_t), ("d_status", C.c_void_p)]


NFL_PACK_MAX_JOBS = 4


class Camera(C.Structure):
    _fields_ = [("c2w", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("reserved", C.c_int32), ("pix0", C.c_int64), ("near", C.c_float), ("far", C.c_float)]


class PassArgs(C.Structure):
    _fields_ = [
        ("d_rays", C.c_void_p), ("h_cam", C.POINTER(Camera)), ("d_view_dir", C.c_void_p),
        ("n_rays", C.c_int32), ("n_samples", C.c_int32),
        ("d_z", C.c_void_p), ("d_lin", C.c_void_p), ("d_perturb_rand", C.c_void_p),
        ("perturb", C.c_float), ("use_disp", C.c_int32),
        ("d_z_out", C.c_void_p),
        ("d_noise", C.c_void_p), ("noise_std", C.c_float),
        ("d_a_emb", C.c_void_p), ("d_t_emb", C.c_void_p),
        ("sigma_only", C.c_int32), ("white_back", C.c_int32),
        ("test_extras", C.c_int32), ("stash_split", C.c_int32),
        ("d_weights", C.c_void_p), ("d_opacity", C.c_void_p), ("d_rgb", C.c_void_p), ("d_depth", C.c_void_p),
        ("d_transient_sigmas", C.c_void_p), ("d_beta", C.c_void_p),
        ("d_rgb_static", C.c_void_p), ("d_rgb_transient", C.c_void_p),
        ("d_rgb_static_only", C.c_void_p), ("d_depth_static_only", C.c_void_p),
        ("d_rgb_transient_only", C.c_void_p), ("d_depth_transient_only", C.c_void_p),
        ("d_field_raw", C.c_void_p), ("d_act_stash", C.c_void_p),
        ("d_pe_w_xyz", C.c_void_p), ("d_pe_w_dir", C.c_void_p),
        ("d_loss_target", C.c_void_p), ("d_losses", C.c_void_p), ("d_seed_rgb", C.c_void_p), ("d_seed_beta", C.c_void_p),
        ("loss_coef", C.c_float), ("lambda_u", C.c_float), ("loss_slot", C.c_int32), ("reserved2", C.c_int32),
        ("d_status", C.c_void_p),
        ("d_embedded", C.c_void_p), ("n_points", C.c_int32), ("embedded_stride", C.c_int32),
        ("d_cam", C.c_void_p),
    ]


class CompBwdArgs(C.Structure):
    _fields_ = [
        ("d_field_raw", C.c_void_p), ("d_z", C.c_void_p), ("d_noise", C.c_void_p), ("noise_std", C.c_float),
        ("n_rays", C.c_int32), ("n_samples", C.c_int32), ("use_transient", C.c_int32), ("white_back", C.c_int32),
        ("reserved", C.c_int32),
        ("g_weights", C.c_void_p), ("g_opacity", C.c_void_p), ("g_rgb", C.c_void_p), ("g_depth", C.c_void_p),
        ("g_transient_sigmas", C.c_void_p), ("g_beta", C.c_void_p), ("g_rgb_static", C.c_void_p),
        ("g_rgb_transient", C.c_void_p), ("g_tsig_const", C.c_float), ("reserved3", C.c_int32), ("d_go", C.c_void_p),
        ("d_head_grads", C.c_void_p), ("d_gmax", C.c_void_p),
    ]


class DgradArgs(C.Structure):
    _fields_ = [
        ("d_head_grads", C.c_void_p), ("d_act_stash", C.c_void_p), ("d_grad_stash", C.c_void_p),
        ("n_rays", C.c_int32), ("n_samples", C.c_int32), ("use_transient", C.c_int32), ("dir_is_data", C.c_int32),
        ("d_g_a_emb", C.c_void_p), ("d_g_t_emb", C.c_void_p), ("d_latent_row", C.c_void_p),
        ("d_g_rays", C.c_void_p), ("d_rays", C.c_void_p), ("d_z", C.c_void_p),
        ("d_pe_w_xyz", C.c_void_p), ("d_pe_w_dir", C.c_void_p), ("d_gmax", C.c_void_p), ("rounding_seed", C.c_uint32),
    ]


NFL_ADAM_MAX_TENSORS = 64


class AdamTensors(C.Structure):
    _fields_ = [("param", C.c_void_p * NFL_ADAM_MAX_TENSORS), ("grad", C.c_void_p * NFL_ADAM_MAX_TENSORS),
                ("exp_avg", C.c_void_p * NFL_ADAM_MAX_TENSORS), ("exp_avg_sq", C.c_void_p * NFL_ADAM_MAX_TENSORS),
                ("numel", C.c_int32 * NFL_ADAM_MAX_TENSORS)]


NFL_OPT_SGD, NFL_OPT_ADAM, NFL_OPT_RADAM, NFL_OPT_RANGER = 0, 1, 2, 3
NFL_OPT_HYPER = 8      # lr, beta1 | momentum, beta2, eps, weight_decay, alpha, k, threshold


class OptimTensors(C.Structure):
    _fields_ = [("param", C.c_void_p * NFL_ADAM_MAX_TENSORS), ("grad", C.c_void_p * NFL_ADAM_MAX_TENSORS),
                ("state0", C.c_void_p * NFL_ADAM_MAX_TENSORS), ("state1", C.c_void_p * NFL_ADAM_MAX_TENSORS),
                ("state2", C.c_void_p * NFL_ADAM_MAX_TENSORS), ("numel", C.c_int32 * NFL_ADAM_MAX_TENSORS)]


class LossArgs(C.Structure):
    _fields_ = [("d_rgb_coarse", C.c_void_p), ("d_rgb_fine", C.c_void_p), ("d_beta", C.c_void_p),
                ("d_transient_sigmas", C.c_void_p), ("d_target", C.c_void_p), ("n_rays", C.c_int32), ("n_samples", C.c_int32),
                ("coef", C.c_float), ("lambda_u", C.c_float), ("d_losses", C.c_void_p), ("d_grad_loss", C.c_void_p * 4),
                ("d_g_rgb_coarse", C.c_void_p), ("d_g_rgb_fine", C.c_void_p), ("d_g_beta", C.c_void_p),
                ("d_g_transient_sigmas", C.c_void_p)]


class FieldGrads(C.Structure):
    _fields_ = [("weight", C.c_void_p * NFL_NUM_LAYERS), ("bias", C.c_void_p * NFL_NUM_LAYERS)]


class PoseArgs(C.Structure):
    _fields_ = [("d_r", C.c_void_p), ("d_t", C.c_void_p), ("d_init_c2w", C.c_void_p), ("d_row_of_id", C.c_void_p),
                ("d_ts", C.c_void_p), ("d_rays_cam", C.c_void_p), ("n_cams", C.c_int32), ("n_ids", C.c_int32),
                ("n_rays", C.c_int32), ("cam_stride", C.c_int32), ("d_rays", C.c_void_p), ("d_rows", C.c_void_p),
                ("d_g_rays", C.c_void_p), ("d_g_r", C.c_void_p), ("d_g_t", C.c_void_p), ("d_status", C.c_void_p)]


class AppFitArgs(C.Structure):
    _fields_ = [("d_zcache", C.c_void_p), ("d_weights", C.c_void_p), ("d_opacity", C.c_void_p), ("d_target", C.c_void_p),
                ("d_items", C.c_void_p), ("d_image_items", C.c_void_p), ("d_codes", C.c_void_p), ("d_w_dir", C.c_void_p),
                ("d_w_rgb", C.c_void_p), ("d_b_rgb", C.c_void_p),
                ("n_rays", C.c_int32), ("n_samples", C.c_int32), ("n_pad", C.c_int32), ("n_items", C.c_int32),
                ("n_images", C.c_int32), ("n_a", C.c_int32), ("ld_dir", C.c_int32), ("col_a", C.c_int32),
                ("white_back", C.c_int32), ("reserved", C.c_int32),
                ("d_partials", C.c_void_p), ("d_grad", C.c_void_p), ("d_loss", C.c_void_p), ("d_rgb", C.c_void_p)]


NFL_LAYOUT_WORLD, NFL_LAYOUT_CAMERA = 0, 1


class ImageRec(C.Structure):
    _fields_ = [("pix0", C.c_int64), ("byte0", C.c_int64), ("width", C.c_int32), ("height", C.c_int32),
                ("channels", C.c_int32), ("id", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("near", C.c_float), ("far", C.c_float), ("c2w", C.c_float * 12)]


class GatherArgs(C.Structure):
    _fields_ = [("d_pixels", C.c_void_p), ("d_table", C.c_void_p), ("n_images", C.c_int32), ("layout", C.c_int32),
                ("n_pixels", C.c_int64), ("start", C.c_int64), ("key", C.c_uint64), ("count", C.c_int32),
                ("reserved", C.c_int32), ("d_rays", C.c_void_p), ("d_ts", C.c_void_p), ("d_rgb", C.c_void_p)]


NFL_METRIC_COLUMNS = 8


class MetricsArgs(C.Structure):
    _fields_ = [("d_pred", C.c_void_p), ("d_pixels", C.c_void_p), ("d_table", C.c_void_p), ("n_images", C.c_int32),
                ("image", C.c_int32), ("d_target", C.c_void_p), ("d_mask", C.c_void_p), ("width", C.c_int32),
                ("height", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32),
                ("clip", C.c_int32), ("slot", C.c_int32), ("d_results", C.c_void_p), ("n_slots", C.c_int32),
                ("reserved", C.c_int32), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("d_pred_u8", C.c_void_p), ("d_ssim_map", C.c_void_p)]


class DepthArgs(C.Structure):
    _fields_ = [("d_depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("x0", C.c_int32),
                ("x1", C.c_int32), ("y0", C.c_int32), ("y1", C.c_int32), ("d_lut", C.c_void_p), ("d_image", C.c_void_p),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class BoundsArgs(C.Structure):
    _fields_ = [("d_xyz", C.c_void_p), ("d_row", C.c_void_p), ("n_points", C.c_int32), ("n_images", C.c_int32),
                ("q_lo", C.c_double), ("q_hi", C.c_double), ("d_bounds", C.c_void_p), ("d_count", C.c_void_p)]


class SurfaceArgs(C.Structure):
    _fields_ = [("d_lattice", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("iso", C.c_float),
                ("lo", C.c_float * 3), ("spacing", C.c_float * 3), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("d_totals", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64),
                ("d_vertices", C.c_void_p), ("d_normals", C.c_void_p), ("d_triangles", C.c_void_p)]


class MeshLabelArgs(C.Structure):
    _fields_ = [("d_triangles", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("d_component", C.c_void_p),
                ("d_totals", C.c_void_p)]


class MeshStatsArgs(C.Structure):
    _fields_ = [("d_component", C.c_void_p), ("d_positions", C.c_void_p), ("d_triangles", C.c_void_p),
                ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("n_components", C.c_int64),
                ("d_n_vertices", C.c_void_p), ("d_n_triangles", C.c_void_p), ("d_bounds", C.c_void_p)]


class MeshCompactArgs(C.Structure):
    _fields_ = [("d_component", C.c_void_p), ("d_keep", C.c_void_p), ("d_triangles", C.c_void_p),
                ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("n_components", C.c_int64),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("d_totals", C.c_void_p),
                ("n_kept_vertices", C.c_int64), ("n_kept_triangles", C.c_int64),
                ("d_vertices", C.c_void_p), ("d_normals", C.c_void_p), ("d_colors", C.c_void_p),
                ("d_out_vertices", C.c_void_p), ("d_out_normals", C.c_void_p), ("d_out_colors", C.c_void_p),
                ("d_out_triangles", C.c_void_p)]


SIMPLIFY_LAMBDA = 1e-3
SIMPLIFY_PLACEMENTS = {"mean": 0, "quadric": 1}


class MeshSimplifyArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_normals", C.c_void_p), ("d_colors", C.c_void_p), ("d_triangles", C.c_void_p),
                ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("cell", C.c_double), ("origin", C.c_double * 3),
                ("placement", C.c_int32), ("reserved", C.c_int32), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("d_totals", C.c_void_p), ("d_cluster", C.c_void_p), ("n_out_vertices", C.c_int64),
                ("n_out_triangles", C.c_int64), ("d_out_vertices", C.c_void_p), ("d_out_normals", C.c_void_p),
                ("d_out_colors", C.c_void_p), ("d_out_triangles", C.c_void_p)]


SMOOTH_MAX_STEPS = 1024
ADJ_SHORT_ROW = 24
NORMAL_WEIGHTINGS = {"area": 0, "uniform": 1}


class MeshAdjacencyArgs(C.Structure):
    _fields_ = [("d_triangles", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("d_totals", C.c_void_p),
                ("n_incident", C.c_int64), ("n_neighbors", C.c_int64), ("d_tri_offsets", C.c_void_p),
                ("d_incident", C.c_void_p), ("d_offsets", C.c_void_p), ("d_neighbors", C.c_void_p),
                ("d_boundary", C.c_void_p)]


class MeshSmoothArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_offsets", C.c_void_p), ("d_neighbors", C.c_void_p),
                ("n_vertices", C.c_int64), ("n_neighbors", C.c_int64), ("d_boundary", C.c_void_p),
                ("d_pinned", C.c_void_p), ("fix_boundary", C.c_int32), ("n_steps", C.c_int32),
                ("factors", C.POINTER(C.c_double)), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("d_out_vertices", C.c_void_p)]


class MeshNormalsArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("d_tri_offsets", C.c_void_p), ("d_incident", C.c_void_p),
                ("n_incident", C.c_int64), ("weighting", C.c_int32), ("reserved", C.c_int32),
                ("d_fallback_normals", C.c_void_p), ("d_out_normals", C.c_void_p)]


class OccBuildArgs(C.Structure):
    _fields_ = [("d_lattice", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("threshold", C.c_float), ("dilate", C.c_int32), ("reserved", C.c_int32), ("d_scratch", C.c_void_p),
                ("scratch_bytes", C.c_size_t), ("d_bits", C.c_void_p)]


class OccClipArgs(C.Structure):
    _fields_ = [("d_rays", C.c_void_p), ("n_rays", C.c_int64), ("d_bits", C.c_void_p), ("nx", C.c_int32),
                ("ny", C.c_int32), ("nz", C.c_int32), ("lo", C.c_float * 3), ("spacing", C.c_float * 3),
                ("reserved", C.c_int32), ("d_near_far", C.c_void_p), ("d_hit", C.c_void_p)]


BLEND_WEIGHTINGS = {"cos": 0, "uniform": 1}


class MeshDepthArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32),
                ("count", C.c_int32), ("reserved", C.c_int32), ("d_depth", C.c_void_p), ("n_depth", C.c_int64)]


class MeshBlendArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_normals", C.c_void_p), ("n_vertices", C.c_int64), ("d_pixels", C.c_void_p),
                ("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32), ("count", C.c_int32),
                ("weighting", C.c_int32), ("d_depth", C.c_void_p), ("n_depth", C.c_int64), ("d_image_weights", C.c_void_p),
                ("d_center", C.c_void_p), ("min_cos", C.c_float), ("depth_tol", C.c_float), ("reject", C.c_float),
                ("start", C.c_int32), ("d_sum", C.c_void_p), ("d_views", C.c_void_p)]


SHADE_MODES = {"color": 0, "normal": 1, "facing": 2}
VIS_EMPTY = -1                                  # 2^64 - 1 as the int64 that torch holds the words in


class MeshVisibilityArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32),
                ("count", C.c_int32), ("reserved", C.c_int32), ("d_vis", C.c_void_p), ("n_vis", C.c_int64)]


class MeshShadeArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32),
                ("count", C.c_int32), ("mode", C.c_int32), ("d_vis", C.c_void_p), ("n_vis", C.c_int64),
                ("d_attr", C.c_void_p), ("background", C.c_float * 3), ("reserved", C.c_int32), ("d_rgb", C.c_void_p),
                ("d_rgb_u8", C.c_void_p), ("d_depth", C.c_void_p), ("d_triangle", C.c_void_p)]


ATLAS_MIN_CELL, ATLAS_MAX_CELL = 6, 1024


class AtlasPointsArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_vertex_normals", C.c_void_p), ("d_triangles", C.c_void_p),
                ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("cell", C.c_int32), ("cols", C.c_int32),
                ("rows", C.c_int32), ("reserved", C.c_int32), ("first_texel", C.c_int64), ("n_texels", C.c_int64),
                ("d_points", C.c_void_p), ("d_normals", C.c_void_p)]


class AtlasResolveArgs(C.Structure):
    _fields_ = [("d_triangles", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("cell", C.c_int32),
                ("cols", C.c_int32), ("rows", C.c_int32), ("reserved", C.c_int32), ("first_texel", C.c_int64),
                ("n_texels", C.c_int64), ("d_sum", C.c_void_p), ("d_views", C.c_void_p), ("d_vertex_colors", C.c_void_p),
                ("fallback", C.c_float * 3), ("background", C.c_float * 3), ("d_texture", C.c_void_p),
                ("d_texture_u8", C.c_void_p), ("d_seen", C.c_void_p)]


class MeshShadeAtlasArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32),
                ("count", C.c_int32), ("reserved", C.c_int32), ("d_vis", C.c_void_p), ("n_vis", C.c_int64),
                ("d_atlas", C.c_void_p), ("d_atlas_u8", C.c_void_p), ("cell", C.c_int32), ("cols", C.c_int32),
                ("rows", C.c_int32), ("reserved2", C.c_int32), ("background", C.c_float * 3), ("reserved3", C.c_int32),
                ("d_rgb", C.c_void_p), ("d_rgb_u8", C.c_void_p), ("d_depth", C.c_void_p), ("d_triangle", C.c_void_p)]


class TsdfFuseArgs(C.Structure):
    _fields_ = [("d_table", C.c_void_p), ("n_images", C.c_int32), ("first", C.c_int32), ("count", C.c_int32),
                ("start", C.c_int32), ("d_depth", C.c_void_p), ("n_depth", C.c_int64), ("d_pixel_weights", C.c_void_p),
                ("d_image_weights", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("trunc", C.c_float), ("lo", C.c_float * 3), ("spacing", C.c_float * 3), ("d_acc", C.c_void_p),
                ("d_views", C.c_void_p)]


class TsdfResolveArgs(C.Structure):
    _fields_ = [("d_acc", C.c_void_p), ("d_views", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("min_views", C.c_int32), ("min_weight", C.c_float), ("fill", C.c_float), ("d_lattice", C.c_void_p),
                ("d_known", C.c_void_p)]


class TsdfSupportArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("n_vertices", C.c_int64), ("d_known", C.c_void_p), ("nx", C.c_int32),
                ("ny", C.c_int32), ("nz", C.c_int32), ("reserved", C.c_int32), ("lo", C.c_float * 3),
                ("spacing", C.c_float * 3), ("d_support", C.c_void_p)]


MESHDIST_MAX_TAU = 8
MESHDIST_COLUMNS = 13                           # count, sum, sum of squares, max, 8 x within tau, sum of |dot|


class TriGridArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("lo", C.c_float * 3), ("cell", C.c_float), ("dims", C.c_int32 * 3),
                ("reserved", C.c_int32), ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("d_totals", C.c_void_p), ("n_entries", C.c_int64), ("d_offsets", C.c_void_p), ("d_entries", C.c_void_p)]


class MeshClosestArgs(C.Structure):
    _fields_ = [("d_points", C.c_void_p), ("n_points", C.c_int64), ("d_vertices", C.c_void_p),
                ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64), ("n_triangles", C.c_int64),
                ("d_offsets", C.c_void_p), ("d_entries", C.c_void_p), ("n_entries", C.c_int64), ("lo", C.c_float * 3),
                ("cell", C.c_float), ("dims", C.c_int32 * 3), ("max_distance", C.c_float), ("d_normals", C.c_void_p),
                ("d_distance", C.c_void_p), ("d_triangle", C.c_void_p), ("d_point", C.c_void_p), ("d_bary", C.c_void_p),
                ("d_dot", C.c_void_p)]


class MeshSampleArgs(C.Structure):
    _fields_ = [("d_vertices", C.c_void_p), ("d_triangles", C.c_void_p), ("n_vertices", C.c_int64),
                ("n_triangles", C.c_int64), ("seed", C.c_uint64), ("density", C.c_float), ("reserved", C.c_int32),
                ("d_scratch", C.c_void_p), ("scratch_bytes", C.c_size_t), ("d_totals", C.c_void_p),
                ("n_samples", C.c_int64), ("d_points", C.c_void_p), ("d_sample_triangles", C.c_void_p),
                ("d_normals", C.c_void_p)]


class MeshDistReduceArgs(C.Structure):
    _fields_ = [("d_distance", C.c_void_p), ("d_dot", C.c_void_p), ("n", C.c_int64), ("n_tau", C.c_int32),
                ("tau", C.c_float * MESHDIST_MAX_TAU), ("reserved", C.c_int32), ("d_scratch", C.c_void_p),
                ("scratch_bytes", C.c_size_t), ("d_row", C.c_void_p)]


# registration (nerf_fl_amd/registration.py): plain arguments, no struct
REGISTER_MODES = {"point": 0, "plane": 1}
REGISTER_STATUS = {"ok": 0, "few": 1, "singular": 2}
REGISTER_TRANSFORM = 13                         # s, R row-major, t
REGISTER_HISTORY = 4                            # count, rms, status, s per iteration
# the columns of the moments row: where each run starts
REGISTER_ROW = {"COUNT": 0, "SUM_DD": 1, "SUM_P": 2, "SUM_Q": 5, "SUM_PP": 8, "SUM_QQ": 9, "SUM_PQ": 10, "ATA": 19, "ATB": 47,
                "SUM_RR": 54, "COLUMNS": 55}

# mesh cast (nerf_fl_amd/raycast.py): plain arguments, no struct
CAST_MODES = {"first": 0, "any": 1}

# mesh solid (nerf_fl_amd/solid.py): plain arguments, no struct
SOLID_MAX_DIRECTIONS = 7

# mesh edges (nerf_fl_amd/topology.py): plain arguments, no struct
EDGE_KINDS = {"interior": 0, "boundary": 1, "flipped": 2, "nonmanifold": 3}
EDGE_SHORT_ROW = 8
EDGE_TOTALS, LOOP_TOTALS, FILL_TOTALS = 7, 3, 3

# every struct include/nerf_fl_amd.h declares: C name -> its mirror
STRUCTS = {
    "nfl_field_desc": FieldDesc, "nfl_field_params": FieldParams, "nfl_pack_job": PackJob, "nfl_camera": Camera,
    "nfl_pass_args": PassArgs, "nfl_compbwd_args": CompBwdArgs, "nfl_dgrad_args": DgradArgs,
    "nfl_field_grads": FieldGrads, "nfl_adam_tensors": AdamTensors, "nfl_optim_tensors": OptimTensors,
    "nfl_loss_args": LossArgs, "nfl_pose_args": PoseArgs, "nfl_appfit_args": AppFitArgs, "nfl_image_rec": ImageRec,
    "nfl_gather_args": GatherArgs, "nfl_metrics_args": MetricsArgs, "nfl_depth_args": DepthArgs,
    "nfl_bounds_args": BoundsArgs, "nfl_surface_args": SurfaceArgs, "nfl_mesh_label_args": MeshLabelArgs,
    "nfl_mesh_stats_args": MeshStatsArgs, "nfl_mesh_compact_args": MeshCompactArgs,
    "nfl_mesh_simplify_args": MeshSimplifyArgs, "nfl_mesh_adjacency_args": MeshAdjacencyArgs,
    "nfl_mesh_smooth_args": MeshSmoothArgs, "nfl_mesh_normals_args": MeshNormalsArgs,
    "nfl_occ_build_args": OccBuildArgs, "nfl_occ_clip_args": OccClipArgs, "nfl_mesh_depth_args": MeshDepthArgs,
    "nfl_mesh_blend_args": MeshBlendArgs, "nfl_mesh_visibility_args": MeshVisibilityArgs,
    "nfl_mesh_shade_args": MeshShadeArgs, "nfl_atlas_points_args": AtlasPointsArgs,
    "nfl_atlas_resolve_args": AtlasResolveArgs, "nfl_mesh_shade_atlas_args": MeshShadeAtlasArgs,
    "nfl_tsdf_fuse_args": TsdfFuseArgs, "nfl_tsdf_resolve_args": TsdfResolveArgs,
    "nfl_tsdf_support_args": TsdfSupportArgs, "nfl_trigrid_args": TriGridArgs,
    "nfl_mesh_closest_args": MeshClosestArgs, "nfl_mesh_sample_args": MeshSampleArgs,
    "nfl_meshdist_reduce_args": MeshDistReduceArgs,
}

# every constant of the header (#define or enum) that this module repeats: C name -> the value held here
CONSTANTS = {
    "NFL_ABI_VERSION": NFL_ABI_VERSION, "NFL_GMAX_SLOTS": NFL_GMAX_SLOTS,
    "NFL_PREC_F16X3": NFL_PREC_F16X3, "NFL_PREC_F16": NFL_PREC_F16, "NFL_PREC_F16W": NFL_PREC_F16W,
    "NFL_STATUS_NONFINITE": NFL_STATUS_NONFINITE, "NFL_STATUS_RANGE": NFL_STATUS_RANGE,
    "NFL_STATUS_POSE_ID": NFL_STATUS_POSE_ID, "NFL_NUM_LAYERS": NFL_NUM_LAYERS,
    "NFL_PACK_MAX_JOBS": NFL_PACK_MAX_JOBS, "NFL_ADAM_MAX_TENSORS": NFL_ADAM_MAX_TENSORS,
    "NFL_OPT_SGD": NFL_OPT_SGD, "NFL_OPT_ADAM": NFL_OPT_ADAM, "NFL_OPT_RADAM": NFL_OPT_RADAM,
    "NFL_OPT_RANGER": NFL_OPT_RANGER, "NFL_OPT_HYPER": NFL_OPT_HYPER,
    "NFL_LAYOUT_WORLD": NFL_LAYOUT_WORLD, "NFL_LAYOUT_CAMERA": NFL_LAYOUT_CAMERA,
    "NFL_METRIC_COLUMNS": NFL_METRIC_COLUMNS,
    "NFL_SIMPLIFY_LAMBDA": SIMPLIFY_LAMBDA,
    "NFL_SIMPLIFY_MEAN": SIMPLIFY_PLACEMENTS["mean"], "NFL_SIMPLIFY_QUADRIC": SIMPLIFY_PLACEMENTS["quadric"],
    "NFL_SMOOTH_MAX_STEPS": SMOOTH_MAX_STEPS, "NFL_ADJ_SHORT_ROW": ADJ_SHORT_ROW,
    "NFL_NORMALS_AREA": NORMAL_WEIGHTINGS["area"], "NFL_NORMALS_UNIFORM": NORMAL_WEIGHTINGS["uniform"],
    "NFL_BLEND_COS": BLEND_WEIGHTINGS["cos"], "NFL_BLEND_UNIFORM": BLEND_WEIGHTINGS["uniform"],
    "NFL_SHADE_COLOR": SHADE_MODES["color"], "NFL_SHADE_NORMAL": SHADE_MODES["normal"],
    "NFL_SHADE_FACING": SHADE_MODES["facing"],
    "NFL_MESHDIST_MAX_TAU": MESHDIST_MAX_TAU, "NFL_MESHDIST_COLUMNS": MESHDIST_COLUMNS,
    "NFL_REGISTER_POINT": REGISTER_MODES["point"], "NFL_REGISTER_PLANE": REGISTER_MODES["plane"],
    "NFL_REGISTER_OK": REGISTER_STATUS["ok"], "NFL_REGISTER_FEW": REGISTER_STATUS["few"],
    "NFL_REGISTER_SINGULAR": REGISTER_STATUS["singular"],
    "NFL_REGISTER_TRANSFORM": REGISTER_TRANSFORM, "NFL_REGISTER_HISTORY": REGISTER_HISTORY,
    **{"NFL_REGISTER_" + k: v for k, v in REGISTER_ROW.items()},
    "NFL_CAST_FIRST": CAST_MODES["first"], "NFL_CAST_ANY": CAST_MODES["any"],
    "NFL_SOLID_MAX_DIRECTIONS": SOLID_MAX_DIRECTIONS,
    **{"NFL_EDGE_" + k.upper(): v for k, v in EDGE_KINDS.items()}, "NFL_EDGE_SHORT_ROW": EDGE_SHORT_ROW,
    "NFL_EDGE_TOTALS": EDGE_TOTALS, "NFL_LOOP_TOTALS": LOOP_TOTALS, "NFL_FILL_TOTALS": FILL_TOTALS,
}

# every function include/nerf_fl_amd.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("nfl_plan_bytes", C.c_size_t, [C.POINTER(FieldDesc)]),
    ("nfl_plan_build", C.c_int, [C.POINTER(FieldDesc), C.c_int, C.c_void_p, C.c_size_t]),
    ("nfl_packed_bytes", C.c_size_t, [C.POINTER(FieldDesc), C.c_int]),
    ("nfl_param_count", C.c_size_t, [C.POINTER(FieldDesc)]),
    ("nfl_pack_field", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(FieldParams), C.c_void_p, C.c_size_t, C.c_void_p,
                                 C.c_void_p]),
    ("nfl_pack_fields", C.c_int, [C.c_int32, C.POINTER(PackJob), C.c_void_p]),
    ("nfl_compose_forward", C.c_int, [C.POINTER(FieldParams), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    ("nfl_render_pass", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PassArgs), C.c_void_p]),
    ("nfl_sample_pdf", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_field_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p]),
    ("nfl_posenc", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_gen_rays", C.c_int, [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int64,
                               C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    ("nfl_act_stash_bytes", C.c_size_t, [C.POINTER(FieldDesc), C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_grad_stash_bytes", C.c_size_t, [C.POINTER(FieldDesc), C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_bwd_plan_build", C.c_int, [C.POINTER(FieldDesc), C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    ("nfl_bwd_packed_bytes", C.c_size_t, [C.POINTER(FieldDesc), C.c_int32, C.c_int32]),
    ("nfl_composite_backward", C.c_int, [C.POINTER(CompBwdArgs), C.c_void_p]),
    ("nfl_mlp_dgrad", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DgradArgs), C.c_void_p]),
    ("nfl_wgrad_plan_bytes", C.c_size_t, []),
    ("nfl_wgrad_plan_build", C.c_int, [C.POINTER(FieldDesc), C.c_int32, C.c_void_p, C.c_size_t]),
    ("nfl_wgrad_scratch_bytes", C.c_size_t, []),
    ("nfl_mlp_wgrad", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                C.POINTER(FieldParams), C.c_void_p, C.POINTER(FieldGrads), C.c_void_p]),
    ("nfl_adam_step", C.c_int, [C.POINTER(AdamTensors), C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                C.c_void_p]),
    ("nfl_adam_step_dev", C.c_int, [C.POINTER(AdamTensors), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nfl_optim_step", C.c_int, [C.POINTER(OptimTensors), C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                 C.c_void_p]),
    ("nfl_optim_step_dev", C.c_int, [C.POINTER(OptimTensors), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p]),
    ("nfl_loss_forward", C.c_int, [C.POINTER(LossArgs), C.c_void_p]),
    ("nfl_loss_backward", C.c_int, [C.POINTER(LossArgs), C.c_void_p]),
    ("nfl_pose_rays", C.c_int, [C.POINTER(PoseArgs), C.c_void_p]),
    ("nfl_pose_rays_backward", C.c_int, [C.POINTER(PoseArgs), C.c_void_p]),
    ("nfl_appearance_cache", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(PassArgs), C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    ("nfl_appfit_partials_floats", C.c_size_t, [C.c_int32]),
    ("nfl_appearance_fit", C.c_int, [C.POINTER(AppFitArgs), C.c_void_p]),
    ("nfl_gather_batch", C.c_int, [C.POINTER(GatherArgs), C.c_void_p]),
    ("nfl_image_metrics_scratch_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("nfl_image_metrics", C.c_int, [C.POINTER(MetricsArgs), C.c_void_p]),
    ("nfl_depth_image_scratch_bytes", C.c_size_t, [C.c_int32, C.c_int32]),
    ("nfl_depth_image", C.c_int, [C.POINTER(DepthArgs), C.c_void_p]),
    ("nfl_depth_bounds", C.c_int, [C.POINTER(BoundsArgs), C.c_void_p]),
    ("nfl_surface_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_surface_count", C.c_int, [C.POINTER(SurfaceArgs), C.c_void_p]),
    ("nfl_surface_emit", C.c_int, [C.POINTER(SurfaceArgs), C.c_void_p]),
    ("nfl_mesh_label_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
    ("nfl_mesh_label", C.c_int, [C.POINTER(MeshLabelArgs), C.c_void_p]),
    ("nfl_mesh_stats", C.c_int, [C.POINTER(MeshStatsArgs), C.c_void_p]),
    ("nfl_mesh_compact_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
    ("nfl_mesh_compact_count", C.c_int, [C.POINTER(MeshCompactArgs), C.c_void_p]),
    ("nfl_mesh_compact_emit", C.c_int, [C.POINTER(MeshCompactArgs), C.c_void_p]),
    ("nfl_mesh_simplify_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
    ("nfl_mesh_simplify_count", C.c_int, [C.POINTER(MeshSimplifyArgs), C.c_void_p]),
    ("nfl_mesh_simplify_emit", C.c_int, [C.POINTER(MeshSimplifyArgs), C.c_void_p]),
    ("nfl_mesh_adjacency_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
    ("nfl_mesh_adjacency_count", C.c_int, [C.POINTER(MeshAdjacencyArgs), C.c_void_p]),
    ("nfl_mesh_adjacency_emit", C.c_int, [C.POINTER(MeshAdjacencyArgs), C.c_void_p]),
    ("nfl_mesh_smooth_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_mesh_smooth", C.c_int, [C.POINTER(MeshSmoothArgs), C.c_void_p]),
    ("nfl_mesh_normals", C.c_int, [C.POINTER(MeshNormalsArgs), C.c_void_p]),
    ("nfl_occ_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_occ_build_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_occ_build", C.c_int, [C.POINTER(OccBuildArgs), C.c_void_p]),
    ("nfl_occ_clip_rays", C.c_int, [C.POINTER(OccClipArgs), C.c_void_p]),
    ("nfl_mesh_depth", C.c_int, [C.POINTER(MeshDepthArgs), C.c_void_p]),
    ("nfl_mesh_blend", C.c_int, [C.POINTER(MeshBlendArgs), C.c_void_p]),
    ("nfl_mesh_visibility", C.c_int, [C.POINTER(MeshVisibilityArgs), C.c_void_p]),
    ("nfl_mesh_shade", C.c_int, [C.POINTER(MeshShadeArgs), C.c_void_p]),
    ("nfl_atlas_points", C.c_int, [C.POINTER(AtlasPointsArgs), C.c_void_p]),
    ("nfl_atlas_resolve", C.c_int, [C.POINTER(AtlasResolveArgs), C.c_void_p]),
    ("nfl_mesh_shade_atlas", C.c_int, [C.POINTER(MeshShadeAtlasArgs), C.c_void_p]),
    ("nfl_tsdf_fuse", C.c_int, [C.POINTER(TsdfFuseArgs), C.c_void_p]),
    ("nfl_tsdf_resolve", C.c_int, [C.POINTER(TsdfResolveArgs), C.c_void_p]),
    ("nfl_tsdf_support", C.c_int, [C.POINTER(TsdfSupportArgs), C.c_void_p]),
    ("nfl_trigrid_bytes", C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    ("nfl_trigrid_count", C.c_int, [C.POINTER(TriGridArgs), C.c_void_p]),
    ("nfl_trigrid_emit", C.c_int, [C.POINTER(TriGridArgs), C.c_void_p]),
    ("nfl_mesh_closest", C.c_int, [C.POINTER(MeshClosestArgs), C.c_void_p]),
    ("nfl_mesh_sample_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_mesh_sample_count", C.c_int, [C.POINTER(MeshSampleArgs), C.c_void_p]),
    ("nfl_mesh_sample_emit", C.c_int, [C.POINTER(MeshSampleArgs), C.c_void_p]),
    ("nfl_meshdist_reduce_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_meshdist_reduce", C.c_int, [C.POINTER(MeshDistReduceArgs), C.c_void_p]),
    ("nfl_register_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_register_apply", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nfl_register_moments", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_int64, C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_double, C.c_double,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("nfl_register_solve", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_double, C.c_double,
                                     C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nfl_mesh_cast", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_occlusion", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    ("nfl_mesh_crossings", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p]),
    ("nfl_mesh_inside", C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_edges_bytes", C.c_size_t, [C.c_int64, C.c_int64]),
    ("nfl_mesh_edges_count", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_edges_emit", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_loops_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_mesh_loops_count", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_loops_emit", C.c_int, [C.c_int64, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_fill_bytes", C.c_size_t, [C.c_int64]),
    ("nfl_mesh_fill_count", C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_void_p]),
    ("nfl_mesh_fill_emit", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    ("nfl_abi_version", C.c_int, []),
    ("nfl_version", C.c_char_p, []),
    ("nfl_strerror", C.c_char_p, [C.c_int]),
    ("nfl_render_kernel_name", C.c_char_p, [C.c_int, C.c_int]),
]

_lib = None


def lib():
    """Load (once) and return the shared library; raises if it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"nerf_fl_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nerf_fl_amd/csrc`. There is no CPU or eager-PyTorch fallback for render_rays.")
    h = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(h, name)            # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if h.nfl_abi_version() != NFL_ABI_VERSION:
        raise RuntimeError(f"nerf_fl_amd: ABI mismatch (library {h.nfl_abi_version()}, python {NFL_ABI_VERSION})")
    _lib = h
    return _lib


def check(code, what):
    if code != 0:
        raise RuntimeError(f"nerf_fl_amd: {what} failed: {lib().nfl_strerror(code).decode()} ({code})")
