"""ctypes binding of include/fi_hip.h (libfi_hip.so).  Fails loudly when the library is missing:
there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FI_HIP_LIB", os.path.join(HERE, "libfi_hip.so"))   # override: experiments only

FI_OK = 0
FI_HOST, FI_DEVICE = 0, 1
FI_F32, FI_F64 = 0, 1
ERR_NAMES = {1: "FI_ERR_INVALID", 2: "FI_ERR_HIP", 3: "FI_ERR_STATE", 4: "FI_ERR_COMM",
             5: "FI_ERR_UNSUPPORTED", 6: "FI_ERR_BREAKDOWN", 7: "FI_ERR_TIMEOUT"}

# every symbol include/fi_hip.h declares
SYMBOLS = [
    "fi_last_error", "fi_device_count", "fi_ctx_create", "fi_ctx_create_slab", "fi_ctx_destroy",
    "fi_slab_range", "fi_slab_point_range", "fi_slab_partition", "fi_halo_width", "fi_comm_unique_id", "fi_comm_init", "fi_comm_init_host", "fi_comm_info", "fi_comm_self_test", "fi_set_model", "fi_add_points", "fi_add_border_prior",
    "fi_add_rows_coo", "fi_assemble", "fi_clear_points", "fi_set_option", "fi_solve_cg", "fi_jacobi", "fi_tile_pass", "fi_error_map",
    "fi_get_solution_f64", "fi_true_residual", "fi_apply_AtA_f64", "fi_get_Atb_f64", "fi_get_diag_f64",
    "fi_get_stats", "fi_memory_pool", "fi_time_apply", "fi_upscale_field",
    "fi_group_create", "fi_group_destroy", "fi_group_size", "fi_group_rank", "fi_group_assemble",
    "fi_group_solve_cg", "fi_group_apply_AtA_f64", "fi_group_true_residual", "fi_group_get_solution_f64", "fi_group_tile_pass", "fi_group_error_map",
    "fi_group_iso_extract", "fi_iso_extract", "fi_iso_extract_field", "fi_mesh_info", "fi_mesh_copy", "fi_mesh_destroy",
    "fi_dual_contour", "fi_dual_contour_field",
    "fi_mesh_create", "fi_mesh_parts", "fi_mesh_measure", "fi_mesh_select", "fi_mesh_simplify",
    "fi_mesh_smooth", "fi_mesh_normals", "fi_mesh_sample", "fi_mesh_deviation", "fi_mesh_register", "fi_points_register",
    "fi_group_sample", "fi_sample", "fi_sample_field",
    "fi_nearest", "fi_distance_field", "fi_points_create", "fi_points_nearest", "fi_points_distance_field", "fi_points_destroy",
    "fi_knn", "fi_points_knn", "fi_estimate_normals", "fi_points_estimate_normals",
    "fi_orient_normals", "fi_points_orient_normals",
    "fi_radius_count", "fi_points_radius_count", "fi_neighbour_distances", "fi_points_neighbour_distances",
    "fi_outliers_statistical", "fi_points_outliers_statistical", "fi_outliers_radius", "fi_points_outliers_radius", "fi_cloud_thin",
    "fi_mls_project", "fi_points_mls_project",
    "fi_cluster", "fi_points_cluster", "fi_cluster_measure", "fi_plane_fit", "fi_planes_segment",
    "fi_shape_fit", "fi_shapes_segment",
    "fi_points_describe", "fi_feature_match", "fi_align_correspondences",
    "fi_surface_create", "fi_surface_from_mesh", "fi_surface_distance", "fi_surface_distance_field", "fi_surface_destroy",
    "fi_surface_raycast", "fi_surface_count_hits", "fi_surface_contains", "fi_surface_signed_distance",
    "fi_surface_signed_distance_field",
    "fi_redistance", "fi_redistance_field",
    "fi_point_count", "fi_point_residuals", "fi_robust_reweight", "fi_reset_point_weights", "fi_solve_robust",
    "fi_depth_unproject", "fi_volume_create", "fi_volume_destroy", "fi_volume_load", "fi_volume_copy", "fi_volume_integrate",
    "fi_volume_constraints", "fi_add_volume",
    "fi_march_default_options", "fi_field_raycast", "fi_field_render", "fi_raycast_field", "fi_render_field", "fi_volume_raycast",
    "fi_volume_render",
    "fi_volume_set_channels", "fi_volume_channels", "fi_volume_colour_load", "fi_volume_colour_copy", "fi_volume_integrate_colour",
    "fi_volume_colour_sample", "fi_volume_render_colour", "fi_volume_colour_constraints",
]
FI_LOSS = {"huber": 0, "cauchy": 1, "tukey": 2}
FI_LOSS_NONE = -1
FI_REGISTER = {"plane": 0, "point": 1}
FI_THIN = {"mean": 0, "first": 1}
FI_SHAPE = {"sphere": 0, "cylinder": 1}
FI_DEPTH = {"z": 0, "range": 1}
FI_DEPTH_CAMERAS = 8
FI_MARCH = {"front": 0, "back": 1, "either": 2}
FI_MARCH_MAX_SAMPLES = 1 << 20


class FiWeights(C.Structure):
    _fields_ = [("data_pos", C.c_float), ("data_gradient", C.c_float),
                ("model_0", C.c_float), ("model_1", C.c_float), ("model_2", C.c_float),
                ("model_3", C.c_float), ("model_4", C.c_float), ("gradient_smoothness", C.c_float),
                ("value_kernel", C.c_int), ("gradient_kernel", C.c_int)]


class FiSolveOptions(C.Structure):
    _fields_ = [("tile", C.c_int), ("tile_size", C.c_int), ("cg", C.c_int),
                ("max_iterations", C.c_int), ("error_tolerance", C.c_float)]


class FiTriplet(C.Structure):
    _fields_ = [("row", C.c_int), ("col", C.c_int), ("value", C.c_float)]


class FiStats(C.Structure):
    _fields_ = [("num_unknowns", C.c_long), ("num_data_rows", C.c_long), ("num_cells", C.c_long),
                ("num_generic_rows", C.c_long), ("iterations", C.c_int), ("converged", C.c_int),
                ("rel_residual", C.c_double), ("assemble_ms", C.c_double), ("solve_ms", C.c_double),
                ("spmv_ms_avg", C.c_double), ("spmv_samples", C.c_int), ("spmv_bytes", C.c_double),
                ("restarts", C.c_int), ("verified_residual", C.c_double),
                ("num_levels", C.c_int), ("coarse_iterations", C.c_int),
                ("prec_ms_avg", C.c_double), ("prec_samples", C.c_int), ("prec_bytes", C.c_double),
                ("operator_applies", C.c_int), ("halo_exchanges", C.c_int), ("reductions", C.c_int),
                ("coarse_unconverged", C.c_int), ("field_estimate", C.c_double), ("field_per_residual", C.c_double),
                ("stop_residual", C.c_double), ("field_rounds", C.c_int)]


class FiRobustOptions(C.Structure):
    _fields_ = [("loss", C.c_int), ("tuning", C.c_float), ("scale", C.c_float), ("rounds", C.c_int),
                ("weight_tolerance", C.c_float)]


class FiRobustStats(C.Structure):
    _fields_ = [("rounds", C.c_int), ("iterations", C.c_int), ("scale", C.c_float), ("max_weight_change", C.c_float),
                ("points_used", C.c_long), ("points_zeroed", C.c_long), ("reweight_ms", C.c_double)]


class FiMeshPart(C.Structure):
    _fields_ = [("vertices", C.c_longlong), ("primitives", C.c_longlong), ("edges", C.c_longlong),
                ("boundary", C.c_longlong), ("irregular", C.c_longlong), ("size", C.c_double), ("enclosed", C.c_double),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3)]


class FiSmoothOptions(C.Structure):
    _fields_ = [("iterations", C.c_int), ("lam", C.c_float), ("mu", C.c_float), ("boundary", C.c_int),
                ("max_move", C.c_float), ("normals", C.c_int)]


class FiDeviation(C.Structure):
    _fields_ = [("queries", C.c_longlong), ("counted", C.c_longlong), ("beyond", C.c_longlong), ("invalid", C.c_longlong),
                ("at", C.c_longlong), ("max", C.c_double), ("mean", C.c_double), ("rms", C.c_double), ("where", C.c_float * 3)]


class FiRegisterOptions(C.Structure):
    _fields_ = [("mode", C.c_int), ("max_iterations", C.c_int), ("max_distance", C.c_float), ("rotation_tolerance", C.c_double),
                ("translation_tolerance", C.c_double), ("loss", C.c_int), ("tuning", C.c_float), ("scale", C.c_float)]


class FiRegistration(C.Structure):
    _fields_ = [("transform", C.c_double * 16), ("iterations", C.c_int), ("converged", C.c_int), ("fixed_mask", C.c_int),
                ("reserved", C.c_int), ("queries", C.c_longlong), ("counted", C.c_longlong), ("beyond", C.c_longlong),
                ("invalid", C.c_longlong), ("degenerate", C.c_longlong), ("rms", C.c_double), ("weighted_rms", C.c_double),
                ("last_rotation", C.c_double), ("last_translation", C.c_double)]


class FiOutlierStats(C.Structure):
    _fields_ = [("counted", C.c_long), ("kept", C.c_long), ("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double)]


class FiClusterStats(C.Structure):
    _fields_ = [("clusters", C.c_long), ("core", C.c_long), ("border", C.c_long), ("noise", C.c_long), ("non_finite", C.c_long)]


class FiClusterRow(C.Structure):
    _fields_ = [("count", C.c_long), ("core", C.c_long), ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("centroid", C.c_double * 3)]


class FiPlaneOptions(C.Structure):
    _fields_ = [("threshold", C.c_float), ("max_trials", C.c_long), ("confidence", C.c_double), ("refine", C.c_int),
                ("seed", C.c_ulonglong), ("axis", C.c_float * 3), ("min_cos", C.c_float)]


class FiPlaneModel(C.Structure):
    _fields_ = [("found", C.c_int), ("refits", C.c_int), ("inliers", C.c_long), ("candidates", C.c_long), ("trials", C.c_long),
                ("normal", C.c_double * 3), ("offset", C.c_double), ("rms", C.c_double)]


class FiShapeOptions(C.Structure):
    _fields_ = [("kind", C.c_int), ("threshold", C.c_float), ("r_min", C.c_float), ("r_max", C.c_float), ("normal_cos", C.c_float),
                ("max_trials", C.c_long), ("confidence", C.c_double), ("refine", C.c_int), ("seed", C.c_ulonglong)]


class FiShapeModel(C.Structure):
    _fields_ = [("found", C.c_int), ("kind", C.c_int), ("refits", C.c_int), ("inliers", C.c_long), ("candidates", C.c_long),
                ("trials", C.c_long), ("center", C.c_double * 3), ("axis", C.c_double * 3), ("radius", C.c_double),
                ("extent", C.c_double * 2), ("rms", C.c_double)]


class FiAlignOptions(C.Structure):
    _fields_ = [("threshold", C.c_float), ("similarity", C.c_float), ("max_trials", C.c_long), ("confidence", C.c_double),
                ("seed", C.c_ulonglong)]


class FiAlignment(C.Structure):
    _fields_ = [("found", C.c_int), ("pairs", C.c_long), ("live", C.c_long), ("trials", C.c_long), ("valid", C.c_long),
                ("inliers", C.c_long), ("transform", C.c_double * 16), ("rms", C.c_double)]


class FiCamera(C.Structure):
    _fields_ = [("pose", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int), ("height", C.c_int), ("kind", C.c_int)]


class FiMarchOptions(C.Structure):
    _fields_ = [("iso", C.c_float), ("step", C.c_float), ("min_weight", C.c_float), ("refine", C.c_int), ("side", C.c_int)]


class FiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (ERR_NAMES.get(code, "error %d" % code), msg))
        self.code = code


_LIB = None


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("field_interpolation_amd: %s is missing -- run `python -m field_interpolation_amd.build` "
                          "(hipcc, gfx950).  There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_double)
    L.fi_last_error.restype = C.c_char_p
    L.fi_device_count.argtypes = [ip]
    L.fi_ctx_create.argtypes = [C.POINTER(vp), C.c_int, ip, C.c_int]
    L.fi_ctx_create_slab.argtypes = [C.POINTER(vp), C.c_int, ip, C.c_int, C.c_int, C.c_int]
    L.fi_ctx_destroy.argtypes = [vp]
    L.fi_slab_range.argtypes = [vp, ip, ip]
    L.fi_slab_point_range.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.fi_slab_partition.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip]
    L.fi_halo_width.argtypes = [C.POINTER(FiWeights), ip]
    L.fi_comm_unique_id.argtypes = [vp]
    L.fi_comm_init.argtypes = [vp, vp]
    L.fi_comm_info.argtypes = [vp, C.POINTER(C.c_long)]
    L.fi_comm_init_host.argtypes = [vp, C.c_char_p, C.c_int]
    L.fi_set_model.argtypes = [vp, C.POINTER(FiWeights)]
    L.fi_add_points.argtypes = [vp, C.c_long, fp, fp, fp, fp, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int]
    L.fi_add_border_prior.argtypes = [vp, C.c_float]
    L.fi_add_rows_coo.argtypes = [vp, C.c_long, C.c_long, vp, fp, C.c_int]
    L.fi_assemble.argtypes = [vp]
    L.fi_clear_points.argtypes = [vp]
    L.fi_solve_cg.argtypes = [vp, fp, C.c_int, C.c_float, fp, ip, C.POINTER(C.c_float), C.c_int]
    L.fi_set_option.argtypes = [vp, C.c_int, C.c_double]
    L.fi_jacobi.argtypes = [vp, fp, C.c_int, C.c_float, fp, C.c_int]
    L.fi_tile_pass.argtypes = [vp, fp, C.c_int, fp, C.c_int]
    L.fi_comm_self_test.argtypes = [C.c_int, C.c_long]
    L.fi_error_map.argtypes = [vp, fp, fp, C.c_int]
    L.fi_get_solution_f64.argtypes = [vp, dp]
    L.fi_true_residual.argtypes = [vp, dp]
    L.fi_apply_AtA_f64.argtypes = [vp, dp, dp]
    L.fi_get_Atb_f64.argtypes = [vp, dp]
    L.fi_get_diag_f64.argtypes = [vp, dp]
    L.fi_get_stats.argtypes = [vp, C.POINTER(FiStats)]
    L.fi_time_apply.argtypes = [vp, C.c_int, dp]
    L.fi_memory_pool.argtypes = [C.c_longlong, C.POINTER(C.c_longlong)]
    L.fi_upscale_field.argtypes = [fp, C.c_int, ip, ip, fp, C.c_int]
    L.fi_group_create.argtypes = [C.POINTER(vp), C.c_int, ip, C.c_int, C.c_int]
    L.fi_group_destroy.argtypes = [vp]
    L.fi_group_size.argtypes = [vp]
    L.fi_group_rank.restype = vp
    L.fi_group_rank.argtypes = [vp, C.c_int]
    L.fi_group_assemble.argtypes = [vp]
    L.fi_group_solve_cg.argtypes = [vp, fp, C.c_int, C.c_float, fp, ip, C.POINTER(C.c_float)]
    L.fi_group_apply_AtA_f64.argtypes = [vp, dp, dp]
    L.fi_group_true_residual.argtypes = [vp, dp]
    L.fi_group_get_solution_f64.argtypes = [vp, dp]
    L.fi_group_tile_pass.argtypes = [vp, fp, C.c_int, fp]
    L.fi_group_error_map.argtypes = [vp, fp, fp]
    L.fi_group_iso_extract.argtypes = [vp, fp, C.c_float, C.POINTER(vp)]
    L.fi_iso_extract.argtypes = [vp, fp, C.c_float, C.c_int, C.POINTER(vp)]
    L.fi_iso_extract_field.argtypes = [fp, C.c_int, ip, C.c_float, C.c_int, C.POINTER(vp)]
    L.fi_dual_contour.argtypes = [vp, fp, fp, C.c_float, C.c_int, C.POINTER(vp)]
    L.fi_dual_contour_field.argtypes = [fp, fp, C.c_int, ip, C.c_float, C.c_int, C.POINTER(vp)]
    L.fi_mesh_info.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_long), ip]
    L.fi_mesh_copy.argtypes = [vp, fp, fp, vp, vp, C.c_int]
    L.fi_mesh_destroy.argtypes = [vp]
    L.fi_mesh_create.argtypes = [C.POINTER(vp), C.c_int, C.c_long, fp, fp, vp, C.c_long, vp, C.c_int]
    L.fi_mesh_parts.argtypes = [vp, C.POINTER(C.c_long), vp, vp, C.c_int]
    L.fi_mesh_measure.argtypes = [vp, C.c_long, vp, C.POINTER(C.c_long)]
    L.fi_mesh_select.argtypes = [vp, C.c_long, vp, C.POINTER(vp)]
    L.fi_mesh_simplify.argtypes = [vp, C.c_float, vp, C.c_int, vp, C.c_int, C.POINTER(vp)]
    L.fi_mesh_smooth.argtypes = [vp, C.POINTER(FiSmoothOptions), C.POINTER(vp)]
    L.fi_mesh_normals.argtypes = [vp, C.POINTER(vp)]
    L.fi_mesh_sample.argtypes = [vp, C.c_long, C.c_ulonglong, C.c_int, fp, fp, vp, C.c_int]
    L.fi_mesh_deviation.argtypes = [vp, vp, C.c_long, C.c_ulonglong, C.c_float, C.POINTER(FiDeviation), C.POINTER(FiDeviation), fp,
                                    C.c_int]
    L.fi_mesh_register.argtypes = [vp, vp, C.c_long, fp, C.POINTER(FiRegisterOptions), dp, C.POINTER(FiRegistration), fp, fp, C.c_int]
    L.fi_points_register.argtypes = [vp, fp, C.c_long, fp, C.POINTER(FiRegisterOptions), dp, C.POINTER(FiRegistration), fp, fp,
                                     C.c_int]
    L.fi_group_sample.argtypes = [vp, fp, C.c_long, fp, C.c_int, C.c_float, fp, fp]
    L.fi_sample.argtypes = [vp, fp, C.c_long, fp, C.c_int, C.c_float, fp, fp, C.c_int]
    L.fi_sample_field.argtypes = [fp, C.c_int, ip, C.c_long, fp, C.c_int, C.c_float, fp, fp, C.c_int]
    L.fi_points_create.argtypes = [C.POINTER(vp), C.c_int, C.c_long, fp, C.c_int]
    # the operations on a point set: fi_<op> over a context's data points and fi_points_<op> over a set of its own take the
    # same arguments after the handle (fi_points_distance_field: a lattice first, which a context brings along)
    POINT_OPS = {
        "nearest": [C.c_long, fp, C.c_float, fp, vp, C.c_int],
        "distance_field": [C.c_float, fp, vp, C.c_int],
        "knn": [C.c_long, fp, C.c_int, C.c_float, fp, vp, C.c_int],
        "estimate_normals": [C.c_int, C.c_float, C.c_int, fp, C.c_long, fp, fp, C.c_int],
        "orient_normals": [C.c_int, C.c_float, C.c_int, fp, C.c_long, fp, vp, C.c_int],
        "radius_count": [C.c_long, fp, C.c_float, C.c_int, vp, C.c_int],
        "neighbour_distances": [C.c_int, C.c_float, fp, fp, vp, C.c_int],
        "outliers_statistical": [C.c_int, C.c_float, C.c_float, vp, C.POINTER(FiOutlierStats), C.c_int],
        "outliers_radius": [C.c_float, C.c_int, vp, C.POINTER(C.c_long), C.c_int],
        "mls_project": [C.c_long, fp, C.c_int, C.c_float, C.c_int, C.c_float, fp, fp, fp, fp, vp, C.c_int],
        "cluster": [C.c_float, C.c_int, vp, vp, C.POINTER(FiClusterStats), C.c_int],
    }
    for op, args in POINT_OPS.items():
        getattr(L, "fi_" + op).argtypes = [vp] + args
        getattr(L, "fi_points_" + op).argtypes = [vp] + ([ip] if op == "distance_field" else []) + args
    L.fi_points_destroy.argtypes = [vp]
    L.fi_cloud_thin.argtypes = [C.c_int, C.c_long, fp, fp, fp, C.c_float, C.POINTER(C.c_float), C.c_int, fp, fp, fp, vp, vp, vp,
                                C.POINTER(C.c_long), C.c_int]
    L.fi_cluster_measure.argtypes = [C.c_int, C.c_long, fp, vp, vp, C.c_long, C.POINTER(FiClusterRow), C.c_int]
    L.fi_plane_fit.argtypes = [C.c_int, C.c_long, fp, vp, C.POINTER(FiPlaneOptions), C.POINTER(FiPlaneModel), vp, C.c_int]
    L.fi_planes_segment.argtypes = [C.c_int, C.c_long, fp, vp, C.POINTER(FiPlaneOptions), C.c_int, C.c_long, vp,
                                    C.POINTER(FiPlaneModel), ip, C.c_int]
    L.fi_shape_fit.argtypes = [C.c_int, C.c_long, fp, fp, vp, C.POINTER(FiShapeOptions), C.POINTER(FiShapeModel), vp, C.c_int]
    L.fi_shapes_segment.argtypes = [C.c_int, C.c_long, fp, fp, vp, C.POINTER(FiShapeOptions), C.c_int, C.c_long, vp,
                                    C.POINTER(FiShapeModel), ip, C.c_int]
    L.fi_points_describe.argtypes = [vp, fp, C.c_int, C.c_float, fp, vp, C.c_int]
    L.fi_feature_match.argtypes = [C.c_int, C.c_long, fp, vp, C.c_long, fp, vp, vp, fp, C.c_int]
    L.fi_align_correspondences.argtypes = [C.c_long, fp, C.c_long, fp, C.c_long, vp, vp, C.POINTER(FiAlignOptions),
                                           C.POINTER(FiAlignment), vp, C.c_int]
    L.fi_surface_create.argtypes = [C.POINTER(vp), C.c_int, C.c_long, fp, C.c_long, vp, C.c_int]
    L.fi_surface_from_mesh.argtypes = [C.POINTER(vp), vp]
    L.fi_surface_distance.argtypes = [vp, C.c_long, fp, C.c_float, fp, vp, fp, C.c_int]
    L.fi_surface_distance_field.argtypes = [vp, ip, C.c_float, fp, vp, C.c_int]
    L.fi_surface_destroy.argtypes = [vp]
    L.fi_surface_raycast.argtypes = [vp, C.c_long, fp, fp, C.c_float, C.c_float, fp, vp, fp, C.c_int]
    L.fi_surface_count_hits.argtypes = [vp, C.c_long, fp, fp, C.c_float, C.c_float, C.c_int, vp, C.c_int]
    L.fi_surface_contains.argtypes = [vp, C.c_long, fp, C.POINTER(C.c_float), vp, C.c_int]
    L.fi_surface_signed_distance.argtypes = [vp, C.c_long, fp, C.c_float, fp, vp, fp, C.c_int]
    L.fi_surface_signed_distance_field.argtypes = [vp, ip, C.c_float, fp, vp, C.c_int]
    L.fi_redistance.argtypes = [vp, fp, C.c_float, C.c_int, C.c_float, fp, vp, C.POINTER(vp), C.c_int]
    L.fi_redistance_field.argtypes = [fp, C.c_int, ip, C.c_float, C.c_int, C.c_float, fp, vp, C.POINTER(vp), C.c_int]
    L.fi_point_count.argtypes = [vp, C.POINTER(C.c_long)]
    L.fi_point_residuals.argtypes = [vp, fp, fp, C.c_int]
    L.fi_robust_reweight.argtypes = [vp, fp, C.POINTER(FiRobustOptions), fp, C.POINTER(C.c_float), C.c_int]
    L.fi_reset_point_weights.argtypes = [vp]
    L.fi_solve_robust.argtypes = [vp, fp, C.POINTER(FiRobustOptions), C.c_int, C.c_float, fp, fp, C.POINTER(FiRobustStats), C.c_int]
    L.fi_depth_unproject.argtypes = [C.POINTER(FiCamera), fp, C.c_float, fp, fp, fp, vp, C.c_int]
    L.fi_volume_create.argtypes = [C.POINTER(vp), C.c_int, ip, C.c_float, C.c_float]
    L.fi_volume_destroy.argtypes = [vp]
    L.fi_volume_load.argtypes = [vp, fp, fp, C.c_int]
    L.fi_volume_copy.argtypes = [vp, fp, fp, C.c_int]
    L.fi_volume_integrate.argtypes = [vp, C.c_long, C.POINTER(FiCamera), fp, fp, fp, C.c_float, C.c_int]
    L.fi_volume_constraints.argtypes = [vp, C.c_float, C.POINTER(C.c_long), fp, fp, fp, C.c_int]
    L.fi_add_volume.argtypes = [vp, vp, C.c_float, C.c_int, C.c_float]
    mo, cam = C.POINTER(FiMarchOptions), C.POINTER(FiCamera)
    L.fi_march_default_options.argtypes = [mo]
    L.fi_field_raycast.argtypes = [fp, fp, C.c_int, ip, mo, C.c_long, fp, fp, C.c_float, C.c_float, fp, fp, fp, vp, C.c_int]
    L.fi_field_render.argtypes = [fp, fp, ip, mo, cam, fp, fp, fp, fp, C.c_int]
    L.fi_raycast_field.argtypes = [vp, fp, mo, C.c_long, fp, fp, C.c_float, C.c_float, fp, fp, fp, vp, C.c_int]
    L.fi_render_field.argtypes = [vp, fp, mo, cam, fp, fp, fp, fp, C.c_int]
    L.fi_volume_raycast.argtypes = [vp, mo, C.c_long, fp, fp, C.c_float, C.c_float, fp, fp, fp, vp, C.c_int]
    L.fi_volume_render.argtypes = [vp, mo, cam, fp, fp, fp, fp, C.c_int]
    L.fi_volume_set_channels.argtypes = [vp, C.c_int]
    L.fi_volume_channels.argtypes = [vp, C.POINTER(C.c_int)]
    L.fi_volume_colour_load.argtypes = [vp, fp, fp, C.c_int]
    L.fi_volume_colour_copy.argtypes = [vp, fp, fp, C.c_int]
    L.fi_volume_integrate_colour.argtypes = [vp, C.c_long, cam, fp, fp, fp, C.c_float, fp, C.c_float, C.c_int]
    L.fi_volume_colour_sample.argtypes = [vp, C.c_float, C.c_long, fp, fp, vp, C.c_int]
    L.fi_volume_render_colour.argtypes = [vp, mo, cam, C.c_float, fp, fp, fp, fp, fp, C.c_int]
    L.fi_volume_colour_constraints.argtypes = [vp, C.c_float, C.POINTER(C.c_long), fp, fp, fp, C.c_int]
    for name in SYMBOLS:
        getattr(L, name)          # AttributeError if the .so lacks a declared symbol
    _LIB = L
    return L


def check(code):
    if code != FI_OK:
        raise FiError(code, lib().fi_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    check(lib().fi_device_count(C.byref(n)))
    return n.value


def memory_pool(keep_bytes=-1):
    """fi_memory_pool: device memory of destroyed contexts kept for the next one, on the current device.  Frees it down
    to keep_bytes (0: all of it; negative: nothing) and returns the bytes that stay cached."""
    left = C.c_longlong(0)
    check(lib().fi_memory_pool(int(keep_bytes), C.byref(left)))
    return left.value
