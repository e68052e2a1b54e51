"""field_interpolation_amd -- MI355X-native solver core for emilk/field_interpolation's hot path.

Host-side mirror of the reference interface (field_interpolation.hpp / sparse_linear.hpp) over the
C ABI of libfi_hip.so (include/fi_hip.h).  All arithmetic runs in hand-written HIP kernels on the
GPU; importing the API without the built library raises ImportError (no CPU fallback).
"""
from .api import (GradientKernel, IsoMesh, LatticeField, LatticeGroup, MeshParts, PointIndex, SolveOptions, SurfaceIndex,  # noqa: F401
                  ValueKernel, Weights, dual_contour, generate_error_map, iso_surface, jacobi_iterations, keep_parts, merge_meshes, mesh_parts, mesh_to_sdf, redistance, sample_field, select_parts,
                  simplify_mesh, smooth_mesh, mesh_normals, sample_mesh, mesh_deviation, register_points, apply_transform, thin_points, clean_points, smooth_points,
                  cluster_points, cluster_measure, keep_clusters, segment_plane, segment_planes, segment_sphere, segment_cylinder, segment_shapes,
                  match_features, align_correspondences, register_global,
                  Camera, DepthVolume, camera_look_at, depth_to_points, sdf_from_depth, raycast_field, render_field,
                  sdf_from_points, sdf_from_unoriented_points, solve_sparse_linear_exact, solve_sparse_linear_with_guess, solve_tiled_with_guess, upscale_field)
from ._capi import FiError, memory_pool  # noqa: F401
