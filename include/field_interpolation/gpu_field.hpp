// gpu_field.hpp -- the matrix-free fast path for lattice problems (not in the reference).
//
// GpuLatticeField is the GPU twin of LatticeField: same call sequence (add_field_constraints, add_points /
// add_value_constraint / add_gradient_constraint, then a solver), but no row is ever written to host memory:
// everything goes straight to libfi_hip (include/fi_hip.h).
#pragma once

#include <limits>
#include <memory>
#include <vector>

#include "field_interpolation.hpp"

struct fi_ctx;
struct fi_volume;

namespace field_interpolation {

// Robust fits (include/fi_hip.h, "robust fits"): data points reweighted by their residuals between solves.
struct RobustOptions
{
	enum class Loss { kHuber = 0, kCauchy = 1, kTukey = 2 };
	Loss  loss             = Loss::kHuber;
	float tuning           = 0; // the loss's constant c; 0: its default (1.345, 2.385, 4.685)
	float scale            = 0; // the residual scale s; 0: 1.4826 x the median residual
	int   rounds           = 5; // reweighted solves at most
	float weight_tolerance = 0; // end when no weight factor moved by this much; 0: never
};

// One connected part of a mesh (include/fi_hip.h fi_mesh_part, field for field): exact counts, the fp64 measures, the box.
struct MeshPart
{
	long long vertices, primitives, edges, boundary, irregular;
	double    size, enclosed; // area and enclosed volume (2-D: length and enclosed area); enclosed means something if closed()
	float     lo[3], hi[3];
	bool      closed() const { return boundary == 0 && irregular == 0; }
	long long euler() const { return vertices - edges + primitives; } // of a 3-D part
};

// Rigid registration (include/fi_hip.h fi_mesh_register): the options and the result, field for field.
struct RegisterOptions
{
	enum class Mode { kPlane = 0, kPoint = 1 };
	enum class Loss { kNone = -1, kHuber = 0, kCauchy = 1, kTukey = 2 };
	Mode   mode                  = Mode::kPlane;
	int    max_iterations        = 30;
	float  max_distance          = std::numeric_limits<float>::infinity(); // pairs further apart are left out
	double rotation_tolerance    = 1e-6; // the loop ends when a step turns and shifts by no more than these
	double translation_tolerance = 1e-6;
	Loss   loss                  = Loss::kNone;
	float  tuning                = 0; // the loss's constant c; 0: its default
	float  scale                 = 0; // the residual scale s: > 0 with a loss
};

struct Registration
{
	double    transform[16]; // (ndim + 1) x (ndim + 1), row-major, in the first entries
	int       iterations, converged, fixed_mask, reserved;
	long long queries, counted, beyond, invalid, degenerate;
	double    rms, weighted_rms, last_rotation, last_translation;
};

// The figures of the statistical outlier rule (include/fi_hip.h fi_outlier_stats), field for field.
struct OutlierStats
{
	long   counted, kept;
	double mean, stddev, threshold;
};

// The totals of a clustering (include/fi_hip.h fi_cluster_stats), field for field.
struct ClusterStats
{
	long clusters, core, border, noise, non_finite;
};

// A hyperplane found by segment_plane / segment_planes (include/fi_hip.h fi_plane_model), field for field.
struct PlaneModel
{
	int    found, refits;
	long   inliers, candidates, trials;
	double normal[3], offset, rms;
};

// A sphere (circle) or cylinder found by segment_shape / segment_shapes (include/fi_hip.h fi_shape_model), field for field.
struct ShapeModel
{
	int    found, kind, refits;
	long   inliers, candidates, trials;
	double center[3], axis[3], radius, extent[2], rms;
};
enum class Shape { kSphere = 0, kCylinder = 1 };

// A pinhole camera for depth images (include/fi_hip.h fi_camera): pose = the rows of [R | t], world (lattice coordinates) to
// camera; it looks along +z, image x goes right, y down; pixel (row, col) has its centre at (col + 0.5, row + 0.5).  range:
// the depth is the distance along the pixel's ray (false: along the optical axis).
struct DepthCamera
{
	float pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
	float fx = 1, fy = 1, cx = 0, cy = 0;
	int   width = 0, height = 0;
	bool  range = true;
};

// How a ray is marched through a lattice field to its first crossing of `iso` (include/fi_hip.h fi_march_options): a sample
// every `step` lattice units, `refine` (0 .. 16) bisections of the first bracket, and which crossings count: kFront, from
// outside (f >= iso) to inside (f < iso), kBack, the opposite ones, or kEither.  min_weight: with a weight array (a volume's), a
// sample counts only where every corner of its cell has weight > 0 and >= min_weight.
enum class MarchSide { kFront = 0, kBack = 1, kEither = 2 };
struct MarchOptions
{
	float     iso = 0, step = 1, min_weight = 0;
	int       refine = 4;
	MarchSide side = MarchSide::kFront;
};

// A truncated signed distance volume over a 3-D lattice on the device: tsdf (1 at first, in units of `truncation`) and weight
// (0 at first) for every lattice point, x fastest.  integrate() fuses depth images into it; constraints() and
// GpuLatticeField::add_volume hand its band to the solve.  The contract is include/fi_hip.h fi_volume_integrate.  Every call
// returns false where the library refused it; valid() is false when the constructor's arguments were refused.
class DepthVolume
{
public:
	DepthVolume(const std::vector<int>& sizes, float truncation, float max_weight = 64.0f);
	~DepthVolume();
	DepthVolume(const DepthVolume&) = delete;
	DepthVolume& operator=(const DepthVolume&) = delete;

	bool   valid() const { return volume_ != nullptr; }
	size_t num_voxels() const { return voxels_; }
	// depths: the cameras' images back to back, image s of height_s x width_s floats; incidences (empty, or laid out the same
	// way: depth_to_points gives them); image_weights (empty, or one per image)
	bool integrate(const std::vector<DepthCamera>& cameras, const std::vector<float>& depths,
	               const std::vector<float>& incidences = std::vector<float>(),
	               const std::vector<float>& image_weights = std::vector<float>(), float min_incidence = 0.5f);
	bool copy(std::vector<float>* tsdf, std::vector<float>* weight) const;              // either may be null
	bool load(const std::vector<float>& tsdf, const std::vector<float>& weight);        // resumes a fusion
	// the voxels with weight >= min_weight, weight > 0 and |tsdf| < 1 in ascending index: positions (3 floats each), values
	// tsdf * truncation, weights W / max_weight; any may be null
	bool constraints(std::vector<float>* positions, std::vector<float>* values, std::vector<float>* weights, float min_weight = 0) const;
	// Rays against the surface the volume holds (its tsdf under its weights, read in place; iso 0 is the surface): t per ray
	// origins[i] + t directions[i] (3 floats each, t_min <= t <= t_max), +inf without a crossing, NaN for a ray that is none;
	// optional hit positions and unit gradients (3 floats each) and sides (+1 front, -1 back, 0 none).  The contract is
	// include/fi_hip.h fi_field_raycast.
	bool raycast(const std::vector<float>& origins, const std::vector<float>& directions, std::vector<float>* t,
	             const MarchOptions& options = MarchOptions(), std::vector<float>* positions = nullptr, std::vector<float>* normals = nullptr,
	             std::vector<signed char>* side = nullptr, float t_min = 0, float t_max = std::numeric_limits<float>::infinity()) const;
	// The depth image of that surface seen by `camera`, in the camera's kind, +inf where a pixel's ray meets none; optional
	// positions, normals and incidences in depth_to_points' layout, so that integrate() can take the image as it is.
	bool render(const DepthCamera& camera, std::vector<float>* depth, const MarchOptions& options = MarchOptions(),
	            std::vector<float>* positions = nullptr, std::vector<float>* normals = nullptr, std::vector<float>* incidence = nullptr) const;
	// Colour (include/fi_hip.h fi_volume_integrate_colour): set_channels(1 .. 4) once gives every lattice point that many fp32
	// channels and a colour weight, 0 at first; channels() is 0 before.  integrate_colour is integrate() with the images'
	// colours beside the depths: pixel-interleaved, height_s x width_s x channels floats per image, the images back to back; a
	// voxel within band * truncation of the surface averages its pixel's colour under the depth sample's weight, and tsdf and
	// weight come out as integrate() leaves them.
	bool set_channels(int channels);
	int  channels() const;
	bool integrate_colour(const std::vector<DepthCamera>& cameras, const std::vector<float>& depths, const std::vector<float>& colours,
	                      const std::vector<float>& incidences = std::vector<float>(),
	                      const std::vector<float>& image_weights = std::vector<float>(), float min_incidence = 0.5f, float band = 1.0f);
	// the channels, planar (channel k of voxel i at k num_voxels() + i), and the colour weights; either may be null
	bool copy_colours(std::vector<float>* colours, std::vector<float>* colour_weight) const;
	bool load_colours(const std::vector<float>& colours, const std::vector<float>& colour_weight);  // resumes a fusion
	// the colour at positions (3 floats each): channels() floats per point, the average of the corners of the point's cell that
	// carry a colour (colour weight > 0 and >= min_weight) under the trilinear weights; NaN and valid 0 where none does or the
	// point lies outside the lattice.  The vertices of iso_surface's mesh are such positions.
	bool sample_colours(const std::vector<float>& positions, std::vector<float>* colours, std::vector<unsigned char>* valid = nullptr,
	                    float min_weight = 0) const;
	// render() and the colour image beside it: sample_colours(hit positions, colour_min_weight), NaN where a pixel has no hit
	bool render_colour(const DepthCamera& camera, std::vector<float>* depth, std::vector<float>* colours,
	                   const MarchOptions& options = MarchOptions(), float colour_min_weight = 0, std::vector<float>* positions = nullptr,
	                   std::vector<float>* normals = nullptr, std::vector<float>* incidence = nullptr) const;
	// the voxels with colour weight > 0 and >= min_weight in ascending index: positions (3 floats each), colours (channels()
	// floats each), weights Wc / max_weight; any may be null
	bool colour_constraints(std::vector<float>* positions, std::vector<float>* colours, std::vector<float>* weights, float min_weight = 0) const;
	const fi_volume* handle() const { return volume_; }

private:
	fi_volume* volume_ = nullptr;
	size_t     voxels_ = 0;
};

class GpuLatticeField
{
public:
	// double_precision: keep all lattice vectors in fp64 (for tolerances below ~1e-5).
	explicit GpuLatticeField(const std::vector<int>& sizes, bool double_precision = false);
	~GpuLatticeField();
	GpuLatticeField(const GpuLatticeField&) = delete;
	GpuLatticeField& operator=(const GpuLatticeField&) = delete;

	const std::vector<int>& sizes() const { return sizes_; }
	size_t num_unknowns() const;

	// Large lattices (the reference's recipe is app code: src/sdf_field.cpp:272-288).  `levels` coarser replicas of
	// the problem are built on the GPU; a zero-length guess then starts from the coarse-to-fine cascade.
	// multigrid: V-cycle preconditioned CG over the levels (needed by SDF problems from oriented points).
	// mixed_precision (double_precision fields): CG in fp64, the V-cycle on an fp32 replica.
	void set_levels(int levels, bool multigrid = false, bool mixed_precision = false);
	// Any solver option of the C ABI by number (include/fi_hip.h FI_OPT_*: e.g. FI_OPT_FIELD_TOLERANCE = 12 stops by the field,
	// FI_OPT_MG_KCYCLE = 13 corrects that many coarse levels by two flexible-CG steps each -- a third of the iterations on SDF
	// problems).  false: the library refused the value.
	bool set_option(int option, double value);

	void add_field_constraints(const Weights& weights);
	bool add_value_constraint(const float pos[], float value, float weight);
	bool add_value_constraint_nearest_neighbor(const float pos[], const float gradient[], float value, float weight);
	bool add_gradient_constraint(const float pos[], const float gradient[], float weight, GradientKernel kernel);
	void add_points(float value_weight, ValueKernel value_kernel, float gradient_weight, GradientKernel gradient_kernel,
	                int num_points, const float positions[], const float* normals, const float* point_weights);
	// The border prior of the reference's SDF application (src/sdf_field.cpp:218-246: options.boundary_weight): every
	// border lattice point is pulled towards its distance to the nearest point added so far.  After add_points.
	bool add_border_prior(float weight);

	// solve_sparse_linear_with_guess / solve_tiled_with_guess / jacobi_iterations of the reference.
	// An empty result means failure (wrong guess length, solver breakdown), as in the reference.
	std::vector<float> solve_with_guess(const std::vector<float>& guess, int max_iterations, float error_tolerance);
	// No guess: starts from the coarse-to-fine cascade when set_levels() built levels, from zero otherwise.
	std::vector<float> solve(int max_iterations, float error_tolerance);
	std::vector<float> solve_tiled_with_guess(const std::vector<float>& guess, const SolveOptions& options);
	std::vector<float> jacobi_iterations(const std::vector<float>& guess, int num_iterations, float weight);
	// generate_error_map(field.eq.triplets, solution, field.eq.rhs) of the reference, from the rows on the device.
	std::vector<float> generate_error_map(const std::vector<float>& solution);

	// The iso-contour (2-D: segments, 2 indices each) or iso-surface (3-D: triangles, 3 indices each) f = iso of the last
	// solution, extracted where it lives on the device -- what src/sdf_field.cpp:605-613 (iso_surface) does on the host.
	// vertices: ndim floats per vertex in lattice units; normals (optional): ndim floats per vertex, towards increasing f.
	// The contract is include/fi_hip.h fi_iso_extract.  false: no solution yet, or the library refused (non-finite values).
	bool iso_surface(float iso, std::vector<float>* vertices, std::vector<int>* indices,
	                 std::vector<float>* normals = nullptr) const;

	// The dual contour f = iso of the last solution, on the device (include/fi_hip.h fi_dual_contour): one vertex per crossed
	// cell, fitted to the planes of the corner gradients so that sharp corners and edges survive; 2-D segments or 3-D
	// triangles, vertices and normals as iso_surface.  gradients (optional): ndim floats per lattice point, interleaved, x
	// fastest; without them, central differences of f - iso.  false: no solution yet, or the library refused the call.
	bool dual_contour(float iso, std::vector<float>* vertices, std::vector<int>* indices, std::vector<float>* normals = nullptr,
	                  const std::vector<float>* gradients = nullptr) const;

	// iso_surface (dual = false) or dual_contour with central differences (dual = true) of the last solution, cut down to
	// chosen connected parts on the device before the one copy to the host: the parts of size (area; 2-D: length) >= min_size
	// and, with largest >= 0, only the `largest` largest of them (ties go to the part with the smaller first vertex).
	// parts (optional): one row per part of the mesh returned, numbered by their smallest vertex.  The contract is
	// include/fi_hip.h fi_mesh_parts .. fi_mesh_select.  false: no solution yet, or the library refused the call.
	bool iso_surface_parts(float iso, bool dual, int largest, double min_size, std::vector<float>* vertices, std::vector<int>* indices,
	                       std::vector<float>* normals = nullptr, std::vector<MeshPart>* parts = nullptr) const;

	// iso_surface_parts' mesh (largest < 0 and min_size <= 0: every part) made coarser on the device before the one copy to the
	// host: the vertices in one cube of edge `cell` (lattice units, the grid starts at 0) become one vertex, placed at the minimum
	// of the cluster's quadric error (placement 0, FI_SIMPLIFY_QUADRIC: corners and edges survive) or at its mean (1,
	// FI_SIMPLIFY_MEAN); collapsed and repeated primitives are dropped.  The contract is include/fi_hip.h fi_mesh_simplify.
	// false: no solution yet, or the library refused the call.
	bool iso_surface_simplified(float iso, bool dual, float cell, int placement, int largest, double min_size, std::vector<float>* vertices,
	                            std::vector<int>* indices, std::vector<float>* normals = nullptr) const;

	// iso_surface_parts' mesh (largest < 0 and min_size <= 0: every part) made smoother on the device before the one copy to the
	// host: `iterations` times, every vertex moves towards the average of its neighbours by the factor lambda and then by the
	// factor mu (Taubin's fairing; mu = 0: plain Laplacian smoothing), the vertices of open edges stay where they are
	// (FI_SMOOTH_BOUNDARY_FIXED), no vertex ends further than max_move from where it started (0: no limit), and the normals are
	// recomputed from the smoothed primitives.  The contract is include/fi_hip.h fi_mesh_smooth.  false: no solution yet, or the
	// library refused the call.
	bool iso_surface_smoothed(float iso, bool dual, int iterations, float lambda, float mu, float max_move, int largest, double min_size,
	                          std::vector<float>* vertices, std::vector<int>* indices, std::vector<float>* normals = nullptr) const;

	// `n` oriented points spread over iso_surface (dual = false) or dual_contour (dual = true) of the last solution by area
	// (2-D: by length), made on the device with one copy to the host at the end: positions and, if asked, normals (the
	// extractor's vertex normals interpolated and normalised, FI_SAMPLE_NORMALS_VERTEX), ndim floats per point, in ascending
	// primitive order; the same `seed` gives the same points.  What sdf_from_points wants of another lattice: a field re-fitted
	// or re-meshed at another resolution.  The contract is include/fi_hip.h fi_mesh_sample.  false: no solution yet, a surface
	// with nothing to sample, or the library refused the call.
	bool iso_surface_points(float iso, bool dual, long n, unsigned long long seed, std::vector<float>* positions,
	                        std::vector<float>* normals = nullptr) const;

	// The rigid transform that lays `n` points (`positions`, ndim floats per point, lattice units) over iso_surface (dual =
	// false) or dual_contour (dual = true) of the last solution by iterated closest points: the mesh is extracted, searched and
	// registered to on the device and never copied to the host.  `transform` receives the (ndim + 1) x (ndim + 1) row-major
	// matrix [R t; 0 1] that maps the points to the surface; `stats`, if asked, the whole result.  The contract is
	// include/fi_hip.h fi_mesh_register.  false: no solution yet, or the library refused the call.
	bool register_points(float iso, bool dual, long n, const float* positions, const RegisterOptions& options,
	                     std::vector<double>* transform, Registration* stats = nullptr) const;

	// Values (and, if asked, gradients: ndim floats per point) of the last solution at `positions` (ndim floats per point,
	// global lattice coordinates, x fastest), sampled where the solution lives on the device: multilinear, or Catmull-Rom
	// with cubic = true; points outside the lattice get NaN.  The contract is include/fi_hip.h fi_sample.  false: no
	// solution yet, or the library refused the call.
	bool sample(const std::vector<float>& positions, std::vector<float>* values, std::vector<float>* gradients = nullptr,
	            bool cubic = false) const;

	// Exact nearest data points: for each of `queries` (ndim floats per point, lattice units, x fastest) the distance to the
	// nearest point given to add_points so far (the border prior's rows are not data points) and, if asked, that point's index
	// in the order the points were added; +inf / -1 beyond max_distance or without points, NaN / -1 for a non-finite query.
	// The contract is include/fi_hip.h fi_nearest.  false: the library refused the call.
	bool nearest(const std::vector<float>& queries, std::vector<float>* distances, std::vector<long long>* indices = nullptr,
	             float max_distance = std::numeric_limits<float>::infinity()) const;
	// The k nearest data points of each query, nearest first, equal distances by ascending index (1 <= k <= 32): k distances
	// (and indices) per query; entries that do not exist are +inf / -1 at the end.  The contract is include/fi_hip.h fi_knn.
	bool knn(const std::vector<float>& queries, int k, std::vector<float>* distances, std::vector<long long>* indices = nullptr,
	         float max_distance = std::numeric_limits<float>::infinity()) const;
	// Normals (ndim floats per point) of the data points given to add_points so far, in that order, each fitted to its k
	// nearest points (itself included) on the device.  viewpoints: ndim floats (one sensor position) or ndim per point --
	// normals look at it, which is outward; empty: each normal's largest component is positive, NOT a consistent
	// orientation.  variation (optional): lambda_min / sum(lambda) per point.  The contract is include/fi_hip.h
	// fi_estimate_normals.  false: the library refused the call.
	bool estimate_normals(std::vector<float>* normals, int k = 16, const std::vector<float>& viewpoints = std::vector<float>(),
	                      std::vector<float>* variation = nullptr,
	                      float max_distance = std::numeric_limits<float>::infinity()) const;
	// One consistent sign for `normals` (ndim floats per data point, in place) per connected component of the points'
	// k-nearest-neighbour graph, spread along its minimum spanning forest on the device; without viewpoints a component's
	// highest point on the last axis looks up that axis, with viewpoints (ndim floats, or ndim per point) they vote per
	// component.  components (optional): each point's component (its smallest point index, -1 for a point without a usable
	// normal).  The contract is include/fi_hip.h fi_orient_normals.  false: the library refused the call.
	bool orient_normals(std::vector<float>* normals, int k = 16, const std::vector<float>& viewpoints = std::vector<float>(),
	                    std::vector<long long>* components = nullptr,
	                    float max_distance = std::numeric_limits<float>::infinity()) const;
	// How many data points lie within `radius` of each query (a point exactly on the radius included), at most `limit`: the
	// search stops there; -1 for a non-finite query.  The contract is include/fi_hip.h fi_radius_count.
	bool radius_count(const std::vector<float>& queries, float radius, std::vector<int>* counts,
	                  int limit = std::numeric_limits<int>::max()) const;
	// Per data point, in the order the points were added: the mean distance to its k nearest OTHER points within
	// max_distance (1 <= k <= 32; the point itself is left out by its index), the distance to the last of them and their
	// number; +inf, +inf, 0 without a neighbour, NaN, NaN, 0 for a non-finite point.  Any of the three may be null, not all.
	// mean or kth to the power ndim is the density weight add_points takes as point_weights.  The contract is
	// include/fi_hip.h fi_neighbour_distances.
	bool neighbour_distances(int k, std::vector<float>* mean, std::vector<float>* kth = nullptr, std::vector<int>* counts = nullptr,
	                         float max_distance = std::numeric_limits<float>::infinity()) const;
	// The statistical outlier rule: keep[i] = 1 where point i's mean neighbour distance is at most mean + std_ratio * standard
	// deviation of that figure over the cloud.  stats (optional): counted, kept, mean, stddev, threshold.  The contract is
	// include/fi_hip.h fi_outliers_statistical.
	bool statistical_outliers(int k, float std_ratio, std::vector<unsigned char>* keep, OutlierStats* stats = nullptr,
	                          float max_distance = std::numeric_limits<float>::infinity()) const;
	// keep[i] = 1 where point i is finite and has at least min_neighbours other points within radius.  The contract is
	// include/fi_hip.h fi_outliers_radius.
	bool radius_outliers(float radius, int min_neighbours, std::vector<unsigned char>* keep, long* num_kept = nullptr) const;
	// The data points, in the order they were added, each projected onto the plane (degree 1) or quadric (degree 2) fitted
	// to its k nearest points within `radius` on the device (moving least squares): what takes the measurement noise off a
	// scan.  positions, normals: ndim floats per point; curvature: the fitted surface's mean curvature, in 1 / length; order:
	// 2 the quadric, 1 the plane, 0 nothing fitted (the point stays); any of the four may be null, not all.  guide_normals
	// (ndim floats per point, or empty): the sign the normals come back with.  max_move limits how far a point may go.  The
	// field's own points stay as they are.  With k = 16 on a noisy surface the quadric amplifies noise: keep k = 32 for
	// degree 2.  The contract is include/fi_hip.h fi_mls_project.  false: the library refused the call.
	bool smooth_points(float radius, std::vector<float>* positions, std::vector<float>* normals = nullptr, int k = 32, int degree = 2,
	                   float max_move = std::numeric_limits<float>::infinity(),
	                   const std::vector<float>& guide_normals = std::vector<float>(), std::vector<float>* curvature = nullptr,
	                   std::vector<unsigned char>* order = nullptr) const;
	// The band of a DepthVolume over this lattice as data points: every voxel with weight >= min_weight and |tsdf| < 1 a value
	// constraint tsdf * truncation of point weight W / max_weight, formed on the device; no gradient rows.  The contract is
	// include/fi_hip.h fi_add_volume.  false: the library refused the call.
	bool add_volume(const DepthVolume& volume, float value_weight, ValueKernel value_kernel = ValueKernel::kNearestNeighbor,
	                float min_weight = 0);
	// The clusters of the data points, in the order the points were added: labels[i] is point i's cluster, -1 for noise and
	// for a non-finite point.  A point is core when min_points points, itself included, lie within eps of it (min_points = 1:
	// plain Euclidean clustering); core points within eps of each other share a cluster, numbered by their lowest core point;
	// any other point takes the cluster of its nearest core point within eps.  core (optional): 1 for a core point.  stats
	// (optional): clusters, core, border, noise, non_finite.  The contract is include/fi_hip.h fi_cluster.
	bool cluster_points(float eps, int min_points, std::vector<int>* labels, std::vector<unsigned char>* core = nullptr,
	                    ClusterStats* stats = nullptr) const;
	// nearest() of every lattice point (x fastest): num_unknowns() distances (and indices)
	bool distance_field(std::vector<float>* distances, std::vector<long long>* indices = nullptr,
	                    float max_distance = std::numeric_limits<float>::infinity()) const;
	// The signed distance of every lattice point (x fastest) to the last solution's own iso-surface f = iso, searched on the
	// device: fi_iso_extract's mesh (inside f < iso) or, with dual = true, fi_dual_contour's (inside f - iso <= 0); negative
	// inside, +-inf beyond max_distance.  primitives (optional): the nearest primitive of that mesh per point, -1 beyond
	// max_distance.  The contract is include/fi_hip.h fi_redistance.  false: no solution yet, or the library refused the call.
	bool redistance(std::vector<float>* out, float iso = 0, bool dual = false,
	                float max_distance = std::numeric_limits<float>::infinity(), std::vector<long long>* primitives = nullptr) const;
	// The closest hit of each ray origins[i] + t directions[i] (ndim floats each, directions not normalised, 0 <= t <= t_max)
	// with the last solution's own iso-surface f = iso -- the mesh redistance() searches, made the same way: t per ray, +inf
	// without a hit, NaN for a ray that is none.  primitives (optional): the primitive of that mesh each ray hits, or -1.
	// The contract is include/fi_hip.h fi_surface_raycast.  false: no solution yet, or the library refused the call.
	bool raycast(const std::vector<float>& origins, const std::vector<float>& directions, std::vector<float>* t, float iso = 0,
	             bool dual = false, float t_max = std::numeric_limits<float>::infinity(),
	             std::vector<long long>* primitives = nullptr) const;
	// The same rays marched through the last solution itself (2-D or 3-D), no mesh in between: DepthVolume::raycast's outputs,
	// ndim floats per position and normal.  The contract is include/fi_hip.h fi_raycast_field.  false: no solution yet, or the
	// library refused the call.
	bool march(const std::vector<float>& origins, const std::vector<float>& directions, std::vector<float>* t,
	           const MarchOptions& options = MarchOptions(), std::vector<float>* positions = nullptr, std::vector<float>* normals = nullptr,
	           std::vector<signed char>* side = nullptr, float t_min = 0, float t_max = std::numeric_limits<float>::infinity()) const;
	// The depth image of the last solution's iso-level seen by `camera` (3-D): DepthVolume::render's outputs.  The contract is
	// include/fi_hip.h fi_render_field.
	bool render(const DepthCamera& camera, std::vector<float>* depth, const MarchOptions& options = MarchOptions(),
	            std::vector<float>* positions = nullptr, std::vector<float>* normals = nullptr, std::vector<float>* incidence = nullptr) const;

	// Iteratively reweighted least squares for data with gross errors: a plain solve, then up to options.rounds solves, each
	// after the data points were reweighted by their residuals against the previous field (fi_solve_robust; every solve as
	// solve() runs it).  point_weights (optional): the weight factor omega of every data point, in the order the points were
	// added.  Afterwards the field holds the last weights.  An empty result means failure; last_iterations() counts all solves.
	// Residuals measure disagreement with the fit: an outlier the field can bend to keeps its weight.
	std::vector<float> solve_robust(const RobustOptions& options, int max_iterations, float error_tolerance,
	                                std::vector<float>* point_weights = nullptr);
	// Every data point's residual against the last solution: the root of the summed squares of its rows at unit point weight,
	// -1 for a point that emits no row.  false: no solution yet, or the library refused the call.
	bool point_residuals(std::vector<float>* residuals) const;

	int    last_iterations() const { return iterations_; }
	float  last_error() const { return error_; }
	size_t num_data_rows() const;   // rows accepted from points (what eq.rhs.size() would have grown by)

private:
	bool assemble();
	fi_ctx*          ctx_ = nullptr;
	std::vector<int> sizes_;
	bool             dirty_ = true;
	int              iterations_ = 0;
	float            error_ = 0;
};

// sdf_from_points without the triplet list.
std::unique_ptr<GpuLatticeField> gpu_sdf_from_points(const std::vector<int>& sizes, const Weights& weights,
                                                     int num_points, const float positions[], const float* normals,
                                                     const float* point_weights);

// A point cloud thinned on a uniform grid of spacing `cell` on the device, no lattice needed: one output point per occupied
// cell in ascending cell order -- the members' mean position (and value, and their summed, normalised normal), or with
// first = true the member with the lowest index bit for bit.  positions: ndim floats per point; normals (ndim per point)
// and values (one per point) may be empty, and so may origin (zeros).  Non-finite points are left out.  out_counts: members
// per cell; out_indices: a cell's lowest member; cell_map: per input point its output, -1 for a point left out; all
// optional.  The contract is include/fi_hip.h fi_cloud_thin.  false: the library refused the call.
bool thin_points(int ndim, const std::vector<float>& positions, float cell, std::vector<float>* out_positions,
                 const std::vector<float>& normals = std::vector<float>(), std::vector<float>* out_normals = nullptr,
                 const std::vector<float>& values = std::vector<float>(), std::vector<float>* out_values = nullptr,
                 const std::vector<float>& origin = std::vector<float>(), bool first = false, std::vector<int>* out_counts = nullptr,
                 std::vector<long long>* out_indices = nullptr, std::vector<int>* cell_map = nullptr);

// GpuLatticeField::smooth_points of a point cloud of its own, no lattice needed (ndim = 2 or 3; positions: ndim floats per
// point): every point projected onto the local surface of its neighbours.  The contract is include/fi_hip.h fi_mls_project.
bool smooth_points(int ndim, const std::vector<float>& positions, float radius, std::vector<float>* out_positions,
                   std::vector<float>* out_normals = nullptr, int k = 32, int degree = 2,
                   float max_move = std::numeric_limits<float>::infinity(),
                   const std::vector<float>& guide_normals = std::vector<float>(), std::vector<float>* curvature = nullptr,
                   std::vector<unsigned char>* order = nullptr);

// A depth image (camera.height x camera.width floats) as oriented points on the device, in pixel order: positions and normals
// (3 floats each), incidence (the cosine between the normal and the ray back to the eye) and valid (1: a finite depth > 0);
// any may be null, not all four.  A neighbour takes part in a pixel's normal when its depth is valid and within max_jump of
// the pixel's.  An invalid pixel has a NaN position; a pixel without a normal a zero normal and a zero incidence.  The
// contract is include/fi_hip.h fi_depth_unproject.  false: the library refused the call.
bool depth_to_points(const DepthCamera& camera, const std::vector<float>& depth, std::vector<float>* positions,
                     std::vector<float>* normals = nullptr, std::vector<float>* incidence = nullptr,
                     std::vector<unsigned char>* valid = nullptr, float max_jump = std::numeric_limits<float>::infinity());

// The dominant plane (ndim = 3) or line (ndim = 2) of a point cloud on the device, no lattice needed: RANSAC with an exact
// inlier count (a point within `threshold` of the plane, inclusive, is an inlier), then `refine` least-squares refits.
// positions: ndim floats per point.  At most max_trials hypotheses, fewer once the best would have been drawn with probability
// `confidence` (0: never stop early).  mask (one byte per point, may be empty): the points that take part.  axis (ndim
// floats, may be empty) and min_cos: only planes with |normal . axis| >= min_cos |axis|.  inliers (optional): one byte per
// point.  Every figure is defined bit for bit: the contract is include/fi_hip.h fi_plane_fit.  false: the library refused
// the call.
bool segment_plane(int ndim, const std::vector<float>& positions, float threshold, PlaneModel* model,
                   std::vector<unsigned char>* inliers = nullptr, long max_trials = 1024, double confidence = 0.999, int refine = 2,
                   unsigned long long seed = 0, const std::vector<unsigned char>& mask = std::vector<unsigned char>(),
                   const std::vector<float>& axis = std::vector<float>(), float min_cos = 0.0f);
// Up to max_planes planes peeled off one after the other: plane p is segment_plane with seed + p over the points no earlier
// plane took; the first plane with fewer than min_inliers inliers ends the loop and is not recorded.  labels[i]: the plane
// that took point i, or -1.  The contract is include/fi_hip.h fi_planes_segment.
bool segment_planes(int ndim, const std::vector<float>& positions, float threshold, int max_planes, std::vector<int>* labels,
                    std::vector<PlaneModel>* models, long min_inliers = 0, long max_trials = 1024, double confidence = 0.999,
                    int refine = 2, unsigned long long seed = 0, const std::vector<unsigned char>& mask = std::vector<unsigned char>(),
                    const std::vector<float>& axis = std::vector<float>(), float min_cos = 0.0f);

// The dominant sphere (a circle with ndim = 2) or cylinder (ndim = 3, needs normals) of a point cloud on the device: RANSAC with
// an exact inlier count (a point whose distance from the shape is within `threshold`, inclusive, is an inlier), then `refine`
// algebraic least-squares refits.  positions and normals: ndim floats per point; normals may be empty for a sphere.  Only radii
// in [r_min, r_max] are considered.  normal_cos > 0: an inlier's normal also lies within that angle of the shape's, either way
// round.  max_trials, confidence, mask and inliers as segment_plane's.  Every figure is defined bit for bit: the contract is
// include/fi_hip.h fi_shape_fit.  false: the library refused the call.
bool segment_shape(int ndim, Shape kind, const std::vector<float>& positions, const std::vector<float>& normals, float threshold,
                   ShapeModel* model, std::vector<unsigned char>* inliers = nullptr, float r_min = 0.0f,
                   float r_max = std::numeric_limits<float>::infinity(), float normal_cos = 0.0f, long max_trials = 1024,
                   double confidence = 0.999, int refine = 2, unsigned long long seed = 0,
                   const std::vector<unsigned char>& mask = std::vector<unsigned char>());
// Up to max_shapes shapes of one kind peeled off one after the other: shape p is segment_shape with seed + p over the points no
// earlier shape took; the first shape with fewer than min_inliers inliers ends the loop and is not recorded.  labels[i]: the
// shape that took point i, or -1.  The contract is include/fi_hip.h fi_shapes_segment.
bool segment_shapes(int ndim, Shape kind, const std::vector<float>& positions, const std::vector<float>& normals, float threshold,
                    int max_shapes, std::vector<int>* labels, std::vector<ShapeModel>* models, long min_inliers = 0, float r_min = 0.0f,
                    float r_max = std::numeric_limits<float>::infinity(), float normal_cos = 0.0f, long max_trials = 1024,
                    double confidence = 0.999, int refine = 2, unsigned long long seed = 0,
                    const std::vector<unsigned char>& mask = std::vector<unsigned char>());

// What every point's neighbourhood looks like, as 33 floats that survive a turn and a shift of the cloud (fast point feature
// histograms over the k nearest points and the normals; 3 floats per point each), on the device.  valid (optional): one byte
// per point, 0 where a point has no descriptor (its 33 floats are zeros).  The contract is include/fi_hip.h
// fi_points_describe.  false: the library refused the call.
bool describe_points(const std::vector<float>& positions, const std::vector<float>& normals, std::vector<float>* features,
                     std::vector<unsigned char>* valid = nullptr, int k = 32,
                     float max_distance = std::numeric_limits<float>::infinity());
// For every row of a (dim floats each) the nearest row of b, equal distances to the smallest index; -1 and +inf for a row that
// is masked out (valid_a / valid_b: one byte per row, may be empty), non-finite or without a partner.  The contract is
// include/fi_hip.h fi_feature_match.
bool match_features(int dim, const std::vector<float>& a, const std::vector<float>& b, std::vector<long long>* indices,
                    std::vector<float>* distances = nullptr, const std::vector<unsigned char>& valid_a = std::vector<unsigned char>(),
                    const std::vector<unsigned char>& valid_b = std::vector<unsigned char>());
// The result of align_correspondences (include/fi_hip.h fi_alignment), field for field.
struct Alignment
{
	int    found;
	long   pairs, live, trials, valid, inliers;
	double transform[16], rms;
};
// The rotation and shift that carries the most matched pairs (source[src_index[c]], target[tgt_index[c]]) to within
// `threshold` of each other, by RANSAC on the device: 3 floats per point; transform is 4 x 4 row-major, source to target.
// inliers (optional): one byte per pair.  Every figure is defined bit for bit: the contract is include/fi_hip.h
// fi_align_correspondences.
bool align_correspondences(const std::vector<float>& source, const std::vector<float>& target, const std::vector<long long>& src_index,
                           const std::vector<long long>& tgt_index, float threshold, Alignment* out,
                           std::vector<unsigned char>* inliers = nullptr, float similarity = 0.9f, long max_trials = 100000,
                           double confidence = 0.999, unsigned long long seed = 0);

// The stateless solver calls of sparse_linear.hpp keep device contexts between calls, keyed by shape and precision (at
// most six, systems of up to 2^20 unknowns only; larger systems get a context per call): the per-frame caller's latency
// (src/bipolar_2d.cpp:730).  This frees the calling thread's cached contexts (they are freed at thread exit otherwise)
// and the device memory the library keeps of destroyed contexts (fi_memory_pool).
void clear_context_cache();

// Whether this thread's last stateless solver call (solve_sparse_linear_with_guess, solve_tiled_with_guess, ...) found the
// note add_field_constraints / add_points leave beside the rows (LinearEquation::recipe) still valid and applied those rows
// matrix-free on their lattice -- the path of the reference's own call sequence, sdf_from_points followed by
// solve_tiled_with_guess(field.eq, ...) (src/sdf_field.cpp:251-304) -- instead of uploading every triplet.
bool last_solve_was_matrix_free();

} // namespace field_interpolation
