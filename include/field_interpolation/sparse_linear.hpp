// sparse_linear.hpp -- drop-in for field_interpolation/sparse_linear.hpp of emilk/field_interpolation.
//
// Same namespace, type names, member names, member order, defaults and function signatures as the reference
// header (sparse_linear.hpp:8-80), so existing callers compile unchanged.  The solver bodies live in
// libfield_interpolation (field_interpolation_amd/cxx/) and run on an MI355X through the C ABI of fi_hip.h: the
// triplets are uploaded as generic sparse rows and A^T A x = A^T b is iterated on the GPU (no Eigen, no explicit
// A^T A matrix).  An empty result vector always means "the solver failed", as in the reference.
#pragma once

#include <initializer_list>
#include <iosfwd>
#include <memory>
#include <vector>

namespace field_interpolation {

namespace detail { struct Recipe; }  // (how the rows were made: libfield_interpolation's note to itself, see below)

// ---- the system in coordinate form ------------------------------------------------------------------------

struct Triplet  // A[row][col] = value; 12 bytes
{
	int row, col;
	float value;
	Triplet() {}
	Triplet(int r, int c, float v) : row(r), col(c), value(v) {}
};

struct LinearEquation  // A x = rhs; entries sharing (row, col) add up
{
	std::vector<Triplet> triplets;
	std::vector<float> rhs;
	// Not in the original: add_field_constraints / add_points of this library note beside the rows what they appended
	// (model weights, the point arrays).  A solver that finds the noted rows unchanged applies them matrix-free on the
	// lattice instead of uploading them as triplets; rows the note does not cover go up as before.  "Unchanged" is checked
	// over every noted triplet and right-hand side at every solve: rows edited in place are solved as edited, through the
	// triplets.  Callers never touch it (brace-initialisation, copies and moves of the two members above work as in the original).
	std::shared_ptr<const detail::Recipe> recipe;
};

struct LinearEquationPair  // one term of a row: value * x[column]
{
	int column;
	float value;
};

struct Weight
{
	float value;
};

struct Rhs
{
	float value;
};

struct SolveOptions
{
	bool tile = false;             // run the tile pre-pass (exact solves of tile_size^D tiles) first
	int tile_size = 16;
	bool cg = true;                // run the iterative phase
	int max_iterations = 0;        // 0: solver default
	float error_tolerance = 1e-3f; // 0: float epsilon
};

// ---- building rows ------------------------------------------------------------------------------------------

// weight * sum(pair.value * x[pair.column]) = weight * rhs.  A zero weight adds nothing, zero coefficients are
// skipped, and a row left without coefficients adds no right-hand side either.
void add_equation(LinearEquation* eq, Weight weight, Rhs rhs, std::initializer_list<LinearEquationPair> pairs);

// One equation per line:  rhs = v * xCOL + v * xCOL ...
std::ostream& operator<<(std::ostream& os, const LinearEquation& eq);

// ---- solving (least squares over eq.rhs.size() rows) -------------------------------------------------------

// "Exact" / "fast": the normal equations iterated on the GPU to a relative residual of 1e-12 in double / 1e-7 in float.
// An empty vector where a factorisation would fail -- an unknown without any equation (zero pivot) -- or on a solver
// breakdown.  A well-posed but badly conditioned system whose attainable residual stays above the target returns its best
// iterate (one line on stderr); an iteration budget given to the *_with_guess calls buys that many operator applications
// (two CG steps per BiCGSTAB step of the original).
std::vector<float> solve_sparse_linear_exact(const LinearEquation& eq, int num_columns);
std::vector<float> solve_sparse_linear_fast(const LinearEquation& eq, int num_columns);

// Iterative, from a guess holding one value per unknown.  max_iterations 0 = default (twice the problem size),
// error_tolerance 0 = default (float epsilon).
std::vector<float> solve_sparse_linear_with_guess(const LinearEquation& eq, const std::vector<float>& guess,
                                                  int max_iterations, float error_tolerance);

// Weighted Jacobi sweeps on the normal equations (weight 2/3 converges fast, 1 can oscillate);
// num_iterations <= 0 returns the guess.
std::vector<float> jacobi_iterations(const LinearEquation& eq, const std::vector<float>& guess, const int num_iterations,
                                     const float weight);

// Guess, optional tile pre-pass, optional iterative phase, on a lattice of the given sizes.  A guess whose
// length is not the number of lattice points gives an empty result.
std::vector<float> solve_tiled_with_guess(const LinearEquation& eq, const std::vector<float>& guess,
                                          const std::vector<int>& sizes, const SolveOptions& options);

}  // namespace field_interpolation
