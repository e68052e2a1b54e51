// fi_jacobi.h -- the eigenvectors of a symmetric 2 x 2 or 3 x 3 matrix in fp64 by a cyclic Jacobi iteration of a fixed number
// of sweeps: the arithmetic tests/normals_reference.py (SWEEPS, point-cloud normals: fi_knn.hip) and
// tests/simplify_reference.py (quadric placement: fi_simplify.hip) reproduce bit for bit.  One rounding per operation: the
// units that include this are built with -ffp-contract=off.
#pragma once

namespace fi {
namespace jacobi {

constexpr int kSweeps = 6;

// one Jacobi rotation of the pair (P, Q) of the symmetric matrix A (both triangles kept) and the vector matrix V (columns)
template <int D, int P, int Q>
__device__ inline void rotate(double (&A)[D][D], double (&V)[D][D])
{
	const double apq = A[P][Q];
	if (apq == 0.0) { return; }
	const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
	const double t     = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
	const double c     = 1.0 / sqrt(t * t + 1.0);
	const double s     = t * c;
	const double tap   = t * apq;
	A[P][P] = A[P][P] - tap;
	A[Q][Q] = A[Q][Q] + tap;
	A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
	for (int r = 0; r < D; ++r) {
		if (r == P || r == Q) { continue; }
		const double arp = A[r][P], arq = A[r][Q];
		A[r][P] = A[P][r] = c * arp - s * arq;
		A[r][Q] = A[Q][r] = s * arp + c * arq;
	}
#pragma unroll
	for (int r = 0; r < D; ++r) {
		const double vrp = V[r][P], vrq = V[r][Q];
		V[r][P] = c * vrp - s * vrq;
		V[r][Q] = s * vrp + c * vrq;
	}
}

// A's diagonal becomes the eigenvalues, V (the identity on entry) their vectors as columns.  A fixed number of sweeps, no
// early exit: the result is defined by the count alone
template <int D>
__device__ inline void jacobi_sweeps(double (&A)[D][D], double (&V)[D][D])
{
#pragma unroll 1
	for (int sweep = 0; sweep < kSweeps; ++sweep) {
		rotate<D, 0, 1>(A, V);
		if constexpr (D == 3) {
			rotate<D, 0, 2>(A, V);
			rotate<D, 1, 2>(A, V);
		}
	}
}

}  // namespace jacobi
}  // namespace fi
