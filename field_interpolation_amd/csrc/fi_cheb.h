// fi_cheb.h -- the Chebyshev interval and three-term recurrence of every polynomial in the solver: the preconditioner of
// the polynomial PCG (fi_poly.hip), the V-cycle's smoothers and their twins in the tail program (fi_multigrid.hip).  The
// constants reach the kernels as bits, and the tail program's cycle is vcycle()'s only while both take them from here.
//     x_1 = Dinv b / theta (from zero),   x_(k+1) = (1 + c1) x_k - c1 x_(k-1) + c2 Dinv (b - A x_k)
// The caller chooses lam (its bound of the largest eigenvalue) and ratio; the interval is [1.1 lam / ratio, 1.1 lam].
// (Plain C++, no device call: tests/cxx/test_cheb.cpp checks it on the host.  The order of the operations is part of the
// contract: solutions are compared bit for bit, tests/test_gpu_solve_frame.py.)
#pragma once

namespace fi {

struct ChebInterval {
	double theta, delta, sigma;
	ChebInterval(double lam, double ratio)
	{
		const double hi = 1.1 * lam, lo = hi / ratio;
		theta = 0.5 * (hi + lo);
		delta = 0.5 * (hi - lo);
		sigma = theta / delta;
	}
};

// next() once per polynomial step: c1 and c2 are then that step's
struct ChebRecurrence {
	double c1 = 0.0, c2 = 0.0;
	explicit ChebRecurrence(const ChebInterval& iv) : sigma_(iv.sigma), delta_(iv.delta), rho_(1.0 / iv.sigma) {}
	void next()
	{
		const double rho_new = 1.0 / (2.0 * sigma_ - rho_);
		c1   = rho_new * rho_;
		c2   = 2.0 * rho_new / delta_;
		rho_ = rho_new;
	}

private:
	double sigma_, delta_, rho_;
};

}  // namespace fi
