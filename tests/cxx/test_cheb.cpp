// fi_cheb.h on the host (no device, no Python in the process; built with the address and undefined-behaviour sanitizers by
// tests/test_cheb.py).  Over lam x ratio x steps:
//   bits:     c1 and c2 of every step equal the loop every call site wrote out before the header existed, transcribed below;
//   property: the scalar smoother x_1 = 1 / theta, x_(k+1) = (1 + c1) x_k - c1 x_(k-1) + c2 (1 - a x_k) leaves the residual
//             1 - a x_k = T_k((theta - a) / delta) / T_k(sigma), the scaled Chebyshev polynomial, for a below, inside and
//             above the interval -- to 1e-12 absolute against a long double evaluation (the formulas' own fp64 deviation on
//             this grid and these steps is 4.3e-14).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "fi_cheb.h"

static int failures = 0;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static long double cheb_t(int k, long double t)  // T_k(t) by the three-term recurrence
{
	long double t0 = 1.0L, t1 = t;
	if (k == 0) { return t0; }
	for (int j = 1; j < k; ++j) {
		const long double t2 = 2.0L * t * t1 - t0;
		t0 = t1;
		t1 = t2;
	}
	return t1;
}

int main()
{
	const double lams[] = {1.0, 1.37, 2.9, 7.5, 16.0}, ratios[] = {1.5, 4.0, 10.0, 30.0, 100.0};
	double worst = 0.0;
	for (double lam : lams) {
		for (double ratio : ratios) {
			for (int steps = 1; steps <= 11; ++steps) {
				// the loop as the call sites had it
				const double hi = 1.1 * lam, lo = hi / ratio;
				const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo), sigma = theta / delta;
				double c1s[11], c2s[11];
				double rho = 1.0 / sigma;
				for (int k = 1; k <= steps; ++k) {
					const double rho_new = 1.0 / (2.0 * sigma - rho);
					c1s[k - 1] = rho_new * rho;
					c2s[k - 1] = 2.0 * rho_new / delta;
					rho = rho_new;
				}
				const fi::ChebInterval iv(lam, ratio);
				if (!same_bits(iv.theta, theta) || !same_bits(iv.delta, delta) || !same_bits(iv.sigma, sigma)) {
					std::printf("interval differs: lam %g ratio %g\n", lam, ratio);
					++failures;
				}
				fi::ChebRecurrence rec(iv);
				for (int k = 1; k <= steps; ++k) {
					rec.next();
					if (!same_bits(rec.c1, c1s[k - 1]) || !same_bits(rec.c2, c2s[k - 1])) {
						std::printf("step %d of %d differs: lam %g ratio %g\n", k, steps, lam, ratio);
						++failures;
					}
				}
				for (int i = 0; i < 23; ++i) {
					const double a = 0.5 * lo + (1.05 * hi - 0.5 * lo) * i / 22.0;
					const long double t = (static_cast<long double>(theta) - a) / delta;
					fi::ChebRecurrence r(iv);
					double x_prev = 0.0, x = 1.0 / iv.theta;
					for (int k = 1;; ++k) {  // x is x_k
						const double want = static_cast<double>(cheb_t(k, t) / cheb_t(k, static_cast<long double>(sigma)));
						const double dev = std::fabs((1.0 - a * x) - want);
						worst = dev > worst ? dev : worst;
						if (!(dev <= 1e-12)) {
							std::printf("residual off by %g: lam %g ratio %g a %g step %d\n", dev, lam, ratio, a, k);
							++failures;
						}
						if (k > steps) { break; }
						r.next();
						const double x_next = (1.0 + r.c1) * x - r.c1 * x_prev + r.c2 * (1.0 - a * x);
						x_prev = x;
						x = x_next;
					}
				}
			}
		}
	}
	std::printf("worst deviation from the Chebyshev polynomial: %.3g\n", worst);
	if (failures) {
		std::printf("%d checks failed\n", failures);
		return 1;
	}
	std::printf("all cheb checks passed\n");
	return 0;
}
