// The regularised incomplete gamma function and its quantile, without Boost: what the discrete Gamma model of the build (hu_dg_model,
// hu_host.cpp) and the rate categories of hmmufotu-amd-tree --gamma (hu_gamma_rates, hu_gamma_host.cpp) share.  Host only; every
// translation unit keeps a copy of its own (static), compiled under its own floating-point flags.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

/* regularised lower incomplete gamma P(a, x): the power series below a + 1, Lentz's continued fraction for Q above */
static inline double dg_gamma_p(double a, double x) {
	if(!(x > 0)) return 0.0;
	if(std::isinf(x)) return 1.0;
	const double lpre = a * std::log(x) - x - std::lgamma(a);
	const double eps = 1e-17;
	if(x < a + 1) {
		double ap = a, del = 1.0 / a, sum = del;
		for(int it = 0; it < 100000; ++it) {
			ap += 1; del *= x / ap; sum += del;
			if(std::fabs(del) < std::fabs(sum) * eps) break;
		}
		return sum * std::exp(lpre);
	}
	const double tiny = 1e-300;
	double b = x + 1 - a, c = 1 / tiny, d = 1 / b, h = d;
	for(int i = 1; i < 100000; ++i) {
		const double an = -i * (i - a);
		b += 2;
		d = an * d + b; if(std::fabs(d) < tiny) d = tiny;
		c = b + an / c; if(std::fabs(c) < tiny) c = tiny;
		d = 1 / d;
		const double del = d * c;
		h *= del;
		if(std::fabs(del - 1) < eps) break;
	}
	return 1.0 - std::exp(lpre) * h;
}

/* the p-quantile of Gamma(shape a, scale 1): bisection on log x down to adjacent doubles, then Newton steps on P(a, x) = p */
static inline double dg_gamma_quantile(double a, double p) {
	if(p <= 0) return 0.0;
	if(p >= 1) return std::numeric_limits<double>::infinity();
	double hi = std::max(a, 1.0);
	while(dg_gamma_p(a, hi) < p) hi *= 2;
	double lo = hi;
	for(int it = 0; it < 4000 && lo > 0 && dg_gamma_p(a, lo) > p; ++it) lo *= 0.5;
	if(!(lo > 0)) return 0.0;
	for(int it = 0; it < 400; ++it) {
		const double mid = std::sqrt(lo) * std::sqrt(hi);
		if(!(mid > lo && mid < hi)) break;
		if(dg_gamma_p(a, mid) < p) lo = mid; else hi = mid;
	}
	double x = std::sqrt(lo) * std::sqrt(hi);
	for(int it = 0; it < 3; ++it) {
		const double pdf = std::exp((a - 1) * std::log(x) - x - std::lgamma(a));
		if(!(pdf > 0)) break;
		const double nx = x - (dg_gamma_p(a, x) - p) / pdf;
		if(!(nx > 0) || std::fabs(nx - x) > 1e-10 * x) break;
		x = nx;
	}
	return x;
}
