// The rates, the checks, the host path and the passes of the fit under the discrete Gamma of rates: hmmufotu-amd-tree
// --ml-lengths --gamma K --host, the reference of the device tests, and what tests/san/gamma_driver.cpp runs under the sanitizers.  No
// HIP headers: a plain C++ compiler builds this file.  The sweep of a category is hu_blen_host_sweep at the lengths rate_c blen, the
// rounds of a fit are hu_blen_rounds (hu_blen_host.cpp), the arithmetic of a column is hu_tree_gamma.h's, shared with the kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "hu_tree_gamma.h"
#include "hu_gamma_fn.h"

extern "C" int hu_gamma_rates(int32_t K, double alpha, double* rates) try {
	if(K < 1 || K > HU_MAX_DGK || !rates) { hu_set_error("hu_gamma_rates: %d categories: 1 to %d", K, HU_MAX_DGK); return HU_ERR_ARG; }
	if(!(alpha >= HU_GAMMA_ALPHA_MIN) || !(alpha <= HU_GAMMA_ALPHA_MAX)) { hu_set_error("hu_gamma_rates: alpha %g: %g to %g", alpha, HU_GAMMA_ALPHA_MIN, HU_GAMMA_ALPHA_MAX); return HU_ERR_ARG; }
	/* alpha b_i = the i / K quantile of Gamma(shape alpha, scale 1); the mean of Gamma(alpha, rate alpha) below b is P(alpha + 1, alpha b) */
	double below = 0.0;
	for(int i = 0; i < K; ++i) {
		const double upto = i + 1 < K ? dg_gamma_p(alpha + 1, dg_gamma_quantile(alpha, (i + 1) / static_cast<double>(K))) : 1.0;
		rates[i] = K * (upto - below);
		below = upto;
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_gamma_rates"); }

/* the messages, the rows, the column values, the step's scratch beyond LDS, 1 MB of slack */
extern "C" int64_t hu_gamma_need(int32_t n, int32_t cs_len, int32_t K) {
	if(n < 1 || cs_len < 1 || K < 1 || K > HU_MAX_DGK) return 0;
	const int64_t cells = (int64_t) n * cs_len;
	const int64_t scratch = hu_gamma_in_lds(K, cs_len) ? 0 : hu_gamma_slab(n) * 32 * K * (int64_t) cs_len;
	return 64 * K * cells + cells + 8 * (int64_t)(K + 1) * cs_len + scratch + (1 << 20);
}

extern "C" void hu_gamma_default_opts(hu_gamma_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	hu_blen_default_opts(&o->blen);
	o->k = 4; o->max_outer = 10; o->alpha = 0.0; o->eps_ll = 0.01;
}

int hu_gamma_check(const char* fn, const hu_gamma_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp) {
	if(!o) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	hu_blen_opts bo = o->blen;
	if(bo.mem_budget > 0) bo.mem_budget = 0;                  /* the need held against it is this family's, below */
	const int rc = hu_blen_check(fn, &bo, n, cs_len, parent, blen, seq, dg_k, tp);
	if(rc != HU_OK) return rc;
	if(o->k < 1 || o->k > HU_MAX_DGK) { hu_set_error("%s: %d rate categories: 1 to %d", fn, o->k, HU_MAX_DGK); return HU_ERR_ARG; }
	if(o->alpha != 0.0 && (!(o->alpha >= HU_GAMMA_ALPHA_MIN) || !(o->alpha <= HU_GAMMA_ALPHA_MAX))) {
		hu_set_error("%s: alpha %g: %g to %g, or 0 to estimate it", fn, o->alpha, HU_GAMMA_ALPHA_MIN, HU_GAMMA_ALPHA_MAX); return HU_ERR_ARG; }
	if(!(o->eps_ll > 0) || !std::isfinite(o->eps_ll)) { hu_set_error("%s: eps_ll %g: above 0", fn, o->eps_ll); return HU_ERR_ARG; }
	if(o->max_outer < 1) { hu_set_error("%s: %d passes: at least 1", fn, o->max_outer); return HU_ERR_ARG; }
	if(o->passes_cap < 0 || (o->passes_cap > 0 && !o->passes)) { hu_set_error("%s: %d pass records without a place for them", fn, o->passes_cap); return HU_ERR_ARG; }
	const int64_t need = hu_gamma_need(n, cs_len, o->k);
	if(o->blen.mem_budget > 0 && need > o->blen.mem_budget) {
		hu_set_error("%s: %d nodes of %d columns in %d rate categories need %lld bytes (%lld of them for the messages), the memory budget is %lld bytes", fn, n, cs_len, o->k,
			(long long) need, (long long)(64 * (int64_t) o->k * n * cs_len), (long long) o->blen.mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

namespace {
struct GammaHost : HuGammaRun {
	const HuBlenTopo& tp; const HuBlenModel& m; int32_t K; int64_t L; const int32_t* parent; const int8_t* seq; double lo, hi;
	size_t cells4;                                            /* doubles of one category's messages of one direction */
	std::vector<double> up, down, len, lr;
	GammaHost(const HuBlenTopo& t, const HuBlenModel& model, int32_t k, int32_t cs_len, const int32_t* par, const int8_t* rows, double lo_, double hi_)
		: tp(t), m(model), K(k), L(cs_len), parent(par), seq(rows), lo(lo_), hi(hi_), cells4((size_t) t.n * (size_t) cs_len * 4),
		  up(cells4 * (size_t) k), down(cells4 * (size_t) k), len((size_t) t.n), lr((size_t) 3 * k, 0.0), rate_((size_t) k, 1.0) {}
	std::vector<double> rate_;
	int set_rates(const double* rate) override { rate_.assign(rate, rate + K); hu_gamma_lr(m, K, rate, lr.data()); return HU_OK; }
	int sweep(const double* blen, bool withDown) override {
		for(int32_t c = 0; c < K; ++c) {
			for(int32_t u = 0; u < tp.n; ++u) len[(size_t) u] = rate_[(size_t) c] * blen[u];
			hu_blen_host_sweep(tp, m, parent, L, len.data(), seq, up.data() + cells4 * (size_t) c, withDown ? down.data() + cells4 * (size_t) c : nullptr);
		}
		return HU_OK;
	}
	int loglik(double* per_col, double* per_cat, double* ll) override {
		std::vector<double> v((size_t) K * (size_t) L);
		for(int32_t c = 0; c < K; ++c) {
			const double* root = up.data() + cells4 * (size_t) c + (size_t) tp.root * (size_t) L * 4;
			for(int64_t j = 0; j < L; ++j) v[(size_t) c * (size_t) L + (size_t) j] = hu_blen_host_loglik_column(m, root + j * 4);
		}
		if(per_cat) memcpy(per_cat, v.data(), v.size() * 8);
		double sum = 0;
		for(int64_t j = 0; j < L; ++j) { const double x = hu_gamma_logmean(v.data() + j, L, K); if(per_col) per_col[j] = x; sum += x; }
		*ll = sum;
		return HU_OK;
	}
	int step(const double* t, double* tStar, double* f, double* d1, double* d2, uint8_t* capped, int64_t* nCap) override {
		std::vector<double> S((size_t) 4 * K * (size_t) L), KJ((size_t) L), E((size_t) 9 * K);
		const double logK = log((double) K);
		*nCap = 0;
		for(int32_t u = 0; u < tp.n; ++u) {
			if(capped) capped[u] = 0;
			if(u == tp.root) { if(tStar) tStar[u] = t[u]; if(f) f[u] = 0; if(d1) d1[u] = 0; if(d2) d2[u] = 0; continue; }
			for(int64_t j = 0; j < L; ++j) {
				for(int32_t c = 0; c < K; ++c) {
					const size_t at = cells4 * (size_t) c + ((size_t) u * (size_t) L + (size_t) j) * 4;
					double r[3], Kc;
					hu_blen_column(m, up.data() + at, down.data() + at, r, &Kc);
					hu_gamma_put(S.data() + j, L, c, r, Kc);
				}
				KJ[(size_t) j] = hu_gamma_close(S.data() + j, L, K);
			}
			auto eval = [&](double x, double* g, double* h) {
				for(int i = 0; i < 3 * K; ++i) hu_gamma_exp1(lr.data(), x, i, E.data());
				double sg = 0, sh = 0;
				for(int64_t j = 0; j < L; ++j) { double a, b; hu_gamma_sums(E.data(), S.data() + j, L, K, &a, &b); sg += a; sh += b; }
				*g = sg; *h = sh;
			};
			double g0, h0;
			eval(t[u], &g0, &h0);
			if(f) { double s = 0; for(int64_t j = 0; j < L; ++j) { double a, b; s += (KJ[(size_t) j] - logK) + log(hu_gamma_sums(E.data(), S.data() + j, L, K, &a, &b)); } f[u] = s; }
			if(d1) d1[u] = g0;
			if(d2) d2[u] = h0;
			if(!tStar) continue;
			int its = 0;
			tStar[u] = hu_blen_solve(t[u], g0, h0, lo, hi, eval, &its);
			if(its > HU_BLEN_MAX_NEWTON) { ++*nCap; if(capped) capped[u] = 1; }
		}
		return HU_OK;
	}
};
}

HuGammaRun* hu_gamma_host_run(const HuBlenTopo& tp, const HuBlenModel& m, int32_t K, int32_t cs_len, const int32_t* parent, const int8_t* seq, double lo, double hi) {
	return new GammaHost(tp, m, K, cs_len, parent, seq, lo, hi);
}

int hu_gamma_fit_run(const char* fn, hu_gamma_opts* o, int32_t n, int32_t root, double* blen, HuGammaRun& run, double* sec) {
	const int32_t K = o->k;
	const bool estimate = o->alpha == 0.0;
	const double tAll = hu_now_s();
	double alpha = estimate ? 1.0 : o->alpha, rate[HU_MAX_DGK], ll = 0, sec3[4] = {0, 0, 0, 0};
	for(int i = 0; i < 5; ++i) sec[i] = 0;
	int rc;
	auto at = [&](double a, double* out) -> int {
		int r;
		if((r = hu_gamma_rates(K, a, rate)) != HU_OK || (r = run.set_rates(rate)) != HU_OK || (r = run.sweep(blen, false)) != HU_OK) return r;
		return run.loglik(nullptr, nullptr, out);
	};
	double t0 = hu_now_s();
	if((rc = at(alpha, &ll)) != HU_OK) return rc;
	sec[3] += hu_now_s() - t0;
	if(!(ll == ll) || ll == -INFINITY) { hu_set_error("%s: the log-likelihood of the start tree is %g: no objective to improve", fn, ll); return HU_ERR_ARG; }
	o->ll_start = o->ll_final = ll; o->n_outer = 0; o->n_capped = 0; o->stop = estimate ? HU_GAMMA_MAX_OUTER : HU_GAMMA_FIXED_ALPHA;
	HuBlenOps ops;
	ops.sweep = [&](const double* b, bool withDown) { return run.sweep(b, withDown); };
	ops.loglik = [&](double* out) { return run.loglik(nullptr, nullptr, out); };
	ops.step = [&](const double* b, double* ts, int64_t* nCap) { return run.step(b, ts, nullptr, nullptr, nullptr, nullptr, nCap); };
	const int32_t passes = estimate ? o->max_outer : 1;
	for(int32_t p = 0; p < passes; ++p) {
		const double llBefore = ll;
		if(estimate) {
			/* golden section on x = log alpha, a fixed number of evaluations; the best point evaluated is taken if it beats the alpha held */
			t0 = hu_now_s();
			const double invphi = 0.5 * (sqrt(5.0) - 1.0);
			double a = log(HU_GAMMA_ALPHA_MIN), b = log(HU_GAMMA_ALPHA_MAX), x1 = b - invphi * (b - a), x2 = a + invphi * (b - a), f1 = 0, f2 = 0;
			auto F = [&](double x, double* out) { return at(std::min(std::max(exp(x), HU_GAMMA_ALPHA_MIN), HU_GAMMA_ALPHA_MAX), out); };
			if((rc = F(x1, &f1)) != HU_OK || (rc = F(x2, &f2)) != HU_OK) return rc;
			double bx = f1 > f2 ? x1 : x2, bf = f1 > f2 ? f1 : f2;
			for(int e = 2; e < HU_GAMMA_SHAPE_EVALS; ++e) {
				if(f1 > f2) { b = x2; x2 = x1; f2 = f1; x1 = b - invphi * (b - a); if((rc = F(x1, &f1)) != HU_OK) return rc; if(f1 > bf) { bf = f1; bx = x1; } }
				else { a = x1; x1 = x2; f1 = f2; x2 = a + invphi * (b - a); if((rc = F(x2, &f2)) != HU_OK) return rc; if(f2 > bf) { bf = f2; bx = x2; } }
			}
			if(bf > ll) { alpha = std::min(std::max(exp(bx), HU_GAMMA_ALPHA_MIN), HU_GAMMA_ALPHA_MAX); ll = bf; }
			sec[0] += hu_now_s() - t0;
		}
		if((rc = hu_gamma_rates(K, alpha, rate)) != HU_OK || (rc = run.set_rates(rate)) != HU_OK) return rc;
		hu_blen_opts bo = hu_search_fit_opts(o->blen);
		if((rc = hu_blen_rounds(fn, &bo, n, root, blen, ops, sec3)) != HU_OK) return rc;
		ll = bo.ll_final;                                        /* the rounds start from the same sweep and column sum, so it is at least ll */
		if(o->passes && o->n_outer < o->passes_cap) { hu_gamma_pass& P = o->passes[o->n_outer]; P.alpha = alpha; P.ll = ll; P.n_rounds = bo.n_rounds; P.reserved = 0; }
		o->n_outer++; o->n_capped += bo.n_capped; o->ll_final = ll;
		if(estimate && ll - llBefore < o->eps_ll) { o->stop = HU_GAMMA_CONVERGED; break; }
	}
	o->alpha_fit = alpha;
	for(int c = 0; c < HU_MAX_DGK; ++c) o->rates[c] = c < K ? rate[c] : 0.0;
	sec[1] = sec3[0]; sec[2] = sec3[1]; sec[3] += sec3[2];
	sec[4] = hu_now_s() - tAll - sec[0] - sec[1] - sec[2] - sec[3];
	return HU_OK;
}
