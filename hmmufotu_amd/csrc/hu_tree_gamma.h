// What the host half (hu_gamma_host.cpp, a plain C++ compiler) and the device half (hu_gamma.cpp, hu_kern_gamma.h) of the fit under
// the discrete Gamma of rates share: the arithmetic of one column over the K categories, on top of hu_tree_blen.h's
// arithmetic of one category.  Every function here is compiled for both sides from this one text, and both translation units are
// built with -ffp-contract=off.  Below it the host half: the checks, the two halves behind one interface, and the entries over it.
#pragma once
#include "hu_tree_blen.h"

#ifndef HU_MAX_DGK
#define HU_MAX_DGK 16            /* hu_common.h's, which the host half cannot include: the rates of a hu_model_desc and of a hu_gamma_opts */
#endif

/* the values a branch keeps of column j, 4 K doubles at s[(4 c + i) * ld]: i = 0: w_jc, i = 1..3: w_jc r_jcm.  Pass 1 puts K_jc and
 * r_jcm of every category there (hu_gamma_put) and then turns them into the weights (hu_gamma_close), which returns K_j = max_c K_jc;
 * a column whose every K_jc is -inf keeps weights of 0 and returns -inf */
HU_BLEN_HD void hu_gamma_put(double* s, int64_t ld, int c, const double* r, double Kc) {
	s[(4 * c) * ld] = Kc; s[(4 * c + 1) * ld] = r[0]; s[(4 * c + 2) * ld] = r[1]; s[(4 * c + 3) * ld] = r[2];
}
HU_BLEN_HD double hu_gamma_close(double* s, int64_t ld, int K) {
	double Kj = -INFINITY;
	for(int c = 0; c < K; ++c) Kj = fmax(Kj, s[(4 * c) * ld]);
	for(int c = 0; c < K; ++c) {
		const double w = Kj > -INFINITY ? exp(s[(4 * c) * ld] - Kj) : 0.0;
		s[(4 * c) * ld] = w;
		for(int i = 1; i < 4; ++i) s[(4 * c + i) * ld] = w * s[(4 * c + i) * ld];
	}
	return Kj;
}

/* what a branch needs of t, 9 K doubles: E[9 c + m] = e_cm = exp(l_cm t), E[9 c + 3 + m] = l_cm e_cm, E[9 c + 6 + m] = l_cm^2 e_cm with
 * l_cm = lam_m rate_c (lr [3 K], hu_gamma_lr): three exp per category and evaluation */
HU_BLEN_HD void hu_gamma_lr(const HuBlenModel& m, int K, const double* rate, double* lr) {
	for(int c = 0; c < K; ++c) for(int k = 0; k < 3; ++k) lr[3 * c + k] = m.lam[k + 1] * rate[c];
}
HU_BLEN_HD void hu_gamma_exp1(const double* lr, double t, int i, double* E) {
	const int c = i / 3, k = i - 3 * c;
	const double l = lr[i], e = exp(l * t);
	E[9 * c + k] = e; E[9 * c + 3 + k] = l * e; E[9 * c + 6 + k] = l * (l * e);
}
/* S_j (kept off zero as hu_blen_den keeps D_j), and the column's terms of f' and f'' */
HU_BLEN_HD double hu_gamma_sums(const double* E, const double* s, int64_t ld, int K, double* g, double* h) {
	double S = 0.0, N = 0.0, M = 0.0;
	for(int c = 0; c < K; ++c) {
		const double* e = E + 9 * c;
		const double w = s[(4 * c) * ld], a0 = s[(4 * c + 1) * ld], a1 = s[(4 * c + 2) * ld], a2 = s[(4 * c + 3) * ld];
		S += w + ((a0 * e[0] + a1 * e[1]) + a2 * e[2]);
		N += (a0 * e[3] + a1 * e[4]) + a2 * e[5];
		M += (a0 * e[6] + a1 * e[7]) + a2 * e[8];
	}
	if(!(S > DBL_MIN)) S = DBL_MIN;
	const double a = N / S;
	*g = a; *h = M / S - a * a;
	return S;
}
/* the mean of exp(v_c) over the categories, in log space above the largest: a column's log-likelihood from its categories' */
HU_BLEN_HD double hu_gamma_logmean(const double* v, int64_t ld, int K) {
	double mx = -INFINITY, s = 0.0;
	for(int c = 0; c < K; ++c) mx = fmax(mx, v[c * ld]);
	if(!(mx > -INFINITY)) return -INFINITY;
	for(int c = 0; c < K; ++c) s += exp(v[c * ld] - mx);
	return mx + log(s / K);
}

/* whether the 4 K values of a branch's columns stay in LDS, and the bytes of a workgroup then: the reduction scratch, E, the values */
inline size_t hu_gamma_lds_bytes(int32_t K, int64_t L) { return ((size_t) 3 * HU_BLEN_WG + (size_t)(9 * K + (9 * K & 1)) + (size_t) 4 * K * (size_t) L) * 8; }
inline bool hu_gamma_in_lds(int32_t K, int64_t L) { return hu_gamma_lds_bytes(K, L) <= HU_GAMMA_LDS_BYTES; }
/* the branches of one launch of the step beyond LDS */
inline int64_t hu_gamma_slab(int32_t n) { const int64_t s = n / 32 > HU_GAMMA_SLAB_MIN ? n / 32 : HU_GAMMA_SLAB_MIN; return s < n ? s : n; }

/* ---- the host half, hu_gamma_host.cpp ---- */
/* the arguments of the entries, checked, the need held against the budget; fills topo */
int hu_gamma_check(const char* fn, const hu_gamma_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* topo);
/* either half behind the operations of the entries.  The messages are those of the last sweep, under the rates last set */
struct HuGammaRun {
	virtual ~HuGammaRun() {}
	virtual int set_rates(const double* rate) = 0;                       /* [K] */
	virtual int sweep(const double* blen, bool withDown) = 0;
	/* per_col [L], per_cat [K][L] (either may be NULL), *ll */
	virtual int loglik(double* per_col, double* per_cat, double* ll) = 0;
	/* scores at t, and with tStar the step; *nCap: the branches at the Newton cap */
	virtual int step(const double* t, double* tStar, double* f, double* d1, double* d2, uint8_t* capped, int64_t* nCap) = 0;
};
/* the host path; the arrays outlive it */
HuGammaRun* hu_gamma_host_run(const HuBlenTopo& tp, const HuBlenModel& m, int32_t K, int32_t cs_len, const int32_t* parent, const int8_t* seq, double lo, double hi);
/* hu_tree_gamma_fit over either half; seconds [5] as hu_gamma_timing */
int hu_gamma_fit_run(const char* fn, hu_gamma_opts* o, int32_t n, int32_t root, double* blen, HuGammaRun& run, double* seconds);
