// What the host half (hu_blen_host.cpp, a plain C++ compiler) and the device half (hu_blen.cpp, hu_kern_blen.h) of the branch-length
// fit share: the model in the form the step reads, the arithmetic of one column and the rule of one Newton step.
// Every function here is compiled for both sides from this one text, and both translation units are built with -ffp-contract=off.
// Below the fit's own host half: what the searches over topologies (§23, §25, §26) share on the host path, their round loop included.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <chrono>
#include <functional>
#include <vector>
#include "../../include/hmmufotu_amd.h"

#if defined(__HIPCC__)
#define HU_BLEN_HD __host__ __device__ inline
#else
#define HU_BLEN_HD inline
#endif

#define HU_BLEN_WG 256           /* threads of a workgroup of k_blen_step: column j belongs to thread j % HU_BLEN_WG */
#define HU_BLEN_MIN_LOGLIK_EXP (-510.0)   /* the scaling rule of the messages, src/PhyloTreeUnrooted.cpp:68 */

/* P(t) = U diag(exp(lam t)) U1 with lam[0] = 0, U[.][0] = 1, U1[0][.] = pi (hu_model_spectral), and A[k][a] = pi_a U[a][k] */
struct HuBlenModel { double pi[4], logpi[4], U[16], U1[16], lam[4], A[16]; };

HU_BLEN_HD void hu_blen_model_set(HuBlenModel* m, const double* U, const double* lam, const double* U1) {
	for(int i = 0; i < 16; ++i) { m->U[i] = U[i]; m->U1[i] = U1[i]; }
	for(int k = 0; k < 4; ++k) { m->lam[k] = lam[k]; m->pi[k] = U1[k]; m->logpi[k] = log(U1[k]); }
	for(int k = 0; k < 4; ++k) for(int a = 0; a < 4; ++a) m->A[k * 4 + a] = U1[a] * U[a * 4 + k];
}

HU_BLEN_HD double hu_blen_max4(const double* v) { return fmax(fmax(v[0], v[1]), fmax(v[2], v[3])); }

/* one column of one branch: r[3] = c_k / c_0 (k = 1..3) and K = log c_0 + max up + max down, from the two messages in log space.
 * A message without a finite entry (a column whose likelihood underflowed) gives r = 0 and K = -inf. */
HU_BLEN_HD void hu_blen_column(const HuBlenModel& m, const double* Mu, const double* Md, double* r, double* K) {
	const double mx = hu_blen_max4(Mu), my = hu_blen_max4(Md);
	if(!(mx > -INFINITY) || !(my > -INFINITY)) { r[0] = r[1] = r[2] = 0.0; *K = -INFINITY; return; }
	double x[4], y[4], c[4];
	for(int a = 0; a < 4; ++a) { x[a] = exp(Mu[a] - mx); y[a] = exp(Md[a] - my); }
	for(int k = 0; k < 4; ++k) {
		const double p = (m.A[k * 4 + 0] * x[0] + m.A[k * 4 + 1] * x[1]) + (m.A[k * 4 + 2] * x[2] + m.A[k * 4 + 3] * x[3]);
		const double q = (m.U1[k * 4 + 0] * y[0] + m.U1[k * 4 + 1] * y[1]) + (m.U1[k * 4 + 2] * y[2] + m.U1[k * 4 + 3] * y[3]);
		c[k] = p * q;
	}
	r[0] = c[1] / c[0]; r[1] = c[2] / c[0]; r[2] = c[3] / c[0];
	*K = (log(c[0]) + mx) + my;
}

/* what a branch needs of t: e_k = exp(lam_k t), lam_k e_k and lam_k^2 e_k for k = 1..3: three exp per branch and evaluation */
struct HuBlenExp { double e[3], le[3], l2e[3]; };
HU_BLEN_HD void hu_blen_exp(const HuBlenModel& m, double t, HuBlenExp* E) {
	for(int k = 0; k < 3; ++k) { const double l = m.lam[k + 1]; E->e[k] = exp(l * t); E->le[k] = l * E->e[k]; E->l2e[k] = l * E->le[k]; }
}
/* D_j = L_j(t) / c_j0, kept off zero: at t = 0 a column whose two sides share no base has L = 0 in exact arithmetic and a positive L' */
HU_BLEN_HD double hu_blen_den(const HuBlenExp& E, const double* r) {
	const double d = 1.0 + ((r[0] * E.e[0] + r[1] * E.e[1]) + r[2] * E.e[2]);
	return d > DBL_MIN ? d : DBL_MIN;
}
/* the column's terms of f' and f'' */
HU_BLEN_HD void hu_blen_terms(const HuBlenExp& E, const double* r, double* g, double* h) {
	const double d = hu_blen_den(E, r);
	const double a = ((r[0] * E.le[0] + r[1] * E.le[1]) + r[2] * E.le[2]) / d;
	const double b = ((r[0] * E.l2e[0] + r[1] * E.l2e[1]) + r[2] * E.l2e[2]) / d;
	*g = a; *h = b - a * a;
}

/* one safeguarded Newton step on f' inside the bracket (lo, hi), f'(lo) > 0 > f'(hi): the bracket takes t by the sign of g, the next t
 * is Newton's when f'' < 0 and it falls inside the bracket, the middle of the bracket otherwise.  Returns the next t; *done when the
 * step is at most HU_BLEN_TAU or g is 0. */
HU_BLEN_HD double hu_blen_newton(double t, double g, double h, double* lo, double* hi, int* done) {
	if(g == 0.0) { *done = 1; return t; }
	if(g > 0) *lo = t; else *hi = t;
	double tn = 0.5 * (*lo + *hi);
	if(h < 0) { const double c = t - g / h; if(c > *lo && c < *hi) tn = c; }
	*done = fabs(tn - t) <= HU_BLEN_TAU;
	return tn;
}

/* the step of one branch from its start t0, where f' and f'' are g0 and h0 already: the ends first (f'(lo) <= 0 gives lo, f'(hi) >= 0 gives
 * hi), then hu_blen_newton from t0 clamped into [lo, hi] until it is done, HU_BLEN_MAX_NEWTON evaluations at the most.  eval(x, &g, &h)
 * gives f'(x) and f''(x).  *its: the evaluations of the loop, HU_BLEN_MAX_NEWTON + 1 when the cap was hit. */
template<class Eval> HU_BLEN_HD double hu_blen_solve(double t0, double g0, double h0, double lo, double hi, const Eval& eval, int* its) {
	double g, h;
	*its = 0;
	eval(lo, &g, &h);
	if(g <= 0) return lo;
	eval(hi, &g, &h);
	if(g >= 0) return hi;
	double x = fmin(fmax(t0, lo), hi);
	int done = 0, it = 0;
	for(; it < HU_BLEN_MAX_NEWTON && !done; ++it) {
		if(x == t0) { g = g0; h = h0; } else eval(x, &g, &h);
		x = hu_blen_newton(x, g, h, &lo, &hi, &done);
	}
	*its = done ? it : HU_BLEN_MAX_NEWTON + 1;
	return x;
}

/* ---- the host half, hu_blen_host.cpp ---- */
/* the tree as the sweeps read it: children in node-id order and the nodes in breadth-first order from the root */
struct HuBlenTopo {
	int32_t n = 0, root = -1;
	std::vector<int32_t> childOff, childIdx, order;
};
/* the arguments of the three entries, checked: HU_OK, or HU_ERR_ARG / HU_ERR_NOMEM with the message set; fills topo */
int hu_blen_check(const char* fn, const hu_blen_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* topo);
/* up, down [n][cs_len][4] in log space with the reference's scaling rule; down == NULL: the up sweep alone */
void hu_blen_host_sweep(const HuBlenTopo& tp, const HuBlenModel& m, const int32_t* parent, int64_t cs_len, const double* blen, const int8_t* seq,
		double* up, double* down);
/* dot_product_scaled(pi, M) of one column of the root message */
static inline double hu_blen_host_loglik_column(const HuBlenModel& m, const double* M) {
	const double mx = hu_blen_max4(M);
	const double s = (mx != -INFINITY && mx < HU_BLEN_MIN_LOGLIK_EXP) ? HU_BLEN_MIN_LOGLIK_EXP - mx : 0.0;
	double d = 0;
	for(int i = 0; i < 4; ++i) d += m.pi[i] * exp(M[i] + s);
	return log(d) - s;
}
/* treeLoglik: the serial sum over the columns of dot_product_scaled(pi, up[root]) */
double hu_blen_host_loglik(const HuBlenModel& m, int64_t cs_len, const double* up_root);
/* scores at t[u] and, with t_star, the step of every non-root branch; returns the branches at the Newton cap */
int64_t hu_blen_host_step(const HuBlenTopo& tp, const HuBlenModel& m, int64_t cs_len, const double* t, const double* up, const double* down,
		double lo, double hi, double* t_star, double* f, double* d1, double* d2, uint8_t* capped);
/* the round loop over either half.  sweep(blen, withDown), loglik() of the last sweep, step(blen, t_star) -> branches at the cap */
struct HuBlenOps {
	std::function<int(const double*, bool)> sweep;
	std::function<int(double*)> loglik;
	std::function<int(const double*, double*, int64_t*)> step;
};
int hu_blen_rounds(const char* fn, hu_blen_opts* o, int32_t n, int32_t root, double* blen, const HuBlenOps& ops, double* seconds);
void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;
/* the clock of every phase time of the tree family */
inline double hu_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* ---- what the searches over topologies (NNI, SPR, insertion) share on the host path ---- */
/* the messages of a tree of up to nCap nodes, and the two operations of a search's round that need no scores */
struct HuBlenHost {
	const HuBlenModel& m; int64_t L; double lo, hi;
	std::vector<double> up, down;
	HuBlenHost(const HuBlenModel& model, int64_t nCap, int64_t cs_len, const hu_blen_opts& bo)
		: m(model), L(cs_len), lo(bo.min_len), hi(bo.max_len), up((size_t)(nCap * cs_len * 4)), down((size_t)(nCap * cs_len * 4)) {}
	void sweep(const HuBlenTopo& tp, const int32_t* parent, const double* blen, const int8_t* seq, bool withDown) {
		hu_blen_host_sweep(tp, m, parent, L, blen, seq, up.data(), withDown ? down.data() : nullptr);
	}
	/* hu_blen_rounds in place under bo, without its round records; ll: the log-likelihood it ends at */
	int fit(const char* fn, const hu_blen_opts* bo, int32_t n, const int32_t* parent, double* blen, const int8_t* seq, double* ll);
	/* one up sweep and the log-likelihood */
	int trial(const char* fn, const hu_blen_opts* bo, int32_t n, const int32_t* parent, const double* blen, const int8_t* seq, double* ll);
};
/* the options of a search's fit: the search's own hu_blen_opts without the round records.  The budget is not the fit's to hold: every
 * search has held it against its own need, which includes hu_blen_need of the largest tree it fits (hu_nni_check, hu_spr_check,
 * hu_add_check), so the fit's check of it could never fire */
inline hu_blen_opts hu_search_fit_opts(const hu_blen_opts& o) { hu_blen_opts bo = o; bo.rounds = nullptr; bo.rounds_cap = 0; bo.mem_budget = 0; return bo; }

/* the set tried after a rejected one: its better half, rounded up; false when a single move was rejected */
bool hu_nni_halve(std::vector<int32_t>* taken);
/* the round loop of the NNI and the SPR search over either half: fit, stop after the last fit allowed, score, select, try the taken set and
 * halve it until the log-likelihood rises, commit, record.
 *   fit(parent, blen, &ll): hu_tree_optimize_lengths in place;  trial(parent, blen, &ll): one up sweep and hu_tree_loglik
 *   score(tp): scores the tree as it stands;  select(tp, &taken): the indices of the moves to try, the best first; none: a local optimum
 *   apply(taken, parent, blen, child_idx): the moves on copies of the arrays (child_idx NULL without an order of children)
 *   record(round, ll, nTaken, taken): the accepted round and its moves, round counted from 1; nTaken: the set before any halving
 * stop: one of HU_SEARCH_*, which HU_NNI_* and HU_SPR_* both equal.  seconds [0..2] += fit, score (with the check of the tree), trials;
 * the selection is timed in none of them */
enum { HU_SEARCH_LOCAL_OPTIMUM = HU_NNI_LOCAL_OPTIMUM, HU_SEARCH_NO_MOVE = HU_NNI_NO_SWAP, HU_SEARCH_MAX_ROUNDS = HU_NNI_MAX_ROUNDS };
static_assert((int) HU_SPR_LOCAL_OPTIMUM == (int) HU_SEARCH_LOCAL_OPTIMUM && (int) HU_SPR_NO_MOVE == (int) HU_SEARCH_NO_MOVE &&
	(int) HU_SPR_MAX_ROUNDS == (int) HU_SEARCH_MAX_ROUNDS, "the SPR search reports hu_search_rounds' stop as its own");
struct HuSearchOps {
	std::function<int(const int32_t*, double*, double*)> fit;
	std::function<int(const int32_t*, const double*, double*)> trial;
	std::function<int(const HuBlenTopo&)> score;
	std::function<void(const HuBlenTopo&, std::vector<int32_t>*)> select;
	std::function<int(const std::vector<int32_t>&, int32_t*, double*, int32_t*)> apply;
	std::function<void(int32_t, double, size_t, const std::vector<int32_t>&)> record;
};
int hu_search_rounds(const char* fn, const hu_blen_opts* bo, int32_t rounds, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuSearchOps& ops, double* ll_start, double* ll_final, int32_t* stop, double* seconds);
