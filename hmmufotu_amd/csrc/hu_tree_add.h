// What the host half (hu_add_host.cpp, a plain C++ compiler) and the device half (hu_add.cpp, hu_kern_add.h) of the insertion of new
// sequences share: the table of the query's side, the arithmetic of one column of an edge, which leaves the edge's
// three ratios and its constant, and the rule of the best edge.  The model, the denominators, the terms of f' and f'' and the
// safeguarded Newton are hu_tree_blen.h's, P(t) and the carried message hu_tree_nni.h's, unchanged.  Both translation units are built
// with -ffp-contract=off.
#pragma once
#include "hu_tree_nni.h"

#define HU_ADD_WG HU_BLEN_WG     /* threads of a workgroup of k_add_score: column j belongs to thread j % HU_ADD_WG */
#define HU_ADD_TAB 20            /* tau [3][5], then kappa [5] */

/* the symbol of a query's column: its base, or 4 where it has none */
HU_BLEN_HD int hu_add_sym(int8_t c) { return c >= 0 ? (int) c : 4; }

/* the query's side of c_jk = A_jk T[k][s]: with y the leaf message of the symbol s (one-hot; exp(log pi - max log pi) for none) and
 * T[k][s] = sum_b U1_kb y_b, entry i < 15 is tau[k][s] = T[k + 1][s] / T[0][s] at i = 5 k + s, entry 15 + s is kappa[s] = log T[0][s]
 * + max y: what the symbol adds to K_j.  T[0][s] > 0 for every s, as pi > 0 */
HU_BLEN_HD double hu_add_tab_entry(const HuBlenModel& m, int i) {
	const int s = i % 5, k = i < 15 ? i / 5 + 1 : 0;
	double y[4], my = 0.0;
	if(s < 4) for(int b = 0; b < 4; ++b) y[b] = b == s ? 1.0 : 0.0;
	else { my = hu_blen_max4(m.logpi); for(int b = 0; b < 4; ++b) y[b] = exp(m.logpi[b] - my); }
	const double T0 = (m.U1[0] * y[0] + m.U1[1] * y[1]) + (m.U1[2] * y[2] + m.U1[3] * y[3]);
	if(i >= 15) return log(T0) + my;
	return ((m.U1[k * 4 + 0] * y[0] + m.U1[k * 4 + 1] * y[1]) + (m.U1[k * 4 + 2] * y[2] + m.U1[k * 4 + 3] * y[3])) / T0;
}

/* one column of one edge w: Mu = up[w] and Md = down[w] in log space, both carried by P = P(blen[w] / 2) to the junction x;
 * rho[3] = A_k / A_0 with A_k = sum_a pi_a x_a U_ak, and K = log A_0 + the two maxima.  A junction of likelihood 0 (two sides that
 * share no base over lengths of 0, or a message without a finite entry) gives rho = 0 and K = -inf, as hu_nni_pair has it */
HU_BLEN_HD void hu_add_edge_column(const HuBlenModel& m, const double* P, const double* Mu, const double* Md, double* rho, double* K) {
	double a[4], b[4], x[4], A[4];
	const double sa = hu_nni_carry(P, Mu, a), sb = hu_nni_carry(P, Md, b), S = sa + sb;
	for(int i = 0; i < 4; ++i) x[i] = a[i] * b[i];
	for(int k = 0; k < 4; ++k) A[k] = (m.A[k * 4 + 0] * x[0] + m.A[k * 4 + 1] * x[1]) + (m.A[k * 4 + 2] * x[2] + m.A[k * 4 + 3] * x[3]);
	if(!(A[0] > 0) || !(S > -INFINITY)) { rho[0] = rho[1] = rho[2] = 0.0; *K = -INFINITY; return; }
	rho[0] = A[1] / A[0]; rho[1] = A[2] / A[0]; rho[2] = A[3] / A[0];
	*K = log(A[0]) + S;
}

/* the ratios of a (edge, query) column: the edge's times the symbol's */
HU_BLEN_HD void hu_add_ratio(const double* tab, int s, double r0, double r1, double r2, double* r) {
	r[0] = r0 * tab[s]; r[1] = r1 * tab[5 + s]; r[2] = r2 * tab[10 + s];
}

/* whether the edge w with the value f replaces the best so far (bw < 0: none yet): the larger f, the smaller w among equals */
HU_BLEN_HD bool hu_add_better(double f, int32_t w, double bf, int32_t bw) { return bw < 0 || f > bf || (f == bf && w < bw); }

/* the start of every pendant: the mean length of the non-root branches, summed in ascending node, clipped to [lo, hi] */
inline double hu_add_start(int32_t n, const int32_t* parent, const double* blen, double lo, double hi) {
	double s = 0;
	for(int32_t i = 0; i < n; ++i) if(parent[i] >= 0) s += blen[i];
	return fmin(fmax(n > 1 ? s / (double)(n - 1) : lo, lo), hi);
}

/* the queries of a tile and the bytes a tile of a launch holds: the outputs, the rows and the records of its queries and, above
 * HU_BLEN_LDS_COLS columns, the ratios of its n workgroups */
inline int32_t hu_add_tile(const hu_add_opts* o) { return o->tile > 0 ? o->tile : HU_ADD_TILE; }
inline int64_t hu_add_tile_bytes(int32_t n, int32_t cs_len, int32_t tile) {
	return (int64_t) tile * (16 * (int64_t) n + cs_len + 24) + (cs_len > HU_BLEN_LDS_COLS ? 24 * (int64_t) cs_len * n : 0);
}
/* the queries a launch takes at the most: whole tiles within HU_ADD_SLAB_BYTES, one tile at the least, opts->slab at the most */
inline int64_t hu_add_slab_queries(const hu_add_opts* o, int32_t n, int32_t cs_len) {
	const int32_t tile = hu_add_tile(o);
	const int64_t fit = std::min<int64_t>(std::max<int64_t>(HU_ADD_SLAB_BYTES / hu_add_tile_bytes(n, cs_len, tile), 1), 65535) * tile;
	return o->slab > 0 ? std::min<int64_t>(o->slab, fit) : fit;
}

/* ---- the host half, hu_add_host.cpp ---- */
/* t_star, f [nq][n] of every (query, edge) from the messages up, down [n][L][4]; the root's entries are 0 and -inf */
void hu_add_host_score(const HuBlenModel& m, int32_t n, int64_t L, int32_t root, const double* blen, const double* up, const double* down,
		double lo, double hi, double t0, int32_t nq, const int8_t* qseq, double* t_star, double* f);
/* the best edge of every query from t_star, f [nq][n] */
void hu_add_host_best(int32_t n, int32_t root, int32_t nq, const double* t_star, const double* f, int32_t* best_w, double* best_t, double* best_f);
/* the insertion on the arrays, checked: HU_OK or HU_ERR_ARG with the message set */
int hu_add_apply(const char* fn, int32_t n, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx, int32_t w, double t, double lo, double hi);
/* the checks of the entries: hu_blen_check's, the options', the queries' codes, and the need held against the budget: of the tree as it
 * stands, or with grows of the tree after every query went in */
int hu_add_check(const char* fn, const hu_add_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t n_query, const int8_t* qseq, bool grows, int32_t dg_k, HuBlenTopo* tp);
/* the round loop over either half.  fit(n, parent, blen, seq, &ll): hu_tree_optimize_lengths in place; sweep(n, parent, blen, seq, tp):
 * the messages of the tree as it stands; score(n, root, blen, t0, nq, rows, best_w, best_t, best_f): the best edge of every query
 * from those messages */
struct HuAddOps {
	std::function<int(int32_t, const int32_t*, double*, const int8_t*, double*)> fit;
	std::function<int(int32_t, const int32_t*, const double*, const int8_t*, const HuBlenTopo&)> sweep;
	std::function<int(int32_t, int32_t, const double*, double, int32_t, const int8_t*, int32_t*, double*, double*)> score;
};
int hu_add_rounds(const char* fn, hu_add_opts* o, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const HuAddOps& ops, double* seconds);
/* the two entries on the host path */
int hu_add_host_scores_entry(const char* fn, const hu_add_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t n_query, const int8_t* qseq, double* t_star, double* f, int32_t* best_w, double* best_t, double* best_f);
int hu_add_host_search_entry(const char* fn, hu_add_opts* o, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const HuBlenModel& m, double* seconds);
