// What the host half (hu_nni_host.cpp, a plain C++ compiler) and the device half (hu_nni.cpp, hu_kern_nni.h) of the NNI search share
// (DESIGN.md §23): the record of an eligible edge, the entries of the four P(t) of an edge and the arithmetic of one column, which
// leaves the nine ratios and the three constants of the edge's three arrangements.  The model, the denominators, the terms of f' and
// f'' and the safeguarded Newton are hu_tree_blen.h's, unchanged.  Both translation units are built with -ffp-contract=off.
#pragma once
#include "hu_tree_blen.h"

#define HU_NNI_WG HU_BLEN_WG     /* threads of a workgroup of k_nni_score: column j belongs to thread j % HU_NNI_WG */

/* the three rooted cases of an eligible edge */
enum { HU_NNI_INNER = 0,         /* p = parent[u] is not the root and has the children {u, C}: d comes from down[p] over blen[p] */
       HU_NNI_ROOT3 = 1,         /* p is the root with the children {u, C, D}: c and d both come from up */
       HU_NNI_ROOT2 = 2 };       /* p is a bifurcating root {u, s}: blen[u] + blen[s] is the edge, C and D are the children of s */

/* an eligible edge.  A < B are the children of u, in node-id order; C (and D, where it is a node: C < D) hang at the other end v.
 * msg[k] is the message of subtree k before its own branch: node x for up[x], n + x for down[x]; len[k] the branch it is carried over. */
struct HuNniEdge {
	int32_t u, v, kind, A, B, C, D, pad0;    /* v: the other end, p or s; D = -1 for HU_NNI_INNER */
	int32_t msg[4]; double len[4];
	double t0;                                 /* the central length: blen[u], or blen[u] + blen[s] */
};

/* entry (row, col) of P(t) = U diag(exp(lam t)) U1; the identity at t = 0 and never below 0, as the sweeps carry a message */
HU_BLEN_HD double hu_nni_pentry(const HuBlenModel& m, double t, int row, int col) {
	if(t == 0) return row == col ? 1.0 : 0.0;
	const double s = (m.U[row * 4 + 0] * m.U1[0 * 4 + col] + m.U[row * 4 + 1] * exp(m.lam[1] * t) * m.U1[1 * 4 + col])
		+ (m.U[row * 4 + 2] * exp(m.lam[2] * t) * m.U1[2 * 4 + col] + m.U[row * 4 + 3] * exp(m.lam[3] * t) * m.U1[3 * 4 + col]);
	return fmax(s, 0.0);
}

/* a message carried over its branch in linear space: v = P . exp(M - max M); returns max M, -inf for a message without a finite entry */
HU_BLEN_HD double hu_nni_carry(const double* P, const double* M, double* v) {
	const double mx = hu_blen_max4(M);
	if(!(mx > -INFINITY)) { v[0] = v[1] = v[2] = v[3] = 0.0; return -INFINITY; }
	double x[4];
	for(int a = 0; a < 4; ++a) x[a] = exp(M[a] - mx);
	for(int i = 0; i < 4; ++i) v[i] = (P[i * 4 + 0] * x[0] + P[i * 4 + 1] * x[1]) + (P[i * 4 + 2] * x[2] + P[i * 4 + 3] * x[3]);
	return mx;
}

/* one arrangement (x | y) of one column: r[3] = c_k / c_0 and K = log c_0 + S.  c_0 = (pi . x)(pi . y) = 0, which two subtrees that
 * share no base at a branch of length 0 give, is a column of likelihood 0: r = 0 and K = -inf, as a message without a finite entry */
HU_BLEN_HD void hu_nni_pair(const HuBlenModel& m, const double* x, const double* y, double S, double* r, double* K) {
	double c[4];
	for(int k = 0; k < 4; ++k) {
		const double p = (m.A[k * 4 + 0] * x[0] + m.A[k * 4 + 1] * x[1]) + (m.A[k * 4 + 2] * x[2] + m.A[k * 4 + 3] * x[3]);
		const double q = (m.U1[k * 4 + 0] * y[0] + m.U1[k * 4 + 1] * y[1]) + (m.U1[k * 4 + 2] * y[2] + m.U1[k * 4 + 3] * y[3]);
		c[k] = p * q;
	}
	if(!(c[0] > 0) || !(S > -INFINITY)) { r[0] = r[1] = r[2] = 0.0; *K = -INFINITY; return; }
	r[0] = c[1] / c[0]; r[1] = c[2] / c[0]; r[2] = c[3] / c[0];
	*K = log(c[0]) + S;
}

/* one column of one edge: P [4][16] of the four branches, M [4][4] the four messages in log space; r [3][3] and K [3] of the
 * arrangements 0: (a.b | c.d), 1: (a.c | b.d), 2: (b.c | a.d) */
HU_BLEN_HD void hu_nni_column(const HuBlenModel& m, const double* P, const double* M, double* r, double* K) {
	double a[4], b[4], c[4], d[4], x[4], y[4];
	const double S = ((hu_nni_carry(P, M, a) + hu_nni_carry(P + 16, M + 4, b)) + hu_nni_carry(P + 32, M + 8, c)) + hu_nni_carry(P + 48, M + 12, d);
	for(int i = 0; i < 4; ++i) { x[i] = a[i] * b[i]; y[i] = c[i] * d[i]; }
	hu_nni_pair(m, x, y, S, r, K);
	for(int i = 0; i < 4; ++i) { x[i] = a[i] * c[i]; y[i] = b[i] * d[i]; }
	hu_nni_pair(m, x, y, S, r + 3, K + 1);
	for(int i = 0; i < 4; ++i) { x[i] = b[i] * c[i]; y[i] = a[i] * d[i]; }
	hu_nni_pair(m, x, y, S, r + 6, K + 2);
}

/* ---- the host half, hu_nni_host.cpp ---- */
/* the eligible edges of a tree in ascending u, and the number of edges between two inner nodes that a polytomy rules out */
void hu_nni_edges(const HuBlenTopo& tp, const int32_t* parent, const double* blen, std::vector<HuNniEdge>* edges, int64_t* skipped);
/* t_star [E][3], f [E][3], f0 [E] of the edges from the messages up, down [n][L][4]; returns the Newton loops at the cap */
int64_t hu_nni_host_score(const HuBlenModel& m, int32_t n, int64_t L, const std::vector<HuNniEdge>& edges, const double* up, const double* down,
		double lo, double hi, double* t_star, double* f, double* f0);
/* the swap of arrangement q (1 or 2) on the arrays, the central edge at t; child_idx may be NULL */
void hu_nni_apply_edge(const HuNniEdge& e, int q, double t, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx);
/* the candidates (gain > min_gain) ordered by gain descending, ties by the smaller u, and those of them taken greedily: no end node
 * shared with one taken before.  gain [E]; order and taken hold indices into the edges */
void hu_nni_select(const std::vector<HuNniEdge>& edges, const double* gain, double min_gain, std::vector<int32_t>* order, std::vector<int32_t>* taken);
/* the set tried after a rejected one: its better half, rounded up; false when a single swap was rejected */
bool hu_nni_halve(std::vector<int32_t>* taken);
/* the checks of the entries (hu_blen_check's and the NNI options'), with the need held against the budget */
int hu_nni_check(const char* fn, const hu_nni_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp);
/* the round loop over either half.  fit(parent, blen, &ll): hu_tree_optimize_lengths in place; score(parent, blen, edges, t_star, f, f0);
 * trial(parent, blen, &ll): one up sweep and hu_tree_loglik */
struct HuNniOps {
	std::function<int(const int32_t*, double*, double*)> fit;
	std::function<int(const int32_t*, const double*, const std::vector<HuNniEdge>&, double*, double*, double*)> score;
	std::function<int(const int32_t*, const double*, double*)> trial;
};
int hu_nni_rounds(const char* fn, hu_nni_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq, const int32_t* child_off,
		int32_t* child_idx, const HuNniOps& ops, double* seconds);
/* the two entries on the host path */
int hu_nni_host_scores_entry(const char* fn, const hu_nni_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, double* f0);
int hu_nni_host_search_entry(const char* fn, hu_nni_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuBlenModel& m, double* seconds);
