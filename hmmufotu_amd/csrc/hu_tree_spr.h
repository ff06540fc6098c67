// What the host half (hu_spr_host.cpp, a plain C++ compiler) and the device half (hu_spr.cpp, hu_kern_spr.h) of the SPR search share
// (DESIGN.md §25): the records of a pruned node's walk, the recomputed message of one step and the arithmetic of one column of a
// target, which leaves the three ratios and the constant of §22's form.  The model, the denominators, the terms of f' and f'' and the
// safeguarded Newton are hu_tree_blen.h's, P(t) and the carried message hu_tree_nni.h's, unchanged.  Both translation units are built
// with -ffp-contract=off.
#pragma once
#include "hu_tree_nni.h"

#define HU_SPR_WG HU_BLEN_WG     /* threads of a workgroup of k_spr_score: column j belongs to thread j % HU_SPR_WG */

/* one step of a walk.  A message is named by an id: x < n is up[x], n + x is down[x], 2 n + k is slot k of the workgroup's stack, -1 none.
 * First (dst >= 0) slot dst takes, or with acc adds to itself, the message src0 carried over len0 and, when src1 >= 0, times src1
 * carried over len1: a product in log space.  Then (tnode >= 0) the target tnode is scored: its two sides sa and sb, carried over la
 * and lb, meet at the junction where the pendant of v hangs, and the outputs go to entry `out` of the pruned node. */
struct HuSprRec {
	int32_t src0, src1, dst, acc, sa, sb, tnode, dist, out, pad0;
	double len0, len1, la, lb;
};
/* a pruned node: its records, its outputs (entry 0 is the baseline), the start of the pendant */
struct HuSprNode { int64_t recOff, outOff; int32_t nRec, v; double t0; };

/* a message carried over its branch, in log space: log(P . exp(M - max M)) + max M; a message without a finite entry stays one */
HU_BLEN_HD void hu_spr_conv(const double* P, const double* M, double* Y) {
	double v[4];
	const double mx = hu_nni_carry(P, M, v);
	for(int i = 0; i < 4; ++i) Y[i] = log(v[i]) + mx;
}

/* one column of one target: A and B the two sides of the edge in log space, carried by Pa and Pb to the junction, Yv = up[v];
 * r[3] = c_k / c_0 and K = log c_0 + the three maxima, with hu_nni_pair's rule for a column of likelihood 0 */
HU_BLEN_HD void hu_spr_column(const HuBlenModel& m, const double* Pa, const double* A, const double* Pb, const double* B, const double* Yv, double* r, double* K) {
	double a[4], b[4], x[4], y[4];
	const double sa = hu_nni_carry(Pa, A, a), sb = hu_nni_carry(Pb, B, b), my = hu_blen_max4(Yv);
	if(!(my > -INFINITY)) { r[0] = r[1] = r[2] = 0.0; *K = -INFINITY; return; }
	for(int i = 0; i < 4; ++i) { x[i] = a[i] * b[i]; y[i] = exp(Yv[i] - my); }
	hu_nni_pair(m, x, y, (sa + sb) + my, r, K);
}

/* ---- the host half, hu_spr_host.cpp ---- */
/* the prunable nodes in ascending v and the number of the others */
void hu_spr_prunable(const HuBlenTopo& tp, const int32_t* parent, std::vector<int32_t>* nodes, int64_t* skipped);
/* the walk of v appended to recs: the baseline, then per target the records of its recomputed side with the target in the last one;
 * returns the outputs of v, the baseline included */
int32_t hu_spr_walk(const HuBlenTopo& tp, const int32_t* parent, const double* blen, int32_t radius, int32_t v, std::vector<HuSprRec>* recs);
/* the outputs of a slab's nodes from the messages up, down [n][L][4]: tStar, f [outputs of the slab], f0 [nodes]; stack [radius][L][4] */
void hu_spr_host_score(const HuBlenModel& m, int32_t n, int64_t L, const HuSprNode* nodes, size_t nNodes, const HuSprRec* recs, int64_t recBase, int64_t outBase,
		const double* up, const double* down, double lo, double hi, double* stack, double* t_star, double* f, double* f0);
/* the scores of a tree: per prunable node the baseline and, in CSR, its targets */
struct HuSprScores {
	std::vector<int32_t> v, w, dist; std::vector<int64_t> off; std::vector<double> baseT, baseF, f0, t, f;
	int64_t skipped = 0;
};
/* a slab scored: nodes [nNodes], their records (recBase the first one's index) and outputs (outBase) -> tStar, f [nOut], f0 [nNodes] */
typedef std::function<int(const HuSprNode*, size_t, const HuSprRec*, size_t, int64_t, int64_t, size_t, double*, double*, double*)> HuSprSlabFn;
/* the nodes a launch takes at the most, from the bounds of the header and opts->slab */
int64_t hu_spr_slab_nodes(const hu_spr_opts* o, int32_t cs_len);
/* plans the walks slab by slab, has each slab scored and gathers the outputs; count_only: the sizes of out->v and out->off alone */
int hu_spr_scores(const char* fn, const hu_spr_opts* o, const HuBlenTopo& tp, int32_t cs_len, const int32_t* parent, const double* blen, bool count_only,
		const HuSprSlabFn& slab, HuSprScores* out);
/* the regraft on the arrays, checked: HU_OK or HU_ERR_ARG with the message set; dist (may be NULL) is not computed here */
int hu_spr_apply(const char* fn, int32_t n, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t v, int32_t w, double t);
/* the checks of the entries (hu_blen_check's and the SPR options'), with the need held against the budget */
int hu_spr_check(const char* fn, const hu_spr_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp);
/* the round loop over either half.  fit(parent, blen, &ll): hu_tree_optimize_lengths in place; score(parent, blen, tp, &scores);
 * trial(parent, blen, &ll): one up sweep and hu_tree_loglik */
struct HuSprOps {
	std::function<int(const int32_t*, double*, double*)> fit;
	std::function<int(const int32_t*, const double*, const HuBlenTopo&, HuSprScores*)> score;
	std::function<int(const int32_t*, const double*, double*)> trial;
};
int hu_spr_rounds(const char* fn, hu_spr_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq, const int32_t* child_off,
		int32_t* child_idx, const HuSprOps& ops, double* seconds);
/* the two entries on the host path */
int hu_spr_host_scores_entry(const char* fn, const hu_spr_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, bool count_only, HuSprScores* out);
int hu_spr_host_search_entry(const char* fn, hu_spr_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuBlenModel& m, double* seconds);
