// What the host half (hu_support_host.cpp, a plain C++ compiler) and the device half (hu_support.cpp, hu_kern_support.h) of the local
// branch supports share: the draw of a replicate, the value of one column of an edge's three arrangements at their own
// optima, and the rule of a supporting replicate.  The column arithmetic is hu_tree_nni.h's, unchanged.  Both translation units are
// built with -ffp-contract=off: S is a multiply and then an add.
#pragma once
#include "hu_tree_nni.h"
#include "hu_sim_rng.h"

#define HU_SUPPORT_RPT 4              /* replicates a thread of k_nni_support holds: one 8-byte read gives their four counts */
#define HU_SUPPORT_DOMAIN 0x53555050u /* the last counter word of every draw: "SUPP" */

/* the replicates of the table, padded so that a thread's HU_SUPPORT_RPT counts are one aligned read */
HU_BLEN_HD int64_t hu_support_bpad(int64_t B) { return (B + HU_SUPPORT_RPT - 1) / HU_SUPPORT_RPT * HU_SUPPORT_RPT; }

/* the four draws i = 4 g .. 4 g + 3 of replicate b among L columns; a caller drops those with i >= L */
HU_BLEN_HD void hu_support_draw4(uint64_t seed, uint32_t b, uint32_t g, uint32_t L, uint32_t* col) {
	const uint32_t key[2] = {(uint32_t) seed, (uint32_t)(seed >> 32)}, ctr[4] = {g, b, 0u, HU_SUPPORT_DOMAIN};
	uint32_t w[4];
	hu_philox4x32_10(ctr, key, w);
	for(int k = 0; k < 4; ++k) col[k] = (uint32_t)(((uint64_t) w[k] * L) >> 32);
}

/* one column of one edge: K [3] and logD [3] = log D^q(t*_q) of the three arrangements, whose sum is l^q, and d [2] = max(l^q - l^0,
 * -DBL_MAX) for q = 1, 2.  Returns whether l^0 is finite; d is 0 where it is not.  E [3]: hu_blen_exp at the three optima */
HU_BLEN_HD bool hu_support_column(const HuBlenModel& m, const double* P, const double* M, const HuBlenExp* E, double* K, double* logD, double* d) {
	double r[9], l[3];
	hu_nni_column(m, P, M, r, K);
	for(int q = 0; q < 3; ++q) { logD[q] = log(hu_blen_den(E[q], r + q * 3)); l[q] = K[q] + logD[q]; }
	if(!(l[0] > -INFINITY) || !(l[0] < INFINITY)) { d[0] = d[1] = 0.0; return false; }
	d[0] = fmax(l[1] - l[0], -DBL_MAX); d[1] = fmax(l[2] - l[0], -DBL_MAX);
	return true;
}

/* the tie threshold of an edge and the rule of a supporting replicate */
HU_BLEN_HD double hu_support_eta(double f0) { return HU_SUPPORT_TIE * fabs(f0); }
HU_BLEN_HD bool hu_support_supports(double S1, double S2, double eta) { return S1 < -eta && S2 < -eta; }

/* ---- the host half, hu_support_host.cpp ---- */
/* the checks of the entry: hu_nni_check's with the need of the supports held against the budget */
int hu_support_check(const char* fn, const hu_support_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		HuBlenTopo* tp, hu_nni_opts* no);
/* f2 [E][3], count [E], sums [E][B][2] (may be NULL) of the edges from the messages and the optima; w [B][L].  *bad: the first edge with a
 * column whose l^0 is not finite, -1 for none */
void hu_support_host_edges(const HuBlenModel& m, int32_t n, int64_t L, int64_t B, const std::vector<HuNniEdge>& edges, const double* up, const double* down,
		const double* t_star, const uint16_t* w, double* f2, int32_t* count, double* sums, int64_t* bad);
/* what both halves do with the kernel's or the host's outputs: f2 against the scorer's f to the bit, and the refusal of a tree of likelihood 0 */
int hu_support_verify(const char* fn, const std::vector<HuNniEdge>& edges, const double* f, const double* f2, int64_t bad);
int hu_support_host_entry(const char* fn, const hu_support_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, int32_t* count,
		double* sums, double* seconds);
