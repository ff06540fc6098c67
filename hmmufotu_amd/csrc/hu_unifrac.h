// What the host half (hu_unifrac_host.cpp, a plain C++ compiler) and the device half (hu_unifrac.cpp, hu_kern_unifrac.h) of hu_unifrac
// share: the plan of a call, made on the host from one walk of the tree, and the constants that fix the summation order.
#pragma once
#include <stdint.h>
#include <vector>
#include "../../include/hmmufotu_amd.h"

#define HU_UF_TILE 64            /* samples per side of a tile of the pair matrix */
#define HU_UF_CHUNK 32           /* branches staged at a time */
#define HU_UF_SCAN_ROWS 256      /* rows per block of the two-level column scan */
#define HU_UF_WANT_WG 1024       /* workgroups the default slab aims at */

struct HuUfPlan {
	int64_t M = 0, S = 0, B = 0;         /* rows, samples, kept branches */
	int64_t L = 0, nSlab = 0;            /* branches per slab, slabs (0 when B == 0) */
	int32_t method = 0;                  /* HU_UF_UNWEIGHTED / WEIGHTED / WEIGHTED_RAW / GENERALIZED: the identity methods and alpha 1 are folded in */
	double alpha = 0.5;
	bool host = false;
	int64_t budget = 0;
	std::vector<int64_t> perm;           /* [M] the rows in depth-first order of their nodes (stable) */
	bool permIsIdentity = true;
	std::vector<int32_t> lo, hi;         /* [B] the rows (in that order) of branch k's subtree: [lo, hi) */
	std::vector<int32_t> node;           /* [B] the node below branch k (identity tree: the row) */
	std::vector<double> b;               /* [B] its length */
};

/* the arguments of hu_unifrac, checked, and the plan; dist and pd are not looked at */
int hu_uf_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, HuUfPlan& pl);
/* the host path, on a plan: P [B][S] */
void hu_uf_host_embed(const HuUfPlan& pl, const double* counts, double* P);
/* dist [S][S], pd [S] or NULL, from P */
void hu_uf_host_pairs(const HuUfPlan& pl, const double* P, double* dist, double* pd);
/* the tiles of the upper triangle */
inline int64_t hu_uf_tiles(int64_t S) { const int64_t nt = (S + HU_UF_TILE - 1) / HU_UF_TILE; return nt * (nt + 1) / 2; }
