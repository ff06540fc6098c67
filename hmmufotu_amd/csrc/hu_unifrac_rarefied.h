// What the host half (hu_unifrac_rarefied_host.cpp, a plain C++ compiler) and the device half (hu_unifrac_rarefied.hip,
// hu_kern_unifrac_rarefied.h) of hu_unifrac_rarefied share: the plan of a call, which joins hu_alpha's resident table
// (hu_alpha.h) with hu_unifrac's branches and slabs (hu_unifrac.h), and the recurrence of the mean.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_alpha.h"

struct HuUrPlan {
	HuAlPlan al;                         /* every sample of the table, dropped ones too: a sample's index is its column, which keys its draws */
	HuUfPlan uf;                         /* the branches of the ids; S = the kept samples, L and nSlab those of (S', B) */
	std::vector<int32_t> keptCol;        /* [S'] the kept columns, ascending */
	std::vector<uint64_t> total;         /* [n_sample] */
	int64_t nSample = 0, Sk = 0, reps = 0;
	uint64_t depth = 0, seed = 0, maxDepth2 = 0;
	bool host = false;
	int64_t drawChunk = 0, budget = 0;
};

/* the arguments of hu_unifrac_rarefied, checked, and the plan */
int hu_ur_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, uint64_t seed, const hu_unifrac_rarefied_opts* opts, HuUrPlan& pl);
/* one step of the recurrence: x is draw number r (1-based) */
HU_HD inline void hu_ur_step(double x, double r, double& mean, double& m2) {
	const double d = x - mean;
	mean = mean + d / r;
	m2 = m2 + d * (x - mean);
}
/* the host path: mean, m2 [S'][S'], draws [R][S'][S'] or NULL */
void hu_ur_host(const HuUrPlan& pl, const double* counts, double* mean, double* m2, double* draws);
/* sd from m2, in place */
void hu_ur_sd(int64_t n, int64_t reps, const double* m2, double* sd);
inline int64_t hu_ur_need_of(const HuUrPlan& pl, int64_t n_draw, bool wantDraws) {
	return hu_unifrac_rarefied_need(pl.nSample, pl.Sk, (int64_t) pl.al.prefix.size() - pl.al.S, (int64_t) pl.al.br.size(), pl.al.maxNnz, pl.al.maxChunk, pl.uf.B,
		pl.uf.L, n_draw, wantDraws ? 1 : 0);
}
