// What the host half (hu_alpha_host.cpp, a plain C++ compiler) and the device half (hu_alpha.hip, hu_kern_alpha.h) of hu_alpha share
// (DESIGN.md §30): the records both read (those of a draw are hu_draw.h's), the plan of a call, made on the host from a checked table and
// one walk of the tree, and the constants that fix the order in which A and PD are added.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_otu_table.h"
#include "hu_draw.h"
#include "hu_unifrac.h"

#define HU_AL_WG 256             /* threads of every workgroup; the order of A and PD is a function of it */
#define HU_AL_WAVES 4
#define HU_AL_DT 8               /* depths of one (sample, repeat) that one key computation serves: the DT of hu_kern_draw.h */

/* a kept branch below which the sample has a nonzero cell: its length and its cells [lo, hi), lo < hi <= nnz; ascending branch number */
struct HuAlBranch { double b; uint32_t lo, hi; };
/* what comes back, one per draw */
struct HuAlStat { uint64_t Q; double A, PD; uint32_t S, F1, F2, pad; };

struct HuAlUnit { int32_t smp, depth, rep; };                 /* depth -1: the whole sample */

struct HuAlPlan {
	int64_t M = 0, S = 0, B = 0, nDepth = 0, reps = 0;
	bool hasTree = false, host = false;
	int32_t chunk = HU_OTU_CHUNK, keyBits = 64;
	int64_t drawChunk = 0, budget = 0;
	uint64_t seed = 0;
	std::vector<uint64_t> depth;
	std::vector<HuAlSample> smp;
	std::vector<uint32_t> prefix;        /* per sample nnz + 1, the cells in table order: it numbers the reads */
	std::vector<uint32_t> slot;          /* per sample nnz: the place of that cell among the sample's in depth-first row order */
	std::vector<HuAlBranch> br;
	std::vector<uint32_t> brK;           /* beside br: the number of the kept branch (hu_unifrac_rarefied's embedding) */
	std::vector<HuAlUnit> unit;          /* the whole samples, then the existing draws by (sample, repeat, depth) */
	int64_t maxNnz = 0, maxChunk = 0;    /* the largest nnz and the largest ceil(T / chunk) of a sample */
};

/* the arguments of hu_alpha, checked, and the plan */
int hu_al_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, uint64_t seed, const hu_alpha_opts* opts, HuAlPlan& pl);
/* the host path: one record per unit */
void hu_al_host(const HuAlPlan& pl, std::vector<HuAlStat>& stat);
/* the records of the units into the outputs, metrics included */
void hu_al_fill(const HuAlPlan& pl, const std::vector<HuAlStat>& stat, hu_alpha_rec* whole, hu_alpha_rec* draws);
inline int64_t hu_al_need_of(const HuAlPlan& pl, int64_t n_draw) {
	return hu_alpha_need(pl.S, (int64_t) pl.prefix.size() - pl.S, (int64_t) pl.br.size(), pl.maxNnz, pl.maxChunk, n_draw);
}
