// What the host half (hu_permanova_design_host.cpp, a plain C++ compiler) and the device half (hu_permanova_design.cpp,
// hu_kern_permanova_design.h) of hu_permanova_design share: the checked arguments of a call, the constants that fix the
// layout and the order of the sums, and the stratified shuffle that names the index array of permutation p by (seed, p, strata) alone.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_permanova.h"
#include "hu_pcoa.h"

#define HU_PMD_SLOT 64           /* permutations per workgroup of the shuffle: a chunk is padded to whole workgroups */
#define HU_PMD_VC 64             /* virtual columns are padded to whole widest column blocks (16 NT, NT = 4) */
#define HU_PMD_MAX_CHUNK 16384   /* the default chunk's ceiling */
#define HU_PMD_DROP 1e-10        /* a column whose norm after projection is below this share of its norm before is dropped */

inline int64_t hu_pmd_pad(int64_t chunk) { return (chunk + HU_PMD_SLOT - 1) / HU_PMD_SLOT * HU_PMD_SLOT; }
inline int64_t hu_pmd_vcpad(int64_t chunk, int64_t q) { return (hu_pmd_pad(chunk) * q + HU_PMD_VC - 1) / HU_PMD_VC * HU_PMD_VC; }
inline int64_t hu_pmd_row_blocks(int64_t n) { return (n + HU_PCOA_TILE - 1) / HU_PCOA_TILE; }

/* the shuffle of permutation p on the n entries idx[0], idx[stride], ..., which hold the identity on entry: within every stratum
 * (members member[start[s]] < ... < member[start[s + 1] - 1]) a Fisher-Yates shuffle whose step t is named by the sample it moves */
template<class T> HU_HD inline void hu_pmd_shuffle(uint64_t seed, uint64_t p, int64_t S, const int32_t* member, const int32_t* start, T* idx, int64_t stride = 1) {
	for(int64_t s = 0; s < S; ++s) {
		const int32_t* m = member + start[s];
		for(int64_t t = (int64_t) start[s + 1] - start[s] - 1; t >= 1; --t) {
			const int64_t a = m[t], b = m[hu_pm_partner_in(seed, p, (uint64_t) a, (uint64_t) t + 1)];     /* the partner's rank is in [0, t] */
			const T x = idx[a * stride], y = idx[b * stride];
			idx[a * stride] = y; idx[b * stride] = x;
		}
	}
}

struct HuPmdPlan {
	int64_t n = 0, q = 0, T = 0, S = 0, perms = 0, chunk = 0, budget = 0;
	uint64_t seed = 1;
	bool host = false, index32 = false;
	std::vector<int64_t> term_start;   /* [T + 1] */
	std::vector<int32_t> member;       /* [n] the samples sorted by (stratum, index) */
	std::vector<int32_t> start;        /* [S + 1] */
};

/* the arguments of hu_permanova_design, checked (the matrix by hu_pm_check_matrix), and the plan */
int hu_pmd_plan(const char* fn, int64_t n, const double* dist, const double* Q, int64_t q, int64_t T, const int64_t* term_start, const int32_t* strata,
		const hu_permanova_design_opts* opts, HuPmdPlan& pl);
/* the host path: ss [(1 + perms)][T], row 0 the identity, row 1 + p permutation p */
void hu_pmd_host_run(const HuPmdPlan& pl, const double* dist, const double* Q, double* ss);
/* SS_res, F, R2, the counts and p of every term from ss [(1 + perms)][T] */
void hu_pmd_result(const HuPmdPlan& pl, double ssT, const double* ss, hu_permanova_design_term* out);
