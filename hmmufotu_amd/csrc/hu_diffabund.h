// What the host half (hu_diffabund_host.cpp, a plain C++ compiler) and the device half (hu_diffabund.cpp, hu_kern_diffabund.h) of
// hu_diffabund share: the plan of a call (the ranked nonzero cells of the tested OTUs), the 128-bit statistic T and
// the reported H as functions that both halves compile, and the constants that fix the shapes of the kernels.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_permanova.h"

#define HU_DA_WG 256             /* permutations per workgroup: a chunk is padded to whole workgroups */
#define HU_DA_BLOCK 64           /* tested OTUs per workgroup of k_da_sums, in table order */
#define HU_DA_STAGE 1024         /* cells of a row staged in LDS at a time; a longer row is walked in pieces */
#define HU_DA_MAX_SAMPLES 16384  /* a cell is sample << 16 | (e_j - e_z), and |D_g| <= 2 N^2 stays below 2^31 */
#define HU_DA_MAX_GROUPS 64      /* the accumulators of k_da_sums are [a][256] words of LDS */
#define HU_DA_MAX_PERMS 10000000
#define HU_DA_MAX_CHUNK 16384    /* the default chunk's ceiling */

/* T += c^2 w in unsigned 128-bit arithmetic as two halves; |c| <= N^2 <= 2^28, so c^2 fits 64 bits */
HU_HD inline void hu_da_T_add(uint64_t& hi, uint64_t& lo, int64_t c, uint64_t w) {
	const uint64_t c2 = (uint64_t)(c * c), pl = c2 * w, ph = hu_pm_mulhi64(c2, w);
	const uint64_t s = lo + pl;
	hi += ph + (s < lo ? 1 : 0);
	lo = s;
}
HU_HD inline bool hu_da_T_ge(uint64_t hi, uint64_t lo, uint64_t ohi, uint64_t olo) { return hi > ohi || (hi == ohi && lo >= olo); }
/* the reported statistic: plain IEEE operations in this order, no fma (both halves are compiled with -ffp-contract=off).
 * dL = (double) L, c2 = 3.0 / ((double) N * (double) (N + 1)), tc = the OTU's tie correction: one rounding each, made on the host */
HU_HD inline double hu_da_H(uint64_t hi, uint64_t lo, double dL, double c2, double tc) {
	const double x = (double) hi * 18446744073709551616.0 + (double) lo;
	return ((x / dL) * c2) / tc;
}

struct HuDaPlan {
	int64_t n = 0, a = 0, n_otu = 0, perms = 0, chunk = 0, budget = 0;
	uint64_t seed = 1;
	bool host = false;
	uint64_t L = 1;
	double dL = 1, c2 = 0;
	std::vector<uint8_t> lab;        /* [n] the observed labels */
	std::vector<int64_t> size;       /* [a] n_g */
	std::vector<uint64_t> w;         /* [a] L / n_g */
	std::vector<int64_t> prevalence; /* [n_otu] nonzero cells of every OTU */
	std::vector<int64_t> row;        /* [m] the tested OTUs, in table order */
	std::vector<int64_t> ptr;        /* [m + 1] into cell */
	std::vector<uint32_t> cell;      /* sample << 16 | (e_j - e_z) of every cell above 0 of the tested OTUs */
	std::vector<int32_t> ez;         /* [m] e_z = -(the cells above 0) */
	std::vector<int32_t> dsum;       /* [m] the sum of e_j - e_z over the row */
	std::vector<double> tc;          /* [m] 1 - sum (t^3 - t) / (N^3 - N), above 0 */
};

inline int64_t hu_da_pad(int64_t chunk) { return (chunk + HU_DA_WG - 1) / HU_DA_WG * HU_DA_WG; }
inline int64_t hu_da_blocks(int64_t m) { return (m + HU_DA_BLOCK - 1) / HU_DA_BLOCK; }

/* the arguments of hu_diffabund, checked, and the plan: totals, ranks, tie sums, L and the cells */
int hu_da_plan(const char* fn, int64_t n_otu, int64_t n_sample, const double* counts, const int32_t* group, const hu_diffabund_opts* opts, HuDaPlan& pl);
/* the labelling of permutation p into g [n] */
void hu_da_host_shuffle(const HuDaPlan& pl, uint64_t p, uint8_t* g);
/* T of tested row r under the labelling g; C [a] (may be null) receives the group sums */
void hu_da_host_T(const HuDaPlan& pl, int64_t r, const uint8_t* g, uint64_t* hi, uint64_t* lo, int64_t* C);
/* the whole host path: per tested row T and H of the observed labelling and the count of T(pi) >= T(observed), per permutation M(pi) */
void hu_da_host_run(const HuDaPlan& pl, uint64_t* tobs /* [m][2] hi, lo */, double* hobs, int64_t* count, double* maxstat);
/* the records from what either path computed: p, p_maxT, q and best */
void hu_da_result(const HuDaPlan& pl, const uint64_t* tobs, const double* hobs, const int64_t* count, const double* maxstat, hu_diffabund_rec* rec);
