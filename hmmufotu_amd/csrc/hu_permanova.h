// What the host half (hu_permanova_host.cpp, a plain C++ compiler) and the device half (hu_permanova.cpp, hu_kern_permanova.h) of
// hu_permanova share: the checked arguments of a call, the constants that fix the summation order, and the shuffle
// that names the labelling of permutation p by (seed, p) alone.  The shuffle and the check of the group labels are hu_diffabund's too.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_sim_rng.h"
#include "../../include/hmmufotu_amd.h"

#define HU_PM_TILE 64            /* samples per side of a tile of the matrix */
#define HU_PM_WG 256             /* permutations per workgroup of the pair kernel: a chunk is padded to whole workgroups */
#define HU_PM_MAX_GROUPS 65535   /* a label is 16 bits on the device */
#define HU_PM_MAX_PERMS 10000000
#define HU_PM_MAX_CHUNK 16384    /* the default chunk's ceiling */

/* the high 64 bits of a 64 x 64 bit product */
HU_HD inline uint64_t hu_pm_mulhi64(uint64_t x, uint64_t y) {
#ifdef __HIP_DEVICE_COMPILE__
	return __umul64hi(x, y);
#else
	return (uint64_t)(((unsigned __int128) x * y) >> 64);
#endif
}
/* a partner in [0, range) drawn under the counter (counter, p): no rejection, so it is off the uniform by range / 2^64 at the most.  The
 * stratified shuffle of hu_permanova_design.h names a step by the sample it moves (the counter) and draws among the step's candidates */
HU_HD inline uint64_t hu_pm_partner_in(uint64_t seed, uint64_t p, uint64_t counter, uint64_t range) {
	const uint32_t c[4] = {(uint32_t) counter, (uint32_t)(counter >> 32), (uint32_t) p, (uint32_t)(p >> 32)}, k[2] = {(uint32_t) seed, (uint32_t)(seed >> 32)};
	uint32_t w[4];
	hu_philox4x32_10(c, k, w);
	return hu_pm_mulhi64(((uint64_t) w[1] << 32) | w[0], range);
}
/* the partner j in [0, i] of position i in the shuffle of permutation p */
HU_HD inline uint64_t hu_pm_partner(uint64_t seed, uint64_t p, uint64_t i) { return hu_pm_partner_in(seed, p, i, i + 1); }
/* the Fisher-Yates shuffle of permutation p on the n labels g[0], g[stride], ...: the host's rows and the columns of k_label_shuffle */
template<class T> HU_HD inline void hu_pm_shuffle(uint64_t seed, uint64_t p, int64_t n, T* g, int64_t stride = 1) {
	for(int64_t i = n - 1; i >= 1; --i) {
		const int64_t j = (int64_t) hu_pm_partner(seed, p, (uint64_t) i);          /* 0 <= j <= i < n */
		const T x = g[i * stride], y = g[j * stride];
		g[i * stride] = y; g[j * stride] = x;
	}
}

void hu_set_error(const char* fmt, ...);
/* the labels of n samples: none negative, dense in 0 .. a-1, 2 <= a <= min(n - 1, max_groups); size [a] receives the groups' sizes.
 * `single` ends the refusal of groups that are all single samples with what the test would lack */
inline int hu_groups_check(const char* fn, int64_t n, const int32_t* group, int64_t max_groups, const char* single, std::vector<int64_t>& size) {
	int64_t top = -1;
	for(int64_t i = 0; i < n; ++i) {
		if(group[i] < 0) { hu_set_error("%s: sample %lld has the negative label %d", fn, (long long) i, group[i]); return HU_ERR_ARG; }
		top = top > group[i] ? top : (int64_t) group[i];
	}
	if(top >= n) { hu_set_error("%s: the labels are not dense in 0 .. a-1: label %lld among %lld samples", fn, (long long) top, (long long) n); return HU_ERR_ARG; }
	const int64_t a = top + 1;
	size.assign((size_t) a, 0);
	for(int64_t i = 0; i < n; ++i) ++size[(size_t) group[i]];
	for(int64_t g = 0; g < a; ++g) if(size[(size_t) g] == 0) {
		hu_set_error("%s: the labels are not dense in 0 .. a-1: label %lld is used, label %lld is not", fn, (long long) top, (long long) g); return HU_ERR_ARG; }
	if(a < 2) { hu_set_error("%s: one group: a test needs 2 at the least", fn); return HU_ERR_ARG; }
	if(a > n - 1) { hu_set_error("%s: %lld groups of %lld samples: every group is a single sample, %s", fn, (long long) a, (long long) n, single); return HU_ERR_ARG; }
	if(a > max_groups) { hu_set_error("%s: %lld groups: %lld at the most", fn, (long long) a, (long long) max_groups); return HU_ERR_ARG; }
	return HU_OK;
}

struct HuPmPlan {
	int64_t n = 0, a = 0, perms = 0, chunk = 0, budget = 0;
	uint64_t seed = 1;
	bool host = false;
	std::vector<double> inv;        /* [a] 1 / n_g, one rounded division each */
	std::vector<uint16_t> lab;      /* [n] the observed labels */
};

inline int64_t hu_pm_tiles(int64_t n) { const int64_t nt = (n + HU_PM_TILE - 1) / HU_PM_TILE; return nt * (nt + 1) / 2; }
inline int64_t hu_pm_pad(int64_t chunk) { return (chunk + HU_PM_WG - 1) / HU_PM_WG * HU_PM_WG; }

/* the arguments of hu_permanova, checked, and the plan */
int hu_pm_plan(const char* fn, int64_t n, const double* dist, const int32_t* group, const hu_permanova_opts* opts, HuPmPlan& pl);
/* the matrix alone: finite, non-negative, squares finite, zero diagonal, symmetric, not all zero; hu_pcoa refuses by the same code */
int hu_pm_check_matrix(const char* fn, int64_t n, const double* dist);
/* SS_T: no label in it, so both paths take it from here */
double hu_pm_ss_total(int64_t n, const double* dist);
/* the host path: SS_W of the labelling g [n] on D2 [n][n] (the squares; only j > i is read) */
double hu_pm_host_ssw(const HuPmPlan& pl, const double* D2, const uint16_t* g);
/* the labelling of permutation p into g [n] */
void hu_pm_host_shuffle(const HuPmPlan& pl, uint64_t p, uint16_t* g);
/* the whole host path: *obs and ssw [perms] */
void hu_pm_host_run(const HuPmPlan& pl, const double* dist, double* obs, double* ssw);
/* F, R2, count_le and p from the sums */
void hu_pm_result(const HuPmPlan& pl, double ssT, double obs, const double* ssw, hu_permanova_result* out);
