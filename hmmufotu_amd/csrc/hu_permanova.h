// What the host half (hu_permanova_host.cpp, a plain C++ compiler) and the device half (hu_permanova.cpp, hu_kern_permanova.h) of
// hu_permanova share: the checked arguments of a call, the constants that fix the summation order, and the shuffle
// that names the labelling of permutation p by (seed, p) alone.
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
/* the partner j in [0, i] of position i in the shuffle of permutation p: no rejection, so j is off the uniform by (i + 1) / 2^64 at the most */
HU_HD inline uint64_t hu_pm_partner(uint64_t seed, uint64_t p, uint64_t i) {
	const uint32_t c[4] = {(uint32_t) i, (uint32_t)(i >> 32), (uint32_t) p, (uint32_t)(p >> 32)}, k[2] = {(uint32_t) seed, (uint32_t)(seed >> 32)};
	uint32_t w[4];
	hu_philox4x32_10(c, k, w);
	return hu_pm_mulhi64(((uint64_t) w[1] << 32) | w[0], i + 1);
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
