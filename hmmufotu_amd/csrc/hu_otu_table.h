// What the host half (hu_otu_table.cpp, a plain C++ compiler) and the device half (hu_otu_subset.cpp, hu_kern_draw.h, hu_kern_otu.h) of hu_otu_subset
// share: the names of a read's key and of a draw, and the checks of a table before it is subsampled.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_sim_rng.h"
#include "../../include/hmmufotu_amd.h"

#define HU_OTU_CHUNK 16384

/* the key of read t of sample j: the first two words of the counter (t, j, 2), the high key_bits of them */
HU_HD inline uint64_t hu_otu_key(const uint32_t k[2], uint64_t t, uint32_t j, int key_bits) {
	const uint32_t c[4] = {(uint32_t) t, (uint32_t)(t >> 32), j, 2u};
	uint32_t w[4];
	hu_philox4x32_10(c, k, w);
	return (((uint64_t) w[0] << 32) | w[1]) >> (64 - key_bits);
}
/* the read that draw m of sample j takes out of T: the high half of r * T, r the first two words of the counter (m, j, 3) */
HU_HD inline uint64_t hu_otu_draw(const uint32_t k[2], uint64_t m, uint32_t j, uint64_t T) {
	const uint32_t c[4] = {(uint32_t) m, (uint32_t)(m >> 32), j, 3u};
	uint32_t w[4];
	hu_philox4x32_10(c, k, w);
	const uint64_t r = ((uint64_t) w[0] << 32) | w[1];
#ifdef __HIP_DEVICE_COMPILE__
	return __umul64hi(r, T);
#else
	return (uint64_t)(((unsigned __int128) r * T) >> 64);
#endif
}

/* the arguments of hu_otu_subset, checked; total [n_sample]: the column sums, each < 2^32 */
int hu_otu_subset_check(const char* fn, int64_t n_otu, int64_t n_sample, const double* counts, uint64_t size, int method, const hu_otu_opts* opts,
		const double* out, hu_otu_opts* eff, std::vector<uint64_t>& total);
/* the cells alone: non-negative integers, every column sum below 2^32 (hu_alpha_host.cpp asks the same of its table) */
int hu_otu_cells_check(const char* fn, int64_t n_otu, int64_t n_sample, const double* counts, std::vector<uint64_t>& total);
/* the host path, on checked arguments */
void hu_otu_subset_host(int64_t n_otu, int64_t n_sample, const double* counts, const std::vector<uint64_t>& total, uint64_t size, int method, uint64_t seed,
		int key_bits, double* out);
