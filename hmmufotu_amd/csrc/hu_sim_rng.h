// The random numbers of hmmufotu-amd-sim: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
// as 1, 2, 3", SC'11), counter-based, so a draw is a function of (key, counter) and needs no state: the kernel (hu_kern_sim.h) and the
// host's rejection loop (hu_sim.cpp) name their draws by read, column and attempt, and a result never depends on how the reads were
// split over launches.  Host and device run the same integer code.  hmmufotu-amd-subset names the reads of an OTU table
// with it too; its host half (hu_otu_table.cpp) is built by a plain C++ compiler, which sees this header without the HIP runtime's.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HU_HD __host__ __device__
#else
#define HU_HD
#endif

/* out = Philox4x32-10(counter, key): ten rounds of two 32 x 32 -> 64 bit products, the key raised by the Weyl constants between rounds */
HU_HD inline void hu_philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
	uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
#ifdef __HIPCC__
	#pragma unroll
#endif
	for(int r = 0; r < 10; ++r) {
		const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
		const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t) p1; c3 = (uint32_t) p0; c0 = n0; c2 = n2;
		k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
	}
	out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
/* a uniform double of [0, 1) from two words: the 27 high bits of hi above the 26 high bits of lo, a 53-bit integer times 2^-53 */
HU_HD inline double hu_sim_u01(uint32_t hi, uint32_t lo) {
	return (double)(((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6)) * 0x1p-53;
}
