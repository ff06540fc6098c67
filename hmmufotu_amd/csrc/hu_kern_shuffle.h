// The labellings of a chunk of permutations (hmmufotu-amd-permanova, hmmufotu-amd-diffabund).
//
//   k_label_shuffle   a thread per slot of the chunk: copies the observed labels into its column of lab [n][cp] (cp = the chunk padded to
//                     whole workgroups), then runs the Fisher-Yates shuffle of permutation first + slot on that column (hu_pm_shuffle:
//                     Philox4x32-10 by (seed, p, i), the code the host runs).  Sample-major, so that the threads of a wave touch
//                     consecutive labels at step i and the staging loads of the kernels that read them are coalesced.  With `observed`
//                     the copy alone: every slot then holds the observed labelling.  T: 16-bit labels, or bytes where a <= 64 is known.
#pragma once
#include "hu_common.h"
#include "hu_permanova.h"

template<class T> __global__ void __launch_bounds__(64) k_label_shuffle(const T* __restrict__ obs, T* __restrict__ lab, int64_t n, int64_t cp,
		uint64_t first, uint64_t seed, int observed) {
	const int64_t slot = (int64_t) blockIdx.x * 64 + threadIdx.x;
	if(slot >= cp) return;
	T* g = lab + slot;
	for(int64_t i = 0; i < n; ++i) g[i * cp] = obs[i];
	if(!observed) hu_pm_shuffle(seed, first + (uint64_t) slot, n, g, cp);
}
