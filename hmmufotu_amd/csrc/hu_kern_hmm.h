// Profile-HMM training counts on the device (the double loop of BandedHMMP7::build, src/BandedHMMP7.cpp:424-465).
// The MSA is the pruned text, row-major [nSeq][csLen], classified through the 256-entry table of hu_msa_encode_table; a column is a
// match column where mask[j] != 0.  A cell's state is determineMatchingState (src/BandedHMMP7.h:713-716): match column with a
// residue M, match column without one D, other column with a residue I, other column without one P (skipped).
// Two kernels: k_hmm_states finds, per row, every cell's own state and the state of the nearest non-P cell to its right;
// k_hmm_counts adds the weights up per column, every sum a serial chain over the rows in ascending order, so that the sums of
// a match column are the reference's bit for bit.
#pragma once
#include "hu_common.h"

#define HU_HMM_M 0
#define HU_HMM_I 1
#define HU_HMM_D 2
#define HU_HMM_NONE 3          /* own state: P; next state: no non-P cell to the right */
#define HU_HMM_COL_VALUES 9    /* per column: 4 emissions, then M->M M->I M->D D->M D->D (match column) or I->M I->I (other column) */

/* one lane per sequence: the row is walked from the last column to the first, carrying the state of the nearest non-P cell to the
 * right.  plane [nSeq][csLen]: own state | next state << 2 | base << 4 (base 0 where the cell holds no residue).  Every lane walks
 * its own row, as in k_msa_seq_weight: the strided access is paid once per training. */
__global__ __launch_bounds__(64) void k_hmm_states(const char* __restrict__ msa, int64_t nSeq, int64_t csLen, const int8_t* __restrict__ encTab,
		const uint8_t* __restrict__ mask, uint8_t* __restrict__ plane) {
	__shared__ int8_t enc[256];
	for(int c = threadIdx.x; c < 256; c += 64) enc[c] = encTab[c];
	__syncthreads();
	const int64_t i = (int64_t) blockIdx.x * 64 + threadIdx.x;
	if(i >= nSeq) return;
	const char* row = msa + i * csLen;
	uint8_t* out = plane + i * csLen;
	unsigned nxt = HU_HMM_NONE;
	for(int64_t j = csLen - 1; j >= 0; --j) {
		const int8_t b = enc[(unsigned char) row[j]];
		const bool match = mask[j] != 0, res = b >= 0;
		const unsigned own = match ? (res ? HU_HMM_M : HU_HMM_D) : (res ? HU_HMM_I : HU_HMM_NONE);
		out[j] = (uint8_t)(own | nxt << 2 | (res ? (unsigned) b : 0u) << 4);
		if(own != HU_HMM_NONE) nxt = own;
	}
}

/* one lane per column, sequences added in i order; 8 rows are loaded ahead of the serial additions (k_msa_wcounts).  w [nSeq]: the
 * weights.  out [csLen][9].  A transition is counted when the row has a non-P cell to the right and the pair is neither I->D nor
 * D->I (src/BandedHMMP7.cpp:456-463).  Plain loads, adds and stores: no atomics, nothing across lanes. */
__global__ __launch_bounds__(256) void k_hmm_counts(const uint8_t* __restrict__ plane, int64_t nSeq, int64_t csLen, const uint8_t* __restrict__ mask,
		const double* __restrict__ w, double* __restrict__ out) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	const unsigned emit = mask[j] != 0 ? HU_HMM_M : HU_HMM_I;     /* the state of this column that emits */
	double e0 = 0, e1 = 0, e2 = 0, e3 = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;     /* named, not an indexed array: no scratch */
	constexpr int AHEAD = 8;
	for(int64_t i0 = 0; i0 < nSeq; i0 += AHEAD) {
		const int k = (int) min<int64_t>(AHEAD, nSeq - i0);
		uint8_t c[AHEAD];
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) c[t] = t < k ? plane[(i0 + t) * csLen + j] : (uint8_t) HU_HMM_NONE;
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) if(t < k) {
			const unsigned own = c[t] & 3u, nxt = (c[t] >> 2) & 3u, b = c[t] >> 4;
			if(own == HU_HMM_NONE) continue;
			const double x = w[i0 + t];
			if(own == emit) {
				if(b == 0) e0 += x; else if(b == 1) e1 += x; else if(b == 2) e2 += x; else e3 += x;
				if(nxt == HU_HMM_M) t0 += x;
				else if(nxt == HU_HMM_I) t1 += x;
				else if(nxt == HU_HMM_D && emit == HU_HMM_M) t2 += x;
			}
			else { /* D: only in a match column */
				if(nxt == HU_HMM_M) t3 += x; else if(nxt == HU_HMM_D) t4 += x;
			}
		}
	}
	double* o = out + j * HU_HMM_COL_VALUES;
	o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3; o[4] = t0; o[5] = t1; o[6] = t2; o[7] = t3; o[8] = t4;
}
