// HIP kernels of a run that summarises its own batches (hmmufotu-amd --otu-table / --otu-cs; gfx950, wave64).
// Included by hu_engine.hip after hu_kern_align.h (HuAlnDev) and hu_kern_otucs.h (HuOtucsRow).
//
//   k_sum_colbits    the profile's column map as one bit per consensus column, from the resident p2cs
//   k_sum_identity   per read the integers behind alignIdentity / hmmIdentity (src/HmmUFOtu_main.cpp:218-239) over its region of its row
//   k_otucs_stage    the spans of the accepted rows of a batch from where they lie (pitch cs_len: no alignment) into the 16-byte aligned
//                    stage of k_otucs_count
//   k_otucs_add_tab  counts added to one OTU's part of the resident table (hu_otucs_add_counts)
#pragma once
#include "hu_common.h"

#define HU_SUM_THREADS 256
#define HU_SUM_WAVES (HU_SUM_THREADS / 64)

/* bits [(L + 31) / 32], zeroed by the caller: bit c is set when CS column c (0-based) is a match column, i.e. p2cs[k] == c + 1 for a
 * profile position k in [1, K] — cs2ProfileIdx[c + 1] != 0 of the reference (hu_tsv::cs_to_profile) */
__global__ __launch_bounds__(256) void k_sum_colbits(const int32_t* __restrict__ p2cs, int K, int L, uint32_t* __restrict__ bits) {
	const int k = blockIdx.x * 256 + threadIdx.x + 1;
	if(k > K) return;
	const int c = p2cs[k] - 1;
	if(c >= 0 && c < L) atomicOr(&bits[c >> 5], 1u << (c & 31));
}

/* One wave per read, HU_SUM_WAVES reads per workgroup.  Read r's region is the columns csStart - 1 .. csEnd - 1 of its row (both from the
 * batch's own record, wave-uniform); a lane takes every 64th column of it, one byte each: consecutive lanes read consecutive bytes, and
 * a region of an amplicon read is a handful of such rounds.  cls [256]: 1 for the bytes that are symbols (hu_sum_rule.h), else 0.
 * out[r] = {n_cols, n_sym, n_match, n_match_sym}; a read that is not HU_READ_OK, or has no region, gets four zeros and reads nothing.
 * The region is cut at the row's end (as the readers of an assignment file cut it at the string's), never below column 0. */
__global__ __launch_bounds__(HU_SUM_THREADS) void k_sum_identity(const char* __restrict__ rows, int L, const HuAlnDev* __restrict__ alns, int n,
		const unsigned char* __restrict__ cls, const uint32_t* __restrict__ bits, int4* __restrict__ out) {
	__shared__ unsigned char sCls[256];
	sCls[threadIdx.x] = cls[threadIdx.x];
	__syncthreads();
	const int lane = threadIdx.x & 63, r = blockIdx.x * HU_SUM_WAVES + (threadIdx.x >> 6);
	if(r >= n) return;
	const HuAlnDev a = alns[r];
	int nCols = 0, lo = 0, hi = -1;
	if(a.status == HU_READ_OK && a.csStart >= 1 && a.csEnd >= a.csStart) { nCols = a.csEnd - a.csStart + 1; lo = a.csStart - 1; hi = (a.csEnd < L ? a.csEnd : L) - 1; }
	const unsigned char* __restrict__ row = reinterpret_cast<const unsigned char*>(rows) + (size_t) r * L;
	int sym = 0, mat = 0, both = 0;
	for(int c = lo + lane; c <= hi; c += 64) {
		const int s = sCls[row[c]], m = (int)((bits[c >> 5] >> (c & 31)) & 1u);
		sym += s; mat += m; both += s & m;
	}
#pragma unroll
	for(int o = 32; o > 0; o >>= 1) { sym += __shfl_down(sym, o); mat += __shfl_down(mat, o); both += __shfl_down(both, o); }
	if(lane == 0) out[r] = make_int4(nCols, sym, mat, both);
}

/* One wave per staged row, HU_SUM_WAVES per workgroup: staged row i is row src[i] of the batch, its columns [c0, c1) go to
 * stage + off16 * 16, padded with '-' up to the next multiple of 16 bytes (c0 is a multiple of 16; c1 is one, or the row's length: the
 * padding stands past the row's end, where k_otucs_count counts nothing).  Bytes, because neither end of the source is aligned. */
__global__ __launch_bounds__(HU_SUM_THREADS) void k_otucs_stage(const char* __restrict__ rows, int L, const int32_t* __restrict__ src,
		const HuOtucsRow* __restrict__ meta, int n, unsigned char* __restrict__ stage) {
	const int lane = threadIdx.x & 63, i = blockIdx.x * HU_SUM_WAVES + (threadIdx.x >> 6);
	if(i >= n) return;
	const HuOtucsRow m = meta[i];
	const int len = m.c1 - m.c0, padded = (len + 15) / 16 * 16;
	const char* __restrict__ row = rows + (size_t) src[i] * L;
	unsigned char* __restrict__ dst = stage + (size_t) m.off16 * 16;
	for(int k = lane; k < padded; k += 64) dst[k] = (unsigned char)(k < len ? row[m.c0 + k] : '-');
}

__global__ __launch_bounds__(256) void k_otucs_add_tab(uint32_t* __restrict__ dst, const uint32_t* __restrict__ add, int n) {
	const int i = blockIdx.x * 256 + threadIdx.x;
	if(i < n) dst[i] += add[i];
}
