// The counts behind hmmufotu-train-sm on the device: per training item the 4 x 4 transition counts of
// DNASubModel::calcTransFreq3Seq / calcTransFreq2Seq (src/DNASubModel.cpp:75-104, :52-62) and the (d, N) of the two SeqUtils::pDist
// calls that decide whether the item is used (src/SeqUtils.cpp:37-54, src/PhyloTreeUnrooted.cpp:449-486); per row the base counts of
// DNASubModel::calcBaseFreq (:106-112).  All integers: the sums are exact in any order.
//
// rows [nRows][stride16] pieces of 16 bytes: the encoded rows (0..3 residue, negative: gap or invalid), each padded to a multiple of
// 16 columns with the gap code, so a lane reads whole pieces and the tail needs no branch.  One workgroup of 256 lanes per item, then
// one per row: workgroup b < nItems counts item b, workgroup nItems + r counts row r.  A lane takes the pieces lane, lane + 256, ...
// of the item's rows.  The 16 counters of a piece live in four words of four 8-bit fields (a piece adds at most 3 x 16 = 48 to a
// field): the word is chosen by compare-and-add on `from`, the field by a shift on `to`, never an array indexed by a code: no scratch.
// They are spread into 32-bit counters after every piece, reduced over the wave with __shfl_xor, over the four waves through LDS, and lane t < 20 writes value t.
#pragma once
#include "hu_common.h"

#define HU_SM_BLOCK 256
#define HU_SM_VALUES 20     /* counts [16], then d, N of (row0, row1) and d, N of (row0, row2) */

struct HuSmAcc {
	uint32_t f[4];       /* the piece at hand: f[from] holds four 8-bit fields, one per `to`; only ever indexed by unrolled constants */
	int32_t c[16];       /* likewise */
	int32_t d1, n1, d2, n2;
};

#define HU_SM_HIGH 0x80808080u     /* the sign bit of each of a word's four codes */
/* bit 7 of every byte of x that is not zero */
__device__ __forceinline__ uint32_t sm_nonzero(uint32_t x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & HU_SM_HIGH; }
/* v, four fields `to`, into the counters of row `from` (0..3) */
__device__ __forceinline__ void sm_add(HuSmAcc& a, uint32_t from, uint32_t v) {
	#pragma unroll
	for(uint32_t r = 0; r < 4; ++r) a.f[r] += from == r ? v : 0u;
}
__device__ __forceinline__ void sm_spread(HuSmAcc& a) {
	#pragma unroll
	for(int r = 0; r < 4; ++r) {
		#pragma unroll
		for(int k = 0; k < 4; ++k) a.c[4 * r + k] += (int32_t)((a.f[r] >> (8 * k)) & 255u);
		a.f[r] = 0;
	}
}

/* four columns of a triple (src/DNASubModel.cpp:82-102) or of a pair (:58-60), and of the two distances: one word of each row.  The
 * tests on the codes are made for the four bytes at once; only the additions into the fields go column by column. */
template<bool PAIR> __device__ __forceinline__ void sm_word(HuSmAcc& a, uint32_t w0, uint32_t w1, uint32_t w2) {
	const uint32_t v1 = ~(w0 | w1) & HU_SM_HIGH, v2 = ~(w0 | w2) & HU_SM_HIGH;     /* both codes non-negative */
	const uint32_t x01 = sm_nonzero(w0 ^ w1), x02 = sm_nonzero(w0 ^ w2);
	a.n1 += __popc(v1); a.d1 += __popc(v1 & x01);
	a.n2 += __popc(v2); a.d2 += __popc(v2 & x02);
	if(PAIR) {
		const uint32_t ok = ~(w1 | w2) & HU_SM_HIGH;
		#pragma unroll
		for(int i = 0; i < 4; ++i) sm_add(a, (w1 >> (8 * i)) & 3u, ((ok >> (8 * i + 7)) & 1u) << (((w2 >> (8 * i)) & 3u) * 8));
	}
	else {
		const uint32_t x12 = sm_nonzero(w1 ^ w2);
		const uint32_t ok = ~(w0 | w1 | w2) & HU_SM_HIGH & ~(x01 & x02 & x12);     /* all three differ: no ancestor to guess */
		const uint32_t useB1 = ((x01 & x02) >> 7) * 255u;                            /* whole bytes where b0 matches neither: the ancestor is b1 (== b2) */
		const uint32_t anc = (w0 & ~useB1) | (w1 & useB1);
		#pragma unroll
		for(int i = 0; i < 4; ++i) {
			const uint32_t g = (ok >> (8 * i + 7)) & 1u;
			const uint32_t v = (g << (((w0 >> (8 * i)) & 3u) * 8)) + (g << (((w1 >> (8 * i)) & 3u) * 8)) + (g << (((w2 >> (8 * i)) & 3u) * 8));
			sm_add(a, (anc >> (8 * i)) & 3u, v);
		}
	}
}
template<bool PAIR> __device__ __forceinline__ void sm_piece(HuSmAcc& a, const uint4 p0, const uint4 p1, const uint4 p2) {
	sm_word<PAIR>(a, p0.x, p1.x, p2.x); sm_word<PAIR>(a, p0.y, p1.y, p2.y); sm_word<PAIR>(a, p0.z, p1.z, p2.z); sm_word<PAIR>(a, p0.w, p1.w, p2.w);
	sm_spread(a);
}
/* four columns of one row: its base counts, in the fields of f[0] */
__device__ __forceinline__ void sm_base_word(HuSmAcc& a, uint32_t w) {
	const uint32_t ok = ~w & HU_SM_HIGH;
	#pragma unroll
	for(int i = 0; i < 4; ++i) a.f[0] += ((ok >> (8 * i + 7)) & 1u) << (((w >> (8 * i)) & 3u) * 8);
}

/* items [nItems][3] rows (row0, row1, row2), row0 = -1 for a pair, all checked against nRows by the host.
 * outItems [nItems][20], outBase [nRows][4].  grid nItems + nRows, block 256. */
__global__ __launch_bounds__(HU_SM_BLOCK, 4) void k_sm_counts(const uint4* __restrict__ rows, int64_t nRows, int64_t stride16, const int32_t* __restrict__ items,
		int64_t nItems, int32_t* __restrict__ outItems, int32_t* __restrict__ outBase) {
	__shared__ int32_t part[HU_SM_BLOCK / 64][HU_SM_VALUES];
	const int64_t b = blockIdx.x;
	const bool isItem = b < nItems;
	HuSmAcc a;
	a.f[0] = a.f[1] = a.f[2] = a.f[3] = 0; a.d1 = a.n1 = a.d2 = a.n2 = 0;
	#pragma unroll
	for(int k = 0; k < 16; ++k) a.c[k] = 0;
	if(isItem) {
		const int32_t i0 = items[b * 3], i1 = items[b * 3 + 1], i2 = items[b * 3 + 2];
		const bool pair = i0 < 0;
		/* a pair's distances are those of (row1, row1) and (row1, row2): the Goldman test compares the first row with itself */
		const uint4* r0 = rows + (int64_t)(pair ? i1 : i0) * stride16;
		const uint4* r1 = rows + (int64_t) i1 * stride16;
		const uint4* r2 = rows + (int64_t) i2 * stride16;
		/* one piece per trip: unrolled or interleaved, the sixteen columns of two pieces at once do not fit the registers of four waves per SIMD */
		if(pair) {
			#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
			for(int64_t q = threadIdx.x; q < stride16; q += HU_SM_BLOCK) sm_piece<true>(a, r0[q], r1[q], r2[q]);
		}
		else {
			#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
			for(int64_t q = threadIdx.x; q < stride16; q += HU_SM_BLOCK) sm_piece<false>(a, r0[q], r1[q], r2[q]);
		}
	}
	else { /* the base counts of one row: counters 0..3 */
		const uint4* r = rows + (b - nItems) * stride16;
		#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
		for(int64_t q = threadIdx.x; q < stride16; q += HU_SM_BLOCK) {
			const uint4 p = r[q];
			sm_base_word(a, p.x); sm_base_word(a, p.y); sm_base_word(a, p.z); sm_base_word(a, p.w);
			sm_spread(a);
		}
	}
	#pragma unroll
	for(int k = 0; k < 16; ++k) { for(int m = 32; m > 0; m >>= 1) a.c[k] += __shfl_xor(a.c[k], m); }
	for(int m = 32; m > 0; m >>= 1) { a.d1 += __shfl_xor(a.d1, m); a.n1 += __shfl_xor(a.n1, m); a.d2 += __shfl_xor(a.d2, m); a.n2 += __shfl_xor(a.n2, m); }
	const int wave = threadIdx.x >> 6;
	if((threadIdx.x & 63) == 0) {
		#pragma unroll
		for(int k = 0; k < 16; ++k) part[wave][k] = a.c[k];
		part[wave][16] = a.d1; part[wave][17] = a.n1; part[wave][18] = a.d2; part[wave][19] = a.n2;
	}
	__syncthreads();
	const int t = threadIdx.x;
	if(t < (isItem ? HU_SM_VALUES : 4)) {
		int32_t s = 0;
		#pragma unroll
		for(int w = 0; w < HU_SM_BLOCK / 64; ++w) s += part[w][t];
		if(isItem) outItems[b * HU_SM_VALUES + t] = s; else outBase[(b - nItems) * 4 + t] = s;
	}
}
