// The within-group sums of squares of every permutation of a chunk (hmmufotu-amd-permanova).
//
//   k_label_shuffle       (hu_kern_shuffle.h) the labelling of every permutation of the chunk as a column of lab [n][cp], 16-bit labels.
//   k_permanova_pairs     a workgroup of 256 threads owns one 64 x 64 tile (I <= J) of the matrix and 256 permutations, one per thread.
//                         The tile's squares go to LDS once (32 KB; cells with j <= i or beyond n are +0, so the loop needs no index
//                         test), the labels of the tile's 128 samples to LDS as [sample / 4][permutation] words of four labels: 16-bit
//                         labels (64 KB, a ds_read_b64 per lane for four samples), or 8-bit labels when a <= 256 (32 KB, a ds_read_b32,
//                         and two workgroups on a CU); consecutive lanes on consecutive words, while the four squares they meet are
//                         two broadcast ds_read_b128.  A thread keeps g_i and r_i of four rows in registers over
//                         the j loop, so one read of the labels serves sixteen terms and four sums that do not meet are in flight:
//                         r_i = fma(m, D2_ij, r_i) from +0 in ascending j with m = 1.0 where the labels match and +0.0 where not (one
//                         select of m's high word instead of a 64-bit select of D2), then s = fma(1 / n_g, r_i, s) over ascending i,
//                         and writes s to part [tile][cp].  fma(1, D2, r) is the rounded r + D2 and fma(+0, D2, r) is r for the finite
//                         D2 >= 0 and r >= 0 here, so the bits are those of plain adds over the matching pairs alone.  On a diagonal tile the j loop of rows 4 q .. 4 q + 3 starts at word q.
//   k_permanova_finish    a thread per slot adds its tile sums in ascending tile order by plain adds and writes SS_W; the host compares
//                         it with the observed SS_W, which came out of the same kernels.
// No atomics, no workgroup waits for another: a result is a function of (matrix, labels, seed, p).  Indices are 64-bit.
#pragma once
#include "hu_common.h"
#include "hu_permanova.h"
#include "hu_kern_shuffle.h"

/* the LDS of k_permanova_pairs<BITS>: 98,304 bytes with 16-bit labels (one workgroup per CU), 65,536 with 8-bit labels (two) */
#define HU_PM_LDS(BITS) (HU_PM_TILE * HU_PM_TILE * 8 + 2 * (HU_PM_TILE / 4) * HU_PM_WG * (BITS) / 2)
template<int BITS> struct HuPmWord;
template<> struct HuPmWord<16> { typedef uint64_t type; };
template<> struct HuPmWord<8> { typedef uint32_t type; };

/* 1.0 or +0.0 from one select of the high word: fma(1, d, r) is the rounded r + d, fma(+0, d, r) is r for the finite d >= 0 and r >= 0 here */
__device__ __forceinline__ double hu_pm_one_if(bool c) { return __hiloint2double(c ? 0x3ff00000 : 0, 0); }

/* grid (tiles, cp / 256); dynamic LDS HU_PM_LDS(BITS); BITS 8 needs a <= 256 */
template<int BITS> __global__ void __launch_bounds__(HU_PM_WG) k_permanova_pairs(const double* __restrict__ dist, const uint16_t* __restrict__ lab, const double* __restrict__ inv,
		double* __restrict__ part, int64_t n, int64_t cp) {
	extern __shared__ __attribute__((aligned(16))) unsigned char pmLds[];
	double (*sD)[HU_PM_TILE] = (double (*)[HU_PM_TILE]) pmLds;
	typedef typename HuPmWord<BITS>::type W;
	const uint32_t mask = (1u << BITS) - 1;
	W (*sL)[HU_PM_WG] = (W (*)[HU_PM_WG])(pmLds + HU_PM_TILE * HU_PM_TILE * 8);     /* rows 0..15: the I side, 16..31: the J side */
	const int tid = threadIdx.x;
	const int nt = (int)((n + HU_PM_TILE - 1) / HU_PM_TILE);
	int t = blockIdx.x, iblk = 0;
	while(t >= nt - iblk) { t -= nt - iblk; ++iblk; }
	const int jblk = iblk + t;
	const int64_t i0 = (int64_t) iblk * HU_PM_TILE, j0 = (int64_t) jblk * HU_PM_TILE;
	{	/* the squares: thread -> row tid >> 2, columns 16 (tid & 3) .. + 15; only the upper triangle is read */
		const int row = tid >> 2, c0 = (tid & 3) * 16;
		const int64_t gi = i0 + row;
#pragma unroll
		for(int c = 0; c < 16; ++c) {
			const int64_t gj = j0 + c0 + c;
			double v = 0.0;
			if(gi < n && gj < n && gj > gi) { const double d = dist[gi * n + gj]; v = d * d; }
			sD[row][c0 + c] = v;
		}
	}
	const int64_t slot = (int64_t) blockIdx.y * HU_PM_WG + tid;                    /* < cp: the grid covers cp exactly */
	{	/* the labels: samples beyond n take the last sample's label, which meets squares of +0 only */
#pragma unroll 4
		for(int q = 0; q < 2 * (HU_PM_TILE / 4); ++q) {
			const int64_t s0 = (q < HU_PM_TILE / 4 ? i0 : j0 - HU_PM_TILE) + 4 * q;
			W w = 0;
#pragma unroll
			for(int k = 0; k < 4; ++k) {
				const int64_t s = min(s0 + k, n - 1);
				w |= (W) lab[s * cp + slot] << (BITS * k);
			}
			sL[q][tid] = w;
		}
	}
	__syncthreads();
	const int jqFirst = iblk == jblk ? 1 : 0;                                     /* a diagonal tile: the rows of word iq meet nothing before word iq */
	double s = 0.0;
	for(int iq = 0; iq < HU_PM_TILE / 4; ++iq) {
		const W gi4 = sL[iq][tid];
		const uint32_t gi[4] = {(uint32_t) gi4 & mask, (uint32_t)(gi4 >> BITS) & mask, (uint32_t)(gi4 >> (2 * BITS)) & mask, (uint32_t)(gi4 >> (3 * BITS))};
		double r[4] = {0.0, 0.0, 0.0, 0.0};                                         /* four rows at a time: four sums that do not meet */
#pragma unroll 2
		for(int jq = jqFirst * iq; jq < HU_PM_TILE / 4; ++jq) {
			const W gj4 = sL[HU_PM_TILE / 4 + jq][tid];
			const uint32_t g0 = (uint32_t) gj4 & mask, g1 = (uint32_t)(gj4 >> BITS) & mask, g2 = (uint32_t)(gj4 >> (2 * BITS)) & mask, g3 = (uint32_t)(gj4 >> (3 * BITS));
#pragma unroll
			for(int k = 0; k < 4; ++k) {
				const double2 d01 = *(const double2*) &sD[4 * iq + k][4 * jq], d23 = *(const double2*) &sD[4 * iq + k][4 * jq + 2];
				r[k] = fma(hu_pm_one_if(g0 == gi[k]), d01.x, r[k]);
				r[k] = fma(hu_pm_one_if(g1 == gi[k]), d01.y, r[k]);
				r[k] = fma(hu_pm_one_if(g2 == gi[k]), d23.x, r[k]);
				r[k] = fma(hu_pm_one_if(g3 == gi[k]), d23.y, r[k]);
			}
		}
#pragma unroll
		for(int k = 0; k < 4; ++k) s = fma(inv[gi[k]], r[k], s);
	}
	part[(int64_t) blockIdx.x * cp + slot] = s;
}

__global__ void __launch_bounds__(256) k_permanova_finish(const double* __restrict__ part, double* __restrict__ ssw, int64_t tiles, int64_t cp) {
	const int64_t slot = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(slot >= cp) return;
	double tot = 0.0;
	for(int64_t t = 0; t < tiles; ++t) tot += part[t * cp + slot];
	ssw[slot] = tot;
}
