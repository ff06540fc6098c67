// The rank statistic of every tested OTU under every permutation of a chunk (hmmufotu-amd-diffabund).
//
//   k_label_shuffle  (hu_kern_shuffle.h) the labelling of every permutation of the chunk as a column of lab [n][cp], byte labels: the
//                  64 lanes of a wave hold 64 permutations and touch 64 consecutive bytes.
//   k_da_sums      a workgroup of 256 threads takes HU_DA_BLOCK tested OTUs (blockIdx.x, table order) and 256 permutations (blockIdx.y),
//                  one per thread.  A row's cells (sample << 16 | e_j - e_z) are staged in LDS, HU_DA_STAGE at a time and padded with
//                  cells of 0 to a multiple of eight, and read back as two broadcast ds_read_b128; a cell is then one byte load of the
//                  label, coalesced across the lanes, and one integer add into D_g.  TWO (a == 2): one register, D_1 += g d, and
//                  D_0 = the row's sum - D_1.  Otherwise (3 <= a <= 64): acc [a][256] words of dynamic LDS, thread t on column t, so the
//                  lanes of a wave are on distinct banks whatever their labels; the add is a ds_add_u32 without return.  At the end of a
//                  row: C_g = n_g e_z + D_g, the 128-bit T (hu_da_T_add), T >= the observed T counted by a ballot and one integer
//                  atomic add per wave into count [row], H (hu_da_H), and the running maximum of the thread's permutation, written
//                  once per workgroup to partmax [block][cp].  With `observed` slot 0 writes T and H of the row and nothing is counted.
//   k_da_finish    a thread per slot takes the maximum over the blocks.
// Integer atomics alone, no workgroup waits for another: a result is a function of (cells, labels, seed, p).  Indices are 64-bit.
// Bounds: a row r < m reads cell [ptr[r], ptr[r + 1]), the plan's; a cell's sample is below n by construction (hu_da_plan), and
// slot < cp because the grid covers cp exactly; a label is below a because the shuffle moves the checked labels.
#pragma once
#include "hu_common.h"
#include "hu_diffabund.h"
#include "hu_kern_shuffle.h"

struct HuDaDev {
	const uint32_t* cell; const int64_t* ptr; const int32_t* ez; const int32_t* dsum; const double* tc;   /* the rows */
	const int64_t* size; const uint64_t* w;                                                               /* [a] n_g and L / n_g */
	const uint8_t* lab;                                                                                   /* [n][cp] */
	uint64_t* tobs; double* hobs; uint32_t* count;                                                        /* [m][2], [m], [m] */
	double* partmax;                                                                                      /* [blocks][cp] */
	int64_t m, cp, cnt;                                                                                   /* cnt: the slots of the chunk that are permutations */
	double dL, c2;
	int a, observed;
};

/* grid (blocks, cp / 256); dynamic LDS: TWO 0, else a * 1024 bytes */
template<bool TWO> __global__ void __launch_bounds__(HU_DA_WG) k_da_sums(const HuDaDev d) {
	__shared__ __attribute__((aligned(16))) uint32_t sCell[HU_DA_STAGE];
	extern __shared__ __attribute__((aligned(16))) uint32_t daAcc[];              /* [a][256] */
	const int tid = threadIdx.x;
	const int64_t slot = (int64_t) blockIdx.y * HU_DA_WG + tid;                   /* < cp: the grid covers cp exactly */
	const uint8_t* __restrict__ myLab = d.lab + slot;
	const int64_t cp = d.cp;
	const int64_t r0 = (int64_t) blockIdx.x * HU_DA_BLOCK, r1 = min(d.m, r0 + HU_DA_BLOCK);
	if(!TWO) for(int g = 0; g < d.a; ++g) daAcc[g * HU_DA_WG + tid] = 0;          /* a thread's own column: nobody else touches it */
	double mx = 0.0;
	for(int64_t r = r0; r < r1; ++r) {
		const int64_t b = d.ptr[r], e = d.ptr[r + 1];
		uint32_t d1 = 0;
		for(int64_t s = b; s < e; s += HU_DA_STAGE) {
			const int len = (int) min((int64_t) HU_DA_STAGE, e - s), len8 = (len + 7) & ~7;
			__syncthreads();                                                          /* the readers of the piece before are done */
			for(int i = tid; i < len8; i += HU_DA_WG) sCell[i] = i < len ? d.cell[s + i] : 0u;
			__syncthreads();
			for(int i = 0; i < len8; i += 8) {
				const uint4 c0 = *(const uint4*) &sCell[i], c1 = *(const uint4*) &sCell[i + 4];
				const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
				uint32_t g[8];
#pragma unroll
				for(int k = 0; k < 8; ++k) g[k] = myLab[(int64_t)(c[k] >> 16) * cp];
#pragma unroll
				for(int k = 0; k < 8; ++k) {
					if(TWO) d1 += g[k] * (c[k] & 0xffffu);
					else atomicAdd(&daAcc[g[k] * HU_DA_WG + tid], c[k] & 0xffffu);
				}
			}
		}
		const int64_t z = d.ez[r];
		uint64_t hi = 0, lo = 0;
		if(TWO) {
			hu_da_T_add(hi, lo, d.size[0] * z + (int64_t)(d.dsum[r] - (int32_t) d1), d.w[0]);
			hu_da_T_add(hi, lo, d.size[1] * z + (int64_t) d1, d.w[1]);
		} else {
			for(int g = 0; g < d.a; ++g) {
				const int64_t D = daAcc[g * HU_DA_WG + tid];
				daAcc[g * HU_DA_WG + tid] = 0;
				hu_da_T_add(hi, lo, d.size[g] * z + D, d.w[g]);
			}
		}
		const double H = hu_da_H(hi, lo, d.dL, d.c2, d.tc[r]);
		if(d.observed) {
			if(slot == 0) { d.tobs[2 * r] = hi; d.tobs[2 * r + 1] = lo; d.hobs[r] = H; }
		} else {
			const bool ge = slot < d.cnt && hu_da_T_ge(hi, lo, d.tobs[2 * r], d.tobs[2 * r + 1]);
			const unsigned long long bal = __ballot(ge);
			if((tid & 63) == 0 && bal) atomicAdd(&d.count[r], (uint32_t) __popcll(bal));
		}
		mx = H > mx ? H : mx;
	}
	d.partmax[(int64_t) blockIdx.x * cp + slot] = mx;
}

__global__ void __launch_bounds__(256) k_da_finish(const double* __restrict__ partmax, double* __restrict__ mx, int64_t blocks, int64_t cp) {
	const int64_t slot = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(slot >= cp) return;
	double v = 0.0;
	for(int64_t b = 0; b < blocks; ++b) { const double x = partmax[b * cp + slot]; v = x > v ? x : v; }
	mx[slot] = v;
}
