// The kernels of hmmufotu-amd-permanova --design.  A virtual column vc of a launch is the pair (slot, design column) =
// (vc / q, vc % q): the chunk's permutations times the q columns of the basis Q [n][q], flattened.  nvc = slots * q of them are real.
//
//   k_pmd_square       once per call: the uploaded distances become their squares in place (one rounded product each).
//   k_index_shuffle    a thread per slot of the chunk: writes the identity into its column of idx [n][cp] (cp = the chunk padded to whole
//                      workgroups of 64), then runs the stratified shuffle of permutation first + slot on that column (hu_pmd_shuffle, the
//                      code the host runs).  Sample-major, for the reason of k_label_shuffle: the threads of a wave touch consecutive
//                      entries at every step, and the staging loads of k_pmd_quad are coalesced.  With `observed` the identity alone.
//                      k_label_shuffle itself does not fit: its steps are positions, a stratum's steps go through `member`.
//   k_pmd_quad<NT, I>  the hot path, part [row block][slab][vc] = sum over the block's 64 rows i of V[i][vc] (D2 V)[i][vc] restricted to
//                      the slab's k, with V[k][vc] = Q[idx[k][slot(vc)]][col(vc)].  The geometry is k_pcoa_d2v's: a workgroup of four
//                      waves owns 64 rows, 16 NT virtual columns and one K slab (hu_pc_slabs, hu_pc_slab_len: functions of n alone), walks
//                      the slab in tiles of 32, stages the 64 x 32 tile of D2 and the gathered 32 x 16NT tile of V through registers into
//                      LDS and issues the next tile's loads before this tile's arithmetic.  Wave w owns rows 16 w .. 16 w + 15 and holds
//                      NT accumulator tiles of v_mfma_f64_16x16x4_f64 in the layout written down at the head of hu_kern_pcoa.h.  Epilogue:
//                      register r of a lane is row (l >> 4) + 4 r of the wave's 16; x = fma(acc[r], V[row][vc], x) for r ascending from +0,
//                      then through LDS the four lane groups ascending and the four waves ascending by plain adds.  Cells beyond n, beyond
//                      the slab or beyond nvc are staged as +0.  Grid (column blocks, row blocks, slabs).
//   k_pmd_finish       a thread per virtual column: s[vc] = the partials over the slabs ascending, then over the row blocks ascending.
//   k_pmd_terms        a thread per (slot, term): SS_t = -1/2 (sum of s over the term's columns, ascending).
// No atomics, no workgroup waits for another, indices are 64-bit: the bits of every s are a function of (n, D2, v) alone.
#pragma once
#include "hu_common.h"
#include "hu_permanova_design.h"

typedef double hu_pmd_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_pmd_square(double* __restrict__ d, int64_t cells) {
	for(int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t) gridDim.x * 256) { const double v = d[i]; d[i] = v * v; }
}

template<class I> __global__ void __launch_bounds__(HU_PMD_SLOT) k_index_shuffle(I* __restrict__ idx, const int32_t* __restrict__ member, const int32_t* __restrict__ start,
		int64_t S, int64_t n, int64_t cp, uint64_t first, uint64_t seed, int observed) {
	const int64_t slot = (int64_t) blockIdx.x * HU_PMD_SLOT + threadIdx.x;
	if(slot >= cp) return;
	I* g = idx + slot;
	for(int64_t i = 0; i < n; ++i) g[i * cp] = (I) i;
	if(!observed) hu_pmd_shuffle(seed, first + (uint64_t) slot, S, member, start, g, cp);
}

template<int NT, class I> __global__ void __launch_bounds__(256) k_pmd_quad(const double* __restrict__ D2, const double* __restrict__ Q, const I* __restrict__ idx,
		double* __restrict__ part, int64_t n, int64_t q, int64_t cp, int64_t nvc, int64_t vcPad, int64_t slabLen) {
	constexpr int MP = 16 * NT, NV = HU_PCOA_KT * MP / 256, RPT = 256 / MP;       /* RPT: rows of the V tile per pass of the 256 threads */
	__shared__ double sA[HU_PCOA_TILE][HU_PCOA_KT + 1];
	__shared__ double sV[HU_PCOA_KT][MP];
	__shared__ double red[16][MP];
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int64_t vc0 = (int64_t) blockIdx.x * MP, r0 = (int64_t) blockIdx.y * HU_PCOA_TILE, s = blockIdx.z, k0 = s * slabLen, k1 = min(n, k0 + slabLen);
	/* the column this thread stages: the same one in every pass, since MP divides 256 */
	const int64_t gvc = vc0 + tid % MP;
	const bool gReal = gvc < nvc;
	const int64_t gSlot = gReal ? gvc / q : 0, gCol = gReal ? gvc % q : 0;
	double ra[8], rv[NV];
	auto load = [&](int64_t kk) {
#pragma unroll
		for(int p = 0; p < 8; ++p) {
			const int e = p * 256 + tid;
			const int64_t gi = r0 + (e >> 5), gk = kk + (e & 31);
			ra[p] = gi < n && gk < k1 ? D2[gi * n + gk] : 0.0;
		}
#pragma unroll
		for(int p = 0; p < NV; ++p) {
			const int64_t gk = kk + p * RPT + tid / MP;
			rv[p] = gReal && gk < k1 ? Q[(int64_t) idx[gk * cp + gSlot] * q + gCol] : 0.0;
		}
	};
	hu_pmd_d4 acc[NT];
#pragma unroll
	for(int t = 0; t < NT; ++t) acc[t] = hu_pmd_d4{0.0, 0.0, 0.0, 0.0};
	if(k0 < k1) load(k0);
	for(int64_t kk = k0; kk < k1; kk += HU_PCOA_KT) {
#pragma unroll
		for(int p = 0; p < 8; ++p) { const int e = p * 256 + tid; sA[e >> 5][e & 31] = ra[p]; }
#pragma unroll
		for(int p = 0; p < NV; ++p) sV[p * RPT + tid / MP][tid % MP] = rv[p];
		__syncthreads();
		if(kk + HU_PCOA_KT < k1) load(kk + HU_PCOA_KT);
#pragma unroll
		for(int u = 0; u < HU_PCOA_KT / 4; ++u) {
			const double a = sA[16 * wave + (lane & 15)][4 * u + (lane >> 4)];
#pragma unroll
			for(int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sV[4 * u + (lane >> 4)][16 * t + (lane & 15)], acc[t], 0, 0, 0);
		}
		__syncthreads();
	}
	/* the epilogue: the block's own rows of V, gathered as above */
#pragma unroll
	for(int t = 0; t < NT; ++t) {
		const int64_t vc = vc0 + 16 * t + (lane & 15);
		const bool real = vc < nvc;
		const int64_t slot = real ? vc / q : 0, col = real ? vc % q : 0;
		double x = 0.0;
#pragma unroll
		for(int r = 0; r < 4; ++r) {
			const int64_t row = r0 + 16 * wave + (lane >> 4) + 4 * r;
			const double v = real && row < n ? Q[(int64_t) idx[row * cp + slot] * q + col] : 0.0;
			x = fma(acc[t][r], v, x);
		}
		red[4 * wave + (lane >> 4)][16 * t + (lane & 15)] = x;
	}
	__syncthreads();
	if(tid < MP) {
		double tot = 0.0;
#pragma unroll
		for(int w = 0; w < 4; ++w) {
			const double y = ((red[4 * w][tid] + red[4 * w + 1][tid]) + red[4 * w + 2][tid]) + red[4 * w + 3][tid];
			tot = w == 0 ? y : tot + y;
		}
		part[((int64_t) blockIdx.y * gridDim.z + s) * vcPad + vc0 + tid] = tot;
	}
}

/* grid ceil(vcs / 256): vcs the virtual columns of the launch padded to whole column blocks */
__global__ void __launch_bounds__(256) k_pmd_finish(const double* __restrict__ part, double* __restrict__ sOut, int64_t rowBlocks, int64_t slabs, int64_t vcPad, int64_t vcs) {
	const int64_t vc = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(vc >= vcs) return;
	double tot = 0.0;
	for(int64_t b = 0; b < rowBlocks; ++b) {
		double x = 0.0;
		for(int64_t s = 0; s < slabs; ++s) x += part[(b * slabs + s) * vcPad + vc];
		tot += x;
	}
	sOut[vc] = tot;
}

/* grid ceil(slots T / 256) */
__global__ void __launch_bounds__(256) k_pmd_terms(const double* __restrict__ sIn, const int64_t* __restrict__ termStart, double* __restrict__ ss, int64_t slots, int64_t T, int64_t q) {
	const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(e >= slots * T) return;
	const int64_t slot = e / T, t = e % T;
	double sum = 0.0;
	for(int64_t c = termStart[t]; c < termStart[t + 1]; ++c) sum += sIn[slot * q + c];
	ss[e] = -0.5 * sum;
}
