// The kernels of hmmufotu-amd-pcoa.  A block is n x MP doubles, row-major, MP = 16 NT the block's width padded to whole
// accumulator tiles (NT = 1 .. 4), the columns from m on zero.
//
//   k_pcoa_square      once per call: the uploaded distances become their squares in place (one rounded product each).
//   k_pcoa_d2v<NT>     the hot path, part [S][n][MP] = D2 V by K slabs.  A workgroup of four waves owns 64 rows of D2, all MP columns and
//                      slab blockIdx.y of K (hu_pc_slabs, hu_pc_slab_len: functions of n alone).  It walks its slab in tiles of 32: the
//                      64 x 32 tile of D2 and the 32 x MP slab of V go from registers to LDS, the next tile's loads are issued before the
//                      arithmetic of this one.  Wave w owns rows 16 w .. 16 w + 15 and holds NT accumulator tiles of
//                      v_mfma_f64_16x16x4_f64: operand A of lane l is D2 [row l & 15][k l >> 4], operand B is V [k l >> 4][column l & 15],
//                      the result of register r is C [row (l >> 4) + 4 r][column l & 15].  Cells beyond n or beyond the slab are staged
//                      as +0, so the arithmetic needs no index test.
//   k_pcoa_colsum      the column sums of sum_s part [s], in partials of 256 rows: four runs of 64 rows by plain adds in ascending order,
//                      the four runs then in ascending order.
//   k_pcoa_finish      W = scale * (sum_s part [s] - mean), the slabs added in ascending order by plain adds, the mean of a column its
//                      partial sums in ascending order divided by n.  With scale -1/2 this is B V of a centred V; with one slab and scale 1
//                      it centres a block.
//   k_pcoa_gram<NT>    gpart [chunk][MP][MP] = X'Y over the chunk's 256 rows in ascending order by fma; k_pcoa_gram_sum adds the chunks in
//                      ascending order.
//   k_pcoa_apply<NT, TWO>  out = X M1 (+ Y M2 with TWO) for small M1, M2 [MP][MP] read from LDS (one matrix's worth without TWO), a thread per entry, by fma over ascending index.
// No atomics, no workgroup waits for another: the bits of every result are a function of (n, MP, the inputs) alone.  Indices are 64-bit.
#pragma once
#include "hu_common.h"
#include "hu_pcoa.h"

typedef double hu_pc_d4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) k_pcoa_square(double* __restrict__ d, int64_t cells) {
	for(int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < cells; i += (int64_t) gridDim.x * 256) { const double v = d[i]; d[i] = v * v; }
}

/* grid (ceil(n / 64), S) */
template<int NT> __global__ void __launch_bounds__(256) k_pcoa_d2v(const double* __restrict__ D2, const double* __restrict__ V, double* __restrict__ part,
		int64_t n, int64_t slabLen) {
	constexpr int MP = 16 * NT, NV = HU_PCOA_KT * MP / 256;
	__shared__ double sA[HU_PCOA_TILE][HU_PCOA_KT + 1];
	__shared__ double sV[HU_PCOA_KT][MP];
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int64_t r0 = (int64_t) blockIdx.x * HU_PCOA_TILE, s = blockIdx.y, k0 = s * slabLen, k1 = min(n, k0 + slabLen);
	double ra[8], rv[NV];
	auto load = [&](int64_t kk) {
#pragma unroll
		for(int p = 0; p < 8; ++p) {
			const int idx = p * 256 + tid;
			const int64_t gi = r0 + (idx >> 5), gk = kk + (idx & 31);
			ra[p] = gi < n && gk < k1 ? D2[gi * n + gk] : 0.0;
		}
#pragma unroll
		for(int p = 0; p < NV; ++p) {
			const int idx = p * 256 + tid;
			const int64_t gk = kk + idx / MP;
			rv[p] = gk < k1 ? V[gk * MP + idx % MP] : 0.0;
		}
	};
	hu_pc_d4 acc[NT];
#pragma unroll
	for(int t = 0; t < NT; ++t) acc[t] = hu_pc_d4{0.0, 0.0, 0.0, 0.0};
	if(k0 < k1) load(k0);
	for(int64_t kk = k0; kk < k1; kk += HU_PCOA_KT) {
#pragma unroll
		for(int p = 0; p < 8; ++p) { const int idx = p * 256 + tid; sA[idx >> 5][idx & 31] = ra[p]; }
#pragma unroll
		for(int p = 0; p < NV; ++p) { const int idx = p * 256 + tid; sV[idx / MP][idx % MP] = rv[p]; }
		__syncthreads();
		if(kk + HU_PCOA_KT < k1) load(kk + HU_PCOA_KT);
#pragma unroll
		for(int q = 0; q < HU_PCOA_KT / 4; ++q) {
			const double a = sA[16 * wave + (lane & 15)][4 * q + (lane >> 4)];
#pragma unroll
			for(int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sV[4 * q + (lane >> 4)][16 * t + (lane & 15)], acc[t], 0, 0, 0);
		}
		__syncthreads();
	}
#pragma unroll
	for(int t = 0; t < NT; ++t)
#pragma unroll
		for(int r = 0; r < 4; ++r) {
			const int64_t row = r0 + 16 * wave + (lane >> 4) + 4 * r;
			if(row < n) part[(s * n + row) * MP + 16 * t + (lane & 15)] = acc[t][r];
		}
}

/* grid ceil(n / 256) */
__global__ void __launch_bounds__(256) k_pcoa_colsum(const double* __restrict__ part, int64_t S, int64_t n, int mp, double* __restrict__ colpart) {
	__shared__ double red[4][64];
	const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
	const int64_t i0 = (int64_t) blockIdx.x * HU_PCOA_CHUNK + 64 * q, i1 = min(n, i0 + 64);
	double sum = 0.0;
	if(c < mp) for(int64_t i = i0; i < i1; ++i) {
		double x = 0.0;
		for(int64_t s = 0; s < S; ++s) x += part[(s * n + i) * mp + c];
		sum += x;
	}
	red[q][c] = sum;
	__syncthreads();
	if(q == 0 && c < mp) colpart[(int64_t) blockIdx.x * mp + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

/* grid ceil(n mp / 256) */
__global__ void __launch_bounds__(256) k_pcoa_finish(const double* __restrict__ part, int64_t S, int64_t n, int mp, const double* __restrict__ colpart, int64_t chunks,
		double scale, double* __restrict__ W) {
	__shared__ double mean[HU_PCOA_MAX_MP];
	if((int) threadIdx.x < mp) {
		double sum = 0.0;
		for(int64_t ch = 0; ch < chunks; ++ch) sum += colpart[ch * mp + threadIdx.x];
		mean[threadIdx.x] = sum / (double) n;
	}
	__syncthreads();
	const int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(idx >= n * mp) return;
	double x = 0.0;
	for(int64_t s = 0; s < S; ++s) x += part[s * n * mp + idx];
	W[idx] = scale * (x - mean[idx % mp]);
}

/* grid ceil(n / 256) */
template<int NT> __global__ void __launch_bounds__(256) k_pcoa_gram(const double* __restrict__ X, const double* __restrict__ Y, int64_t n, double* __restrict__ gpart) {
	constexpr int MP = 16 * NT, NV = 32 * MP / 256;
	__shared__ double sX[32][MP], sY[32][MP];
	const int tid = threadIdx.x, ta = tid >> 4, tb = tid & 15;
	const int64_t i0 = (int64_t) blockIdx.x * HU_PCOA_CHUNK;
	double acc[NT][NT];
#pragma unroll
	for(int i = 0; i < NT; ++i)
#pragma unroll
		for(int j = 0; j < NT; ++j) acc[i][j] = 0.0;
	for(int64_t rb = i0; rb < min(n, i0 + HU_PCOA_CHUNK); rb += 32) {
#pragma unroll
		for(int p = 0; p < NV; ++p) {
			const int idx = p * 256 + tid;
			const int64_t row = rb + idx / MP;
			sX[idx / MP][idx % MP] = row < n ? X[row * MP + idx % MP] : 0.0;
			sY[idx / MP][idx % MP] = row < n ? Y[row * MP + idx % MP] : 0.0;
		}
		__syncthreads();
		for(int r = 0; r < 32; ++r) {
			double xa[NT], yb[NT];
#pragma unroll
			for(int i = 0; i < NT; ++i) { xa[i] = sX[r][ta + 16 * i]; yb[i] = sY[r][tb + 16 * i]; }
#pragma unroll
			for(int i = 0; i < NT; ++i)
#pragma unroll
				for(int j = 0; j < NT; ++j) acc[i][j] = fma(xa[i], yb[j], acc[i][j]);
		}
		__syncthreads();
	}
#pragma unroll
	for(int i = 0; i < NT; ++i)
#pragma unroll
		for(int j = 0; j < NT; ++j) gpart[(int64_t) blockIdx.x * MP * MP + (ta + 16 * i) * MP + tb + 16 * j] = acc[i][j];
}

/* grid ceil(cells / 256), cells = mp mp */
__global__ void __launch_bounds__(256) k_pcoa_gram_sum(const double* __restrict__ gpart, int64_t chunks, int cells, double* __restrict__ G) {
	const int e = blockIdx.x * 256 + threadIdx.x;
	if(e >= cells) return;
	double sum = 0.0;
	for(int64_t ch = 0; ch < chunks; ++ch) sum += gpart[ch * cells + e];
	G[e] = sum;
}

/* grid ceil(n MP / 256); TWO: out = X M1 + Y M2, otherwise out = X M1 and Y, M2 are not read; out is neither X nor Y */
template<int NT, bool TWO> __global__ void __launch_bounds__(256) k_pcoa_apply(const double* __restrict__ X, const double* __restrict__ M1, const double* __restrict__ Y,
		const double* __restrict__ M2, double* __restrict__ out, int64_t n) {
	constexpr int MP = 16 * NT;
	__shared__ double sM[TWO ? 2 : 1][MP * MP];
	for(int e = threadIdx.x; e < MP * MP; e += 256) { sM[0][e] = M1[e]; if constexpr(TWO) sM[1][e] = M2[e]; }
	__syncthreads();
	const int64_t idx = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(idx >= n * MP) return;
	const int64_t row = idx / MP;
	const int c = (int)(idx % MP);
	double s = 0.0;
#pragma unroll 8
	for(int a = 0; a < MP; ++a) s = fma(X[row * MP + a], sM[0][a * MP + c], s);
	if constexpr(TWO) {
#pragma unroll 8
		for(int a = 0; a < MP; ++a) s = fma(Y[row * MP + a], sM[1][a * MP + c], s);
	}
	out[idx] = s;
}
