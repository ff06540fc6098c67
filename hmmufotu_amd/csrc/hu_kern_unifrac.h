// The distances between the samples of an OTU table on the database's tree (hmmufotu-amd-unifrac).
//
// Embedding.  The host (hu_unifrac_host.cpp) numbers the kept branches in depth-first order and sorts the table's rows by the same
// order, so that the rows below branch k are the interval [lo_k, hi_k).  C [M + 1][Sp] holds the rows in that order from row 1 on
// (row 0 is zero), Sp the samples padded to whole tiles with zero columns.
//   k_unifrac_scan_sums   a thread per (block of HU_UF_SCAN_ROWS rows, sample): the block's column sum, rows in ascending order
//   k_unifrac_scan_offs   a thread per sample: the exclusive scan of its block sums, in ascending order
//   k_unifrac_scan_rows   a thread per (block, sample): C[q + 1] = offset + the rows of the block up to q, in place
//   k_unifrac_gather      a thread per (branch, sample): P[k][j] = (C[hi_k][j] - C[lo_k][j]) / C[M][j]; the padding columns are 0
// Integer counts below 2^53 come out exact; every thread adds in an order that the table and the tree alone fix.
//
// Pairs.  k_unifrac_pairs<METHOD> is shaped like a tiled GEMM whose inner product is b |x - y| and b (x + y); FP64 on the vector ALU.
// A workgroup of 256 threads owns one 64 x 64 tile (iblk <= jblk) of the pair matrix and one slab of L consecutive branches.  It walks
// the slab in chunks of 32 branches: the two 32 x 64 panels of P and the 32 lengths go through registers into LDS (32.25 KB) while the
// chunk before is being added, and every thread keeps a 4 x 4 register tile of numerators and denominators.  A thread's samples are
// {2 t, 2 t + 1, 32 + 2 t, 33 + 2 t} on either side, so that the 16 lanes of a ds_read_b128 group read 256 contiguous bytes (no bank
// conflict) on the j side and broadcast on the i side.  Rows beyond the slab are staged as zeros with b = 0: fma(0, v, acc) == acc, so the
// bits are those of the sum over the slab's own branches in ascending order.  The partial sums of a (slab, tile) go to part[], and
//   k_unifrac_finish      a thread per pair of a tile adds the slabs in ascending order, divides, and writes d(i,j) and its copy d(j,i).
//   k_unifrac_pd          Faith's PD: a thread per (slab, sample), then the slabs in order in k_unifrac_pd_finish.
// No atomics anywhere: a result is a function of (table, tree, L).
#pragma once
#include "hu_common.h"
#include "hu_unifrac.h"

#define HU_UF_WG 256

static __global__ void __launch_bounds__(256) k_unifrac_scan_sums(const double* __restrict__ C, double* __restrict__ blkSum, int64_t M, int64_t Sp) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
	if(j >= Sp) return;
	const int64_t q0 = blk * HU_UF_SCAN_ROWS, q1 = min(M, q0 + (int64_t) HU_UF_SCAN_ROWS);
	double s = 0.0;
	for(int64_t q = q0; q < q1; ++q) s += C[(q + 1) * Sp + j];
	blkSum[blk * Sp + j] = s;
}

static __global__ void __launch_bounds__(256) k_unifrac_scan_offs(double* __restrict__ blkSum, int64_t nBlk, int64_t Sp) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= Sp) return;
	double off = 0.0;
	for(int64_t blk = 0; blk < nBlk; ++blk) { const double s = blkSum[blk * Sp + j]; blkSum[blk * Sp + j] = off; off += s; }
}

static __global__ void __launch_bounds__(256) k_unifrac_scan_rows(double* __restrict__ C, const double* __restrict__ blkOff, int64_t M, int64_t Sp) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
	if(j >= Sp) return;
	const int64_t q0 = blk * HU_UF_SCAN_ROWS, q1 = min(M, q0 + (int64_t) HU_UF_SCAN_ROWS);
	double run = blkOff[blk * Sp + j];
	for(int64_t q = q0; q < q1; ++q) { run += C[(q + 1) * Sp + j]; C[(q + 1) * Sp + j] = run; }
}

static __global__ void __launch_bounds__(256) k_unifrac_gather(const double* __restrict__ C, const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
		double* __restrict__ P, int64_t M, int64_t S, int64_t Sp, int64_t B) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
	if(j >= Sp || k >= B) return;
	double p = 0.0;
	if(j < S) p = (C[(int64_t) hi[k] * Sp + j] - C[(int64_t) lo[k] * Sp + j]) / C[M * Sp + j];
	P[k * Sp + j] = p;
}

template<int METHOD> __device__ __forceinline__ void hu_uf_term(double b, double x, double y, double alpha, double& num, double& den) {
	if(METHOD == HU_UF_UNWEIGHTED) { num = fma(b, fabs(x - y), num); den = fma(b, fmax(x, y), den); }      /* x, y are 0 or 1 here */
	else if(METHOD == HU_UF_WEIGHTED) { num = fma(b, fabs(x - y), num); den = fma(b, x + y, den); }
	else if(METHOD == HU_UF_WEIGHTED_RAW) num = fma(b, fabs(x - y), num);
	else {
		const double s = x + y;
		if(s > 0) {
			const double pw = alpha == 0.5 ? sqrt(s) : pow(s, alpha);
			num = fma(b * pw, fabs(x - y) / s, num); den = fma(b, pw, den);
		}
	}
}

/* one workgroup's tile (of nTile) and slab; part [slab][tile][2][64][64].  hu_kern_unifrac_rarefied.h calls it once per resident draw */
template<int METHOD> __device__ __forceinline__ void hu_uf_pairs_wg(const double* __restrict__ P, const double* __restrict__ blen,
		double* __restrict__ part, int64_t Sp, int64_t B, int64_t L, double alpha, const int tile, const int slab, const int nTile) {
	__shared__ __attribute__((aligned(16))) double sI[HU_UF_CHUNK][HU_UF_TILE], sJ[HU_UF_CHUNK][HU_UF_TILE];
	__shared__ double sB[HU_UF_CHUNK];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int nt = (int)(Sp / HU_UF_TILE);
	int t = tile, iblk = 0;
	while(t >= nt - iblk) { t -= nt - iblk; ++iblk; }
	const int jblk = iblk + t;
	const int64_t k0 = (int64_t) slab * L, k1 = min(B, k0 + L);
	/* staging: thread -> row tid >> 3 of the chunk, columns 8 (tid & 7) .. + 7 of either panel */
	const int sr = tid >> 3, sc = (tid & 7) * 8;
	const double* gI = P + (int64_t) iblk * HU_UF_TILE + sc;
	const double* gJ = P + (int64_t) jblk * HU_UF_TILE + sc;
	double2 ri[4], rj[4]; double rb = 0.0;
	auto fetch = [&](int64_t kc) {
		const int64_t k = kc + sr;
		if(k < k1) {
			const double2* a = (const double2*)(gI + k * Sp); const double2* c = (const double2*)(gJ + k * Sp);
#pragma unroll
			for(int u = 0; u < 4; ++u) { ri[u] = a[u]; rj[u] = c[u]; }
		}
		else {
#pragma unroll
			for(int u = 0; u < 4; ++u) { ri[u] = make_double2(0.0, 0.0); rj[u] = make_double2(0.0, 0.0); }
		}
		if(tid < HU_UF_CHUNK) rb = kc + tid < k1 ? blen[kc + tid] : 0.0;
	};
	double num[4][4], den[4][4];
#pragma unroll
	for(int r = 0; r < 4; ++r)
#pragma unroll
		for(int c = 0; c < 4; ++c) { num[r][c] = 0.0; den[r][c] = 0.0; }
	fetch(k0);
	for(int64_t kc = k0; kc < k1; kc += HU_UF_CHUNK) {
		__syncthreads();                                                  /* the chunk before has been added */
#pragma unroll
		for(int u = 0; u < 4; ++u) {
			double2 a = ri[u], c = rj[u];
			if(METHOD == HU_UF_UNWEIGHTED) { a.x = a.x > 0 ? 1.0 : 0.0; a.y = a.y > 0 ? 1.0 : 0.0; c.x = c.x > 0 ? 1.0 : 0.0; c.y = c.y > 0 ? 1.0 : 0.0; }
			*(double2*) &sI[sr][sc + 2 * u] = a; *(double2*) &sJ[sr][sc + 2 * u] = c;
		}
		if(tid < HU_UF_CHUNK) sB[tid] = rb;
		__syncthreads();
		if(kc + HU_UF_CHUNK < k1) fetch(kc + HU_UF_CHUNK);
#pragma unroll 4
		for(int k = 0; k < HU_UF_CHUNK; ++k) {
			const double b = sB[k];
			const double2 x0 = *(const double2*) &sI[k][2 * ty], x1 = *(const double2*) &sI[k][32 + 2 * ty];
			const double2 y0 = *(const double2*) &sJ[k][2 * tx], y1 = *(const double2*) &sJ[k][32 + 2 * tx];
			const double x[4] = {x0.x, x0.y, x1.x, x1.y}, y[4] = {y0.x, y0.y, y1.x, y1.y};
#pragma unroll
			for(int r = 0; r < 4; ++r)
#pragma unroll
				for(int c = 0; c < 4; ++c) hu_uf_term<METHOD>(b, x[r], y[c], alpha, num[r][c], den[r][c]);
		}
	}
	double* out = part + ((int64_t) slab * nTile + tile) * (2 * HU_UF_TILE * HU_UF_TILE);
#pragma unroll
	for(int r = 0; r < 4; ++r) {
		const int row = 2 * ty + (r & 1) + 32 * (r >> 1);
#pragma unroll
		for(int h = 0; h < 2; ++h) {
			const int col = 2 * tx + 32 * h;
			*(double2*) &out[row * HU_UF_TILE + col] = make_double2(num[r][2 * h], num[r][2 * h + 1]);
			if(METHOD != HU_UF_WEIGHTED_RAW) *(double2*) &out[HU_UF_TILE * HU_UF_TILE + row * HU_UF_TILE + col] = make_double2(den[r][2 * h], den[r][2 * h + 1]);
		}
	}
}

/* grid (tiles, slabs) */
template<int METHOD> __global__ void __launch_bounds__(HU_UF_WG) k_unifrac_pairs(const double* __restrict__ P, const double* __restrict__ blen,
		double* __restrict__ part, int64_t Sp, int64_t B, int64_t L, double alpha) {
	hu_uf_pairs_wg<METHOD>(P, blen, part, Sp, B, L, alpha, (int) blockIdx.x, (int) blockIdx.y, (int) gridDim.x);
}

/* grid (tiles, 16): a thread per pair of the tile */
static __global__ void __launch_bounds__(256) k_unifrac_finish(const double* __restrict__ part, double* __restrict__ dist, int64_t S, int64_t Sp, int64_t nSlab, int raw) {
	const int nt = (int)(Sp / HU_UF_TILE);
	int t = blockIdx.x, iblk = 0;
	while(t >= nt - iblk) { t -= nt - iblk; ++iblk; }
	const int jblk = iblk + t;
	const int e = blockIdx.y * 256 + threadIdx.x, row = e >> 6, col = e & 63;
	const int64_t i = (int64_t) iblk * HU_UF_TILE + row, j = (int64_t) jblk * HU_UF_TILE + col;
	if(i >= S || j >= S || i > j) return;
	if(i == j) { dist[i * S + i] = 0.0; return; }
	double N = 0.0, D = 0.0;
	for(int64_t s = 0; s < nSlab; ++s) {
		const double* p = part + (s * gridDim.x + blockIdx.x) * (2 * HU_UF_TILE * HU_UF_TILE) + e;
		N += p[0];
		if(!raw) D += p[HU_UF_TILE * HU_UF_TILE];
	}
	const double d = raw ? N : D > 0 ? N / D : 0.0;
	dist[i * S + j] = d; dist[j * S + i] = d;
}

/* grid (ceil(Sp / 256), slabs) */
static __global__ void __launch_bounds__(256) k_unifrac_pd(const double* __restrict__ P, const double* __restrict__ blen, double* __restrict__ pdPart, int64_t Sp, int64_t B, int64_t L) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= Sp) return;
	const int64_t k0 = (int64_t) blockIdx.y * L, k1 = min(B, k0 + L);
	double acc = 0.0;
	for(int64_t k = k0; k < k1; ++k) acc += P[k * Sp + j] > 0 ? blen[k] : 0.0;
	pdPart[(int64_t) blockIdx.y * Sp + j] = acc;
}

static __global__ void __launch_bounds__(256) k_unifrac_pd_finish(const double* __restrict__ pdPart, double* __restrict__ pd, int64_t S, int64_t Sp, int64_t nSlab) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= S) return;
	double tot = 0.0;
	for(int64_t s = 0; s < nSlab; ++s) tot += pdPart[s * Sp + j];
	pd[j] = tot;
}
