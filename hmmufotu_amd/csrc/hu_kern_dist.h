// The pairwise distances of an alignment's rows (hmmufotu-amd-tree).
//
// Planes.  k_dist_encode turns the rows (codes of hu_msa_encode_table: A C G T = 0 1 2 3, negative = no symbol) into three planes of
// 64-bit words, plane [3][np][Wp]: V (the row holds a symbol), B0 (bit 0 of the code: C or T) and B1 (bit 1: G or T); np is n padded
// to whole tiles and Wp the words of a row padded to whole chunks, both with zero words, which count nothing.  For a pair of rows and
// one word, with v = Vi & Vj, x0 = B0i ^ B0j and x1 = B1i ^ B1j:
//   N   += popc(v)                       both hold a symbol
//   Q   += popc(v & x0)                  bit 0 differs: one of A, G against one of C, T, a transversion
//   P_R += popc(v & ~x0 & x1 & ~B0i)     bit 0 equal and clear, bit 1 differs: A <-> G
//   P_Y += popc(v & ~x0 & x1 &  B0i)     bit 0 equal and set, bit 1 differs: C <-> T
// Integers, so exact in any order.
//
// k_dist_pairs<COUNTS> is shaped like k_unifrac_pairs: a workgroup of 256 threads owns one 64 x 64 tile (iblk <= jblk) of the pair
// matrix and walks the words in chunks of HU_DIST_CHUNK.  The two panels of a chunk (3 planes x 64 rows x 8 words each, 24 KB with
// the padding) go through registers into LDS; the loads of the next chunk are issued before the current one is counted.  A thread
// holds a 4 x 4 register tile of the four counters: rows {2 t, 2 t + 1, 32 + 2 t, 33 + 2 t} on either side, so that a ds_read_b128
// fetches two rows' words, the 16 lanes of a group read 256 contiguous bytes on the j side and broadcast on the i side.  The epilogue
// applies hu_sub_dist (hu_tree_nj.h) and writes the value and its mirror; a saturated pair gets +inf, which k_dist_fix
// replaces.  COUNTS: the four integers are written instead.
//   k_dist_scan   per workgroup, the largest finite value and the number of +inf above the diagonal of its rows
//   k_dist_fix    replaces +inf by the fill value
#pragma once
#include "hu_common.h"
#include "hu_tree_nj.h"

#define HU_DIST_WG 256
#define HU_DIST_LDS_ROWS (HU_DIST_TILE + 2)     /* the padding keeps the 16-byte alignment of the paired reads */

/* grid (ceil(Wp / 256), np): a thread per (row, word) */
__global__ void __launch_bounds__(256) k_dist_encode(const int8_t* __restrict__ rows, uint64_t* __restrict__ plane, int64_t n, int64_t csLen, int64_t np, int64_t Wp) {
	const int64_t w = (int64_t) blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
	if(w >= Wp || row >= np) return;
	uint64_t v = 0, b0 = 0, b1 = 0;
	if(row < n) {
		const int64_t c0 = w * 64;
		const int8_t* src = rows + row * csLen;
		for(int b = 0; b < 64; ++b) {
			const int64_t c = c0 + b;
			if(c >= csLen) break;
			const int code = src[c];
			if(code >= 0) { v |= 1ull << b; b0 |= (uint64_t)(code & 1) << b; b1 |= (uint64_t)((code >> 1) & 1) << b; }
		}
	}
	plane[row * Wp + w] = v; plane[(np + row) * Wp + w] = b0; plane[(2 * np + row) * Wp + w] = b1;
}

struct HuDistArgs {
	const uint64_t* plane; int64_t np, Wp, n;
	int32_t type; double pi[4];
	double* D; int32_t* counts;
};

/* grid (tiles of the upper triangle) */
template<bool COUNTS> __global__ void __launch_bounds__(HU_DIST_WG) k_dist_pairs(HuDistArgs a) {
	__shared__ __attribute__((aligned(16))) uint64_t sI[3][HU_DIST_CHUNK][HU_DIST_LDS_ROWS], sJ[3][HU_DIST_CHUNK][HU_DIST_LDS_ROWS];
	const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
	const int nt = (int)(a.np / HU_DIST_TILE);
	int t = blockIdx.x, iblk = 0;
	while(t >= nt - iblk) { t -= nt - iblk; ++iblk; }
	const int jblk = iblk + t;
	/* staging: element e = tid + 256 u of a panel is (plane e / 512, row (e % 512) / 8, word e % 8): 8 lanes read 64 contiguous bytes */
	uint64_t ri[6], rj[6];
	auto fetch = [&](int64_t wc) {
#pragma unroll
		for(int u = 0; u < 6; ++u) {
			const int e = tid + 256 * u, p = e >> 9, row = (e & 511) >> 3, w = e & 7;
			ri[u] = a.plane[((int64_t) p * a.np + (int64_t) iblk * HU_DIST_TILE + row) * a.Wp + wc + w];
			rj[u] = a.plane[((int64_t) p * a.np + (int64_t) jblk * HU_DIST_TILE + row) * a.Wp + wc + w];
		}
	};
	int32_t cN[4][4], cR[4][4], cY[4][4], cQ[4][4];
#pragma unroll
	for(int r = 0; r < 4; ++r)
#pragma unroll
		for(int c = 0; c < 4; ++c) { cN[r][c] = 0; cR[r][c] = 0; cY[r][c] = 0; cQ[r][c] = 0; }
	fetch(0);
	for(int64_t wc = 0; wc < a.Wp; wc += HU_DIST_CHUNK) {
		__syncthreads();                                                  /* the chunk before has been counted */
#pragma unroll
		for(int u = 0; u < 6; ++u) {
			const int e = tid + 256 * u, p = e >> 9, row = (e & 511) >> 3, w = e & 7;
			sI[p][w][row] = ri[u]; sJ[p][w][row] = rj[u];
		}
		__syncthreads();
		if(wc + HU_DIST_CHUNK < a.Wp) fetch(wc + HU_DIST_CHUNK);
#pragma unroll 2
		for(int w = 0; w < HU_DIST_CHUNK; ++w) {
			uint64_t vi[4], ai[4], bi[4], vj[4], aj[4], bj[4];
#pragma unroll
			for(int h = 0; h < 2; ++h) {
				const ulonglong2 q0 = *(const ulonglong2*) &sI[0][w][2 * ty + 32 * h], q1 = *(const ulonglong2*) &sI[1][w][2 * ty + 32 * h], q2 = *(const ulonglong2*) &sI[2][w][2 * ty + 32 * h];
				vi[2 * h] = q0.x; vi[2 * h + 1] = q0.y; ai[2 * h] = q1.x; ai[2 * h + 1] = q1.y; bi[2 * h] = q2.x; bi[2 * h + 1] = q2.y;
				const ulonglong2 p0 = *(const ulonglong2*) &sJ[0][w][2 * tx + 32 * h], p1 = *(const ulonglong2*) &sJ[1][w][2 * tx + 32 * h], p2 = *(const ulonglong2*) &sJ[2][w][2 * tx + 32 * h];
				vj[2 * h] = p0.x; vj[2 * h + 1] = p0.y; aj[2 * h] = p1.x; aj[2 * h + 1] = p1.y; bj[2 * h] = p2.x; bj[2 * h + 1] = p2.y;
			}
#pragma unroll
			for(int r = 0; r < 4; ++r)
#pragma unroll
				for(int c = 0; c < 4; ++c) {
					const uint64_t v = vi[r] & vj[c], x0 = ai[r] ^ aj[c], x1 = bi[r] ^ bj[c];
					const uint64_t ts = v & ~x0 & x1;
					cN[r][c] += __popcll(v);
					cQ[r][c] += __popcll(v & x0);
					cR[r][c] += __popcll(ts & ~ai[r]);
					cY[r][c] += __popcll(ts & ai[r]);
				}
		}
	}
#pragma unroll
	for(int r = 0; r < 4; ++r) {
		const int64_t i = (int64_t) iblk * HU_DIST_TILE + 2 * ty + (r & 1) + 32 * (r >> 1);
#pragma unroll
		for(int c = 0; c < 4; ++c) {
			const int64_t j = (int64_t) jblk * HU_DIST_TILE + 2 * tx + (c & 1) + 32 * (c >> 1);
			if(i >= a.n || j >= a.n) continue;
			if(COUNTS) {
				if(iblk == jblk && i > j) continue;                           /* a diagonal tile holds both orders: one writes */
				const int4 q = make_int4(cN[r][c], cR[r][c], cY[r][c], cQ[r][c]);
				*(int4*) &a.counts[(i * a.n + j) * 4] = q; *(int4*) &a.counts[(j * a.n + i) * 4] = q;
			}
			else {
				if(i == j) { a.D[i * a.n + i] = 0.0; continue; }
				if(iblk == jblk && i > j) continue;
				int s = 0;
				double d = hu_sub_dist(a.type, a.pi, cN[r][c], cR[r][c], cY[r][c], cQ[r][c], &s);
				if(s) d = INFINITY;                                            /* k_dist_fix replaces it */
				a.D[i * a.n + j] = d; a.D[j * a.n + i] = d;
			}
		}
	}
}

/* grid (G): workgroup b takes the rows b, b + G, ...; above the diagonal only */
__global__ void __launch_bounds__(256) k_dist_scan(const double* __restrict__ D, int64_t n, double* __restrict__ blkMax, unsigned long long* __restrict__ blkInf) {
	__shared__ double sM[256];
	__shared__ unsigned long long sC[256];
	double m = -1.0; unsigned long long c = 0;
	for(int64_t i = blockIdx.x; i < n; i += gridDim.x)
		for(int64_t j = i + 1 + threadIdx.x; j < n; j += 256) {
			const double d = D[i * n + j];
			if(isinf(d)) ++c; else if(d > m) m = d;
		}
	sM[threadIdx.x] = m; sC[threadIdx.x] = c;
	__syncthreads();
	for(int s = 128; s > 0; s >>= 1) {
		if((int) threadIdx.x < s) { sM[threadIdx.x] = fmax(sM[threadIdx.x], sM[threadIdx.x + s]); sC[threadIdx.x] += sC[threadIdx.x + s]; }
		__syncthreads();
	}
	if(threadIdx.x == 0) { blkMax[blockIdx.x] = sM[0]; blkInf[blockIdx.x] = sC[0]; }
}

__global__ void __launch_bounds__(256) k_dist_fix(double* __restrict__ D, int64_t total, double fill) {
	for(int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t) gridDim.x * 256) if(isinf(D[e])) D[e] = fill;
}
