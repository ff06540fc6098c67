// Neighbour joining on the device (hmmufotu-amd-tree).  D [n][n] with stride n, both triangles stored; the slots
// 0 .. r - 1 hold the active nodes, R [n] their row sums, id [n] their node numbers.  A join is five stream-ordered launches, and the
// host, which knows r without reading anything back, only enqueues them:
//   k_nj_pick     workgroup b scans the rows b, b + G, ... above the diagonal, lane by lane in ascending j, and leaves the least
//                 (Q, i, j) of its rows in cand[b]; the comparison is on all three, so neither G nor the lanes matter
//   k_nj_winner   one workgroup: the least of the G candidates; the lengths of the two branches, the join record, the new node's id
//   k_nj_update   a thread per slot k: d_uk into row and column i, R_k brought up to date
//   k_nj_move     a thread per slot k: the last slot's row into row and column j, with its R and id; nothing when j is the last slot
//   k_nj_rowsum   one workgroup: R_i of the new row, a thread per block of HU_NJ_SUM_BLOCK slots, then thread 0 adds the block sums
// and k_nj_end leaves the three last nodes and their lengths.  The records are read once when all joins are done.  No kernel waits
// for another workgroup, and nothing is added atomically: every value has one writer and a fixed order of operations, the order
// of hu_nj_host_run, built from the same functions of hu_tree_nj.h.
#pragma once
#include "hu_common.h"
#include "hu_tree_nj.h"

struct HuNjCand { double q; int32_t i, j; };

struct HuNjDev {
	double* D; double* R; int32_t* id; int64_t n;
	HuNjCand* cand;      /* [HU_NJ_PICK_WG] */
	HuNjCand* win;       /* [1] */
	int32_t* join;       /* [n - 3][2], then the three last nodes */
	double* len;         /* [n - 3][2], then their three lengths */
};

__device__ __forceinline__ void hu_nj_reduce_cand(HuNjCand* s, int tid, int nThreads) {
	for(int h = nThreads >> 1; h > 0; h >>= 1) {
		if(tid < h) { const HuNjCand o = s[tid + h]; if(hu_nj_less(o.q, o.i, o.j, s[tid].q, s[tid].i, s[tid].j)) s[tid] = o; }
		__syncthreads();
	}
}

/* grid (n): R_row = the sum of row blockIdx.x (rowFromWinner: of the winner's row i) over the slots [0, r) */
__global__ void __launch_bounds__(256) k_nj_rowsum(HuNjDev a, int64_t r, int rowFromWinner) {
	__shared__ double sB[HU_NJ_MAX_N / HU_NJ_SUM_BLOCK];
	const int64_t row = rowFromWinner ? a.win->i : blockIdx.x;
	const int64_t nb = (r + HU_NJ_SUM_BLOCK - 1) / HU_NJ_SUM_BLOCK;
	const double* src = a.D + row * a.n;
	for(int64_t b = threadIdx.x; b < nb; b += 256) {
		const int64_t k0 = b * HU_NJ_SUM_BLOCK, k1 = min(r, k0 + (int64_t) HU_NJ_SUM_BLOCK);
		double s = 0.0;
		for(int64_t k = k0; k < k1; ++k) s += src[k];
		sB[b] = s;
	}
	__syncthreads();
	if(threadIdx.x == 0) {
		double tot = 0.0;
		for(int64_t b = 0; b < nb; ++b) tot += sB[b];
		a.R[row] = tot;
	}
}

/* grid (G <= HU_NJ_PICK_WG) */
__global__ void __launch_bounds__(256) k_nj_pick(HuNjDev a, int64_t r) {
	__shared__ HuNjCand s[256];
	HuNjCand best; best.q = INFINITY; best.i = INT32_MAX; best.j = INT32_MAX;
	for(int64_t i = blockIdx.x; i < r - 1; i += gridDim.x) {
		const double Ri = a.R[i];
		const double* row = a.D + i * a.n;
		for(int64_t j = i + 1 + threadIdx.x; j < r; j += 256) {
			const double q = hu_nj_q(r, row[j], Ri, a.R[j]);
			if(hu_nj_less(q, (int32_t) i, (int32_t) j, best.q, best.i, best.j)) { best.q = q; best.i = (int32_t) i; best.j = (int32_t) j; }
		}
	}
	s[threadIdx.x] = best;
	__syncthreads();
	hu_nj_reduce_cand(s, threadIdx.x, 256);
	if(threadIdx.x == 0) a.cand[blockIdx.x] = s[0];
}

/* one workgroup; t: the join's number */
__global__ void __launch_bounds__(256) k_nj_winner(HuNjDev a, int64_t r, int64_t t, int nCand) {
	__shared__ HuNjCand s[256];
	HuNjCand best; best.q = INFINITY; best.i = INT32_MAX; best.j = INT32_MAX;
	for(int c = threadIdx.x; c < nCand; c += 256) { const HuNjCand o = a.cand[c]; if(hu_nj_less(o.q, o.i, o.j, best.q, best.i, best.j)) best = o; }
	s[threadIdx.x] = best;
	__syncthreads();
	hu_nj_reduce_cand(s, threadIdx.x, 256);
	if(threadIdx.x == 0) {
		HuNjCand w = s[0];
		if(w.i == INT32_MAX) { w.i = 0; w.j = 1; }                        /* every Q is not a number: as hu_nj_host_run */
		*a.win = w;
		double li, lj;
		hu_nj_lengths(r, a.D[(int64_t) w.i * a.n + w.j], a.R[w.i], a.R[w.j], &li, &lj);
		a.join[2 * t] = a.id[w.i]; a.join[2 * t + 1] = a.id[w.j];
		a.len[2 * t] = li; a.len[2 * t + 1] = lj;
		a.id[w.i] = (int32_t)(a.n + t);
	}
}

/* grid (ceil(r / 256)) */
__global__ void __launch_bounds__(256) k_nj_update(HuNjDev a, int64_t r) {
	const int64_t k = (int64_t) blockIdx.x * 256 + threadIdx.x;
	const int64_t i = a.win->i, j = a.win->j;
	if(k >= r || k == i || k == j) return;
	const double dij = a.D[i * a.n + j];                                 /* no thread writes this cell */
	const double dik = a.D[i * a.n + k], djk = a.D[j * a.n + k];
	const double duk = hu_nj_duk(dik, djk, dij);
	a.R[k] = hu_nj_rk(a.R[k], dik, djk, duk);
	a.D[i * a.n + k] = duk; a.D[k * a.n + i] = duk;
}

/* grid (ceil((r - 1) / 256)): reads row r - 1, writes row and column j */
__global__ void __launch_bounds__(256) k_nj_move(HuNjDev a, int64_t r) {
	const int64_t k = (int64_t) blockIdx.x * 256 + threadIdx.x;
	const int64_t j = a.win->j, last = r - 1;
	if(j == last || k >= last) return;
	if(k == j) { a.D[j * a.n + j] = 0.0; a.R[j] = a.R[last]; a.id[j] = a.id[last]; return; }
	const double v = a.D[last * a.n + k];
	a.D[j * a.n + k] = v; a.D[k * a.n + j] = v;
}

/* one thread: the three nodes left */
__global__ void k_nj_end(HuNjDev a) {
	if(threadIdx.x != 0 || blockIdx.x != 0) return;
	const int64_t m = 2 * (a.n - 3);
	double l[3];
	hu_nj_last3(a.D[1], a.D[2], a.D[a.n + 2], l);
	for(int s = 0; s < 3; ++s) { a.join[m + s] = a.id[s]; a.len[m + s] = l[s]; }
}
