// The scorer of the NNI search: one workgroup per eligible edge finds, for the edge's three arrangements q,
//   t*_q = argmax f^q(t) on [lo, hi],   f^q(t) = sum_j [K^q_j + log(1 + sum_k r^q_jk exp(lam_k t))],
// from the four directed messages around the edge, which the level sweeps (hu_kern_tree.h) leave in log space.
// The first 64 threads build the four P(t) of the edge's outer branches from the spectral form (three exp each) into LDS, where the
// reduction scratch lies later.  Pass 1 reads the four messages (128 B per column, 16-byte loads), carries them to the ends of the edge
// and leaves the nine ratios r^q_jk of every column: in LDS while four workgroups' ratios and reduction scratch fit a CU's 160 KB
// (LDS = true, cs_len <= HU_NNI_LDS_COLS), in a global scratch of the same layout otherwise.  The three Newton loops (hu_blen_solve)
// then read 24 B per column and evaluation.  Column j belongs to thread j % HU_NNI_WG in every pass, so a thread reads back only what
// it wrote itself; the sums run serially per thread in ascending column and then down blen_reduce's fixed tree: their shape depends on
// cs_len alone and the control flow of the Newton loops is uniform.  Thread 0 is the one writer of the edge's outputs; no atomics, no
// waiting for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_kern_blen.h"
#include "hu_tree_nni.h"

struct HuNniArgs {
	const double* up; const double* down;     /* [n][csLen][4], log space */
	const HuNniEdge* edges;                    /* [nEdges] */
	const HuBlenModel* m;                      /* in a buffer: 60 doubles are no kernel arguments */
	int64_t csLen; int32_t n, nEdges;
	double lo, hi;
	double* ratio;                             /* LDS = false: [nEdges][9][csLen] */
	double* tStar; double* f;                  /* [nEdges][3] */
	double* f0;                                /* [nEdges] */
	int32_t* iters;                            /* [nEdges][3]; HU_BLEN_MAX_NEWTON + 1: the cap was hit */
};

template<bool LDS> __global__ __launch_bounds__(HU_NNI_WG) void k_nni_score(HuNniArgs a) {
	extern __shared__ __attribute__((aligned(16))) double nni_sm[];
	const int64_t e = blockIdx.x, L = a.csLen;
	if(e >= a.nEdges) return;
	const int tid = threadIdx.x;
	const HuBlenModel& m = *a.m;
	const HuNniEdge& ed = a.edges[e];
	double* red = nni_sm;                                              /* [3][HU_NNI_WG]; the four P(t) in its first 64 entries during pass 1 */
	double* R = LDS ? nni_sm + 3 * HU_NNI_WG : a.ratio + e * 9 * L;   /* [9][L] */
	if(tid < 64) red[tid] = hu_nni_pentry(m, ed.len[tid >> 4], (tid >> 2) & 3, tid & 3);
	__syncthreads();
	const double* src[4];
	for(int k = 0; k < 4; ++k) { const int64_t x = ed.msg[k]; src[k] = x < a.n ? a.up + x * L * 4 : a.down + (x - a.n) * L * 4; }
	const double t0 = ed.t0;
	HuBlenExp E;
	hu_blen_exp(m, t0, &E);
	/* pass 1: the ratios, the constants, and f' and f'' of the three arrangements at t0 */
	double sK[3] = {0.0, 0.0, 0.0}, sD[3] = {0.0, 0.0, 0.0}, sg[3] = {0.0, 0.0, 0.0}, sh[3] = {0.0, 0.0, 0.0};
	for(int64_t j = tid; j < L; j += HU_NNI_WG) {
		double M[16], r[9], K[3];
		for(int k = 0; k < 4; ++k) blen_ld4(src[k] + j * 4, M + k * 4);
		hu_nni_column(m, red, M, r, K);
		for(int i = 0; i < 9; ++i) R[i * L + j] = r[i];
		for(int q = 0; q < 3; ++q) {
			double g, h;
			hu_blen_terms(E, r + q * 3, &g, &h);
			sK[q] += K[q]; sD[q] += log(hu_blen_den(E, r + q * 3)); sg[q] += g; sh[q] += h;
		}
	}
	__syncthreads();                                                   /* the P(t) are read no more: the scratch is the reduction's */
	blen_reduce<3>(red, sK); blen_reduce<3>(red, sD); blen_reduce<3>(red, sg); blen_reduce<3>(red, sh);
	if(tid == 0) a.f0[e] = sK[0] + sD[0];
	for(int q = 0; q < 3; ++q) {
		const double* Rq = R + (int64_t) q * 3 * L;
		auto ratioAt = [&](int64_t j, double* r) { r[0] = Rq[j]; r[1] = Rq[L + j]; r[2] = Rq[2 * L + j]; };
		int it = 0;
		const double x = blen_solve_wg(m, t0, sg[q], sh[q], a.lo, a.hi, red, L, ratioAt, &it);
		const double w = blen_logden_wg(m, x, red, L, ratioAt);
		if(tid == 0) { a.tStar[e * 3 + q] = x; a.f[e * 3 + q] = sK[q] + w; a.iters[e * 3 + q] = it; }
	}
}
