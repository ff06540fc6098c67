// The per-branch optimiser of the fit under the discrete Gamma of rates: one workgroup per non-root node finds the
// maximiser of
//   f_u(t) = sum_j [K_j - log K + log S_j(t)],   S_j(t) = sum_c w_jc (1 + sum_m r_jcm exp(lam_m rate_c t))
// on [lo, hi] from the two directed messages of the branch in every rate category, which the sweeps over the categories
// (k_tree_up_cat, k_tree_down_cat) leave in log space.  One pass over the messages (64 K bytes per column) leaves w_jc and w_jc r_jcm of
// every column, 4 K doubles: in LDS while four workgroups' values fit a CU's 160 KB (LDS = true), and otherwise in a global scratch
// [slab][4 K][L] for the branches of one launch.  Every later evaluation of f' and f'' costs 3 K exp per branch, which the first 3 K
// threads leave in LDS, and none per column.  Column j belongs to thread j % HU_BLEN_WG in every pass, so a thread reads back only what
// it wrote itself; the sums run serially per thread in ascending column and then down blen_reduce's fixed tree.  Every output has one
// writer; no atomics, no waiting for another workgroup.  The Newton tail is hu_blen_solve, as in k_blen_step.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_kern_blen.h"
#include "hu_tree_gamma.h"

struct HuGammaArgs {
	const double* up; const double* down;     /* [K][n][csLen][4], log space */
	const double* t;                           /* [n]: where the scores are taken, and where the step starts */
	const double* lr;                          /* [3 K]: lam_m rate_c */
	int64_t csLen; int32_t n, root, doStep, K, node0, pad0;   /* node0: the first node of this launch */
	double lo, hi, logK;
	double* scratch;                           /* LDS = false: [gridDim.x][4 K][csLen] */
	double* tStar; double* f; double* d1; double* d2; int32_t* iters;   /* [n]; iters = HU_BLEN_MAX_NEWTON + 1: the cap was hit */
	HuBlenModel m;
};

template<bool LDS> __global__ __launch_bounds__(HU_BLEN_WG) void k_gamma_step(HuGammaArgs a) {
	extern __shared__ __attribute__((aligned(16))) double gamma_sm[];
	const int64_t u = (int64_t) a.node0 + blockIdx.x, L = a.csLen;
	if(u >= a.n || u == a.root) return;
	const int tid = threadIdx.x, K = a.K;
	double* red = gamma_sm;                                           /* [3][HU_BLEN_WG] */
	double* E = gamma_sm + 3 * HU_BLEN_WG;                            /* [K][9] */
	double* S = LDS ? E + (9 * K + (9 * K & 1)) : a.scratch + (int64_t) blockIdx.x * 4 * K * L;   /* [4 K][L] */
	const int64_t cat = (int64_t) a.n * L * 4;
	const double* mu = a.up + u * L * 4;
	const double* md = a.down + u * L * 4;
	const double t0 = a.t[u];
	if(tid < 3 * K) hu_gamma_exp1(a.lr, t0, tid, E);
	__syncthreads();
	/* pass 1: the weights and the weighted ratios, and the scores at t0 */
	double v[3] = {0.0, 0.0, 0.0};
	for(int64_t j = tid; j < L; j += HU_BLEN_WG) {
		for(int c = 0; c < K; ++c) {
			double Mu[4], Md[4], r[3], Kc;
			blen_ld4(mu + c * cat + j * 4, Mu); blen_ld4(md + c * cat + j * 4, Md);
			hu_blen_column(a.m, Mu, Md, r, &Kc);
			hu_gamma_put(S + j, L, c, r, Kc);
		}
		const double Kj = hu_gamma_close(S + j, L, K);
		double g, h;
		const double Sj = hu_gamma_sums(E, S + j, L, K, &g, &h);
		v[0] += (Kj - a.logK) + log(Sj); v[1] += g; v[2] += h;
	}
	blen_reduce<3>(red, v);
	const double g0 = v[1], h0 = v[2];
	if(tid == 0) { a.f[u] = v[0]; a.d1[u] = g0; a.d2[u] = h0; }
	if(!a.doStep) return;
	/* every thread holds the same f' and f'', so the control flow of the solver is uniform; blen_reduce ends in a barrier, so E is free
	 * to be written again when an evaluation begins */
	auto eval = [&](double x, double* g, double* h) {
		if(tid < 3 * K) hu_gamma_exp1(a.lr, x, tid, E);
		__syncthreads();
		double w[2] = {0.0, 0.0};
		for(int64_t j = tid; j < L; j += HU_BLEN_WG) { double p, q; hu_gamma_sums(E, S + j, L, K, &p, &q); w[0] += p; w[1] += q; }
		blen_reduce<2>(red, w);
		*g = w[0]; *h = w[1];
	};
	int it = 0;
	const double x = hu_blen_solve(t0, g0, h0, a.lo, a.hi, eval, &it);
	if(tid == 0) { a.tStar[u] = x; a.iters[u] = it; }
}
