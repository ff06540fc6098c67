// The per-branch optimiser of the branch-length fit: one workgroup per non-root node finds the maximiser of
//   f_u(t) = sum_j log L_j(t),   L_j(t) / c_j0 = 1 + sum_k r_jk exp(lam_k t)
// on [lo, hi] from the two directed messages of the branch, which the level sweeps (hu_kern_tree.h) leave in log space.
// One pass over the messages (64 B per column) leaves the three ratios r_jk of every column, in LDS while four workgroups' ratios and
// reduction scratch fit a CU's 160 KB (LDS = true, cs_len <= HU_BLEN_LDS_COLS) and in a global scratch of the same layout otherwise,
// which a workgroup reads back from the L2; every later evaluation of f' and f'' costs three exp per branch and none per column.
// Column j belongs to thread j % HU_BLEN_WG in every pass, so a thread reads back only what it wrote itself; the sums run serially
// per thread in ascending column and then down a fixed tree over the threads: their shape depends on cs_len alone.  Every output has
// one writer; no atomics, no waiting for another workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_tree_blen.h"

struct HuBlenArgs {
	const double* up; const double* down;     /* [n][csLen][4], log space */
	const double* t;                           /* [n]: where the scores are taken, and where the step starts */
	int64_t csLen; int32_t n, root, doStep, pad0;
	double lo, hi;
	double* ratio;                             /* LDS = false: [n][3][csLen] */
	double* tStar; double* f; double* d1; double* d2; int32_t* iters;   /* [n]; iters = HU_BLEN_MAX_NEWTON + 1: the cap was hit */
	HuBlenModel m;
};

/* sums of NV values over the workgroup: red [NV][HU_BLEN_WG]; every thread returns with all sums in v */
template<int NV> __device__ inline void blen_reduce(double* red, double* v) {
	const int tid = threadIdx.x;
	for(int c = 0; c < NV; ++c) red[c * HU_BLEN_WG + tid] = v[c];
	__syncthreads();
	for(int s = HU_BLEN_WG / 2; s > 0; s >>= 1) {
		if(tid < s) for(int c = 0; c < NV; ++c) red[c * HU_BLEN_WG + tid] += red[c * HU_BLEN_WG + tid + s];
		__syncthreads();
	}
	for(int c = 0; c < NV; ++c) v[c] = red[c * HU_BLEN_WG];
	__syncthreads();
}

/* a message's four entries of one column: 32 bytes as two 16-byte accesses */
__device__ inline void blen_ld4(const double* p, double* M) {
	const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
	M[0] = a.x; M[1] = a.y; M[2] = b.x; M[3] = b.y;
}
__device__ inline void blen_st4(double* p, const double* M) {
	*reinterpret_cast<double2*>(p) = make_double2(M[0], M[1]); *reinterpret_cast<double2*>(p + 2) = make_double2(M[2], M[3]);
}

/* the Newton tail of every scorer of the family, for the whole workgroup: the maximiser of f on [lo, hi] from t0, where f' and f'' are
 * g0 and h0 already (hu_blen_solve).  ratioAt(j, r) gives the three ratios of column j; column j belongs to thread j % HU_BLEN_WG, the
 * sums run serially per thread in ascending column and then down blen_reduce's tree, so every thread holds the same f' and f'' and the
 * control flow is uniform.  red [2][HU_BLEN_WG] */
template<class Ratio> __device__ inline double blen_solve_wg(const HuBlenModel& m, double t0, double g0, double h0, double lo, double hi, double* red, int64_t L,
		const Ratio& ratioAt, int* it) {
	HuBlenExp E;
	auto eval = [&](double x, double* g, double* h) {
		hu_blen_exp(m, x, &E);
		double w[2] = {0.0, 0.0};
		for(int64_t j = threadIdx.x; j < L; j += HU_BLEN_WG) {
			double r[3], p, q;
			ratioAt(j, r);
			hu_blen_terms(E, r, &p, &q);
			w[0] += p; w[1] += q;
		}
		blen_reduce<2>(red, w);
		*g = w[0]; *h = w[1];
	};
	return hu_blen_solve(t0, g0, h0, lo, hi, eval, it);
}
/* sum_j log D_j(x) over the workgroup, in every thread: what f(x) adds to the sum of the columns' constants.  red [HU_BLEN_WG] */
template<class Ratio> __device__ inline double blen_logden_wg(const HuBlenModel& m, double x, double* red, int64_t L, const Ratio& ratioAt) {
	HuBlenExp E;
	hu_blen_exp(m, x, &E);
	double w[1] = {0.0};
	for(int64_t j = threadIdx.x; j < L; j += HU_BLEN_WG) { double r[3]; ratioAt(j, r); w[0] += log(hu_blen_den(E, r)); }
	blen_reduce<1>(red, w);
	return w[0];
}

template<bool LDS> __global__ __launch_bounds__(HU_BLEN_WG) void k_blen_step(HuBlenArgs a) {
	extern __shared__ __attribute__((aligned(16))) double blen_sm[];
	const int64_t u = blockIdx.x, L = a.csLen;
	if(u >= a.n || u == a.root) return;
	const int tid = threadIdx.x;
	double* red = blen_sm;                                            /* [3][HU_BLEN_WG] */
	double* R = LDS ? blen_sm + 3 * HU_BLEN_WG : a.ratio + u * 3 * L;  /* [3][L] */
	const double* mu = a.up + u * L * 4;
	const double* md = a.down + u * L * 4;
	const double t0 = a.t[u];
	HuBlenExp E;
	hu_blen_exp(a.m, t0, &E);
	/* pass 1: the ratios, and the scores at t0 */
	double v[3] = {0.0, 0.0, 0.0};
	for(int64_t j = tid; j < L; j += HU_BLEN_WG) {
		double Mu[4], Md[4], r[3], K, g, h;
		blen_ld4(mu + j * 4, Mu); blen_ld4(md + j * 4, Md);
		hu_blen_column(a.m, Mu, Md, r, &K);
		R[j] = r[0]; R[L + j] = r[1]; R[2 * L + j] = r[2];
		hu_blen_terms(E, r, &g, &h);
		v[0] += K + log(hu_blen_den(E, r)); v[1] += g; v[2] += h;
	}
	blen_reduce<3>(red, v);
	const double g0 = v[1], h0 = v[2];
	if(tid == 0) { a.f[u] = v[0]; a.d1[u] = g0; a.d2[u] = h0; }
	if(!a.doStep) return;
	int it = 0;
	const double x = blen_solve_wg(a.m, t0, g0, h0, a.lo, a.hi, red, L, [&](int64_t j, double* r) { r[0] = R[j]; r[1] = R[L + j]; r[2] = R[2 * L + j]; }, &it);
	if(tid == 0) { a.tStar[u] = x; a.iters[u] = it; }
}
