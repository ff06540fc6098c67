// The scorer of the insertion of new sequences: one workgroup takes one edge w and a tile of queries and finds, for
// every query r of the tile,
//   t*_{w,r} = argmax f_{w,r}(t) on [lo, hi],   f_{w,r}(t) = sum_j [K_j + kappa(s_rj) + log(1 + sum_k rho_jk tau_k(s_rj) exp(lam_k t))],
// the objective of the pendant length of r hung into the middle of w.  The junction of the edge does not depend on the query: one
// pass over the two messages of w (64 B per column, two carries over blen[w] / 2 with their exp and log) leaves the edge's three
// ratios rho_jk = A_jk / A_j0 and the sum of its K_j, once for the whole tile.  The ratios lie where k_blen_step keeps them: in LDS up
// to HU_BLEN_LDS_COLS columns (LDS = true), in a global scratch of the same layout beyond (§22's measured switch).  The query's side
// is a look-up by the symbol of its column in a table of 20 values (hu_add_tab_entry), which lies in LDS with P(blen[w] / 2) behind
// the two rows of reduction scratch the sums use.  One Newton loop (hu_blen_solve) per query then reads 24 B of ratios and 1 B of the
// query's row per column and evaluation.  Column j belongs to thread j % HU_ADD_WG in every pass, so a thread reads back only the
// ratios it wrote itself.  The sums run serially per thread in ascending column and then down blen_reduce's fixed tree, so the
// control flow of the Newton loops is uniform and a value does not depend on the tile or the slab.  Thread 0 is the one writer of the
// outputs; no atomics, no waiting for another workgroup, 64-bit indices.  k_add_best finds every query's best edge in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_kern_blen.h"
#include "hu_tree_add.h"

struct HuAddArgs {
	const double* up; const double* down;     /* [n][csLen][4], log space */
	const double* blen;                        /* [n] */
	const int8_t* q;                           /* [nq][csLen]: the rows of the launch's queries */
	const HuBlenModel* m;
	int64_t csLen;
	int32_t n, root, nq, tile;
	double lo, hi, t0;
	double* ratio;                             /* LDS = false: [tiles][n][3][csLen] */
	double* tStar; double* f;                  /* [nq][n] */
	int32_t* bestW; double* bestT; double* bestF;   /* [nq] */
};

template<bool LDS> __global__ __launch_bounds__(HU_ADD_WG) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_add_score(HuAddArgs a) {
	extern __shared__ __attribute__((aligned(16))) double add_sm[];
	const int64_t w = blockIdx.x, ty = blockIdx.y, L = a.csLen, n = a.n;
	const int64_t q0 = ty * a.tile, q1 = q0 + a.tile < a.nq ? q0 + a.tile : a.nq;
	if(w >= n || q0 >= a.nq) return;
	const int tid = threadIdx.x;
	if(w == a.root) {
		if(tid == 0) for(int64_t q = q0; q < q1; ++q) { a.tStar[q * n + w] = 0.0; a.f[q * n + w] = -INFINITY; }
		return;
	}
	const HuBlenModel& m = *a.m;
	double* red = add_sm;                                              /* [2][HU_ADD_WG] for the sums */
	double* P = add_sm + 2 * HU_ADD_WG;                                /* [16] */
	double* tab = P + 16;                                              /* [HU_ADD_TAB] */
	double* R = LDS ? add_sm + 3 * HU_ADD_WG : a.ratio + (ty * n + w) * 3 * L;    /* [3][L] */
	if(tid < 16) P[tid] = hu_nni_pentry(m, 0.5 * a.blen[w], tid >> 2, tid & 3);
	else if(tid < 16 + HU_ADD_TAB) tab[tid - 16] = hu_add_tab_entry(m, tid - 16);
	__syncthreads();
	const double* mu = a.up + w * L * 4;
	const double* md = a.down + w * L * 4;
	/* the pass over the edge's messages: its ratios and the sum of its K */
	double vk[1] = {0.0};
	for(int64_t j = tid; j < L; j += HU_ADD_WG) {
		double Mu[4], Md[4], r[3], K;
		blen_ld4(mu + j * 4, Mu); blen_ld4(md + j * 4, Md);
		hu_add_edge_column(m, P, Mu, Md, r, &K);
		R[j] = r[0]; R[L + j] = r[1]; R[2 * L + j] = r[2];
		vk[0] += K;
	}
	blen_reduce<1>(red, vk);
	const double t0 = a.t0;
	for(int64_t q = q0; q < q1; ++q) {
		const int8_t* row = a.q + q * L;
		HuBlenExp E;
		hu_blen_exp(m, t0, &E);
		double v[3] = {0.0, 0.0, 0.0};                                     /* kappa, f' and f'' at t0 */
		for(int64_t j = tid; j < L; j += HU_ADD_WG) {
			const int s = hu_add_sym(row[j]);
			double r[3], g, h;
			hu_add_ratio(tab, s, R[j], R[L + j], R[2 * L + j], r);
			hu_blen_terms(E, r, &g, &h);
			v[0] += tab[15 + s]; v[1] += g; v[2] += h;
		}
		blen_reduce<1>(red, v); blen_reduce<2>(red, v + 1);
		auto ratioAt = [&](int64_t j, double* r) { hu_add_ratio(tab, hu_add_sym(row[j]), R[j], R[L + j], R[2 * L + j], r); };
		int it = 0;
		const double x = blen_solve_wg(m, t0, v[1], v[2], a.lo, a.hi, red, L, ratioAt, &it);
		const double u = blen_logden_wg(m, x, red, L, ratioAt);
		if(tid == 0) { a.tStar[q * n + w] = x; a.f[q * n + w] = (vk[0] + v[0]) + u; }
	}
}

/* the best edge of one query per workgroup: every thread scans its edges in ascending w, then a fixed tree over the threads */
__global__ __launch_bounds__(HU_ADD_WG) void k_add_best(HuAddArgs a) {
	__shared__ double sf[HU_ADD_WG];
	__shared__ int32_t sw[HU_ADD_WG];
	const int64_t q = blockIdx.x, n = a.n;
	if(q >= a.nq) return;
	const int tid = threadIdx.x;
	double bf = -INFINITY; int32_t bw = -1;
	for(int64_t w = tid; w < n; w += HU_ADD_WG) {
		if(w == a.root) continue;
		const double f = a.f[q * n + w];
		if(hu_add_better(f, (int32_t) w, bf, bw)) { bf = f; bw = (int32_t) w; }
	}
	sf[tid] = bf; sw[tid] = bw;
	__syncthreads();
	for(int s = HU_ADD_WG / 2; s > 0; s >>= 1) {
		if(tid < s && sw[tid + s] >= 0 && hu_add_better(sf[tid + s], sw[tid + s], sf[tid], sw[tid])) { sf[tid] = sf[tid + s]; sw[tid] = sw[tid + s]; }
		__syncthreads();
	}
	if(tid == 0) { a.bestW[q] = sw[0]; a.bestF[q] = sf[0]; a.bestT[q] = sw[0] >= 0 ? a.tStar[q * n + sw[0]] : 0.0; }
}
