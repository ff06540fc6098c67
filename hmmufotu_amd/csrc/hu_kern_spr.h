// The scorer of the SPR search: one workgroup walks the neighbourhood of one pruned node v and finds, for the baseline
// and for every target edge w within the radius,
//   t*_w = argmax f_w(t) on [lo, hi],   f_w(t) = sum_j [K_j + log(1 + sum_k r_jk exp(lam_k t))],
// the objective of the pendant length of v hung into the middle of w.  The host lays the walk out as records in depth-first order
// (hu_tree_spr.h).  A record first recomputes a message without v (one step outwards from the edge of s, the product of the carried
// messages of the node's other neighbours) into a slot of the workgroup's stack, 32 bytes per column in log space in global memory,
// and then scores a target from that slot, the level sweeps' message of the far side and up[v].  The first 64 threads build the
// record's four P(t) from the spectral form into LDS, where the reduction scratch lies later.  One pass over the columns computes the
// message, stores it and leaves the three ratios of every column: in LDS up to HU_BLEN_LDS_COLS columns (LDS = true), in a global
// scratch of the same layout beyond (§22's measured switch).  The Newton loop (hu_blen_solve) then reads 24 B per column and
// evaluation.  Column j belongs to thread j % HU_SPR_WG in every pass and in every record, so a thread reads back only the slots and
// ratios it wrote itself: only the reductions and the staging of P(t) need barriers.  The sums run serially per thread in ascending
// column and then down blen_reduce's fixed tree, so the control flow of the Newton loops is uniform.  Thread 0 is the one writer of
// the outputs; no atomics, no waiting for another workgroup, 64-bit indices.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_kern_blen.h"
#include "hu_tree_spr.h"

struct HuSprArgs {
	const double* up; const double* down;     /* [n][csLen][4], log space */
	const HuSprNode* nodes;                    /* [nNodes], the launch's slab */
	const HuSprRec* recs;                      /* the slab's records; a node's begin at recOff - recBase */
	const HuBlenModel* m;
	int64_t csLen, recBase, outBase;
	int32_t n, nNodes, slots, pad0;
	double lo, hi;
	double* stack;                             /* [nNodes][slots][csLen][4] */
	double* ratio;                             /* LDS = false: [nNodes][3][csLen] */
	double* tStar; double* f;                  /* the slab's outputs; a node's begin at outOff - outBase */
	double* f0;                                /* [nNodes]: the baseline at t0 */
	int32_t* iters;                            /* as tStar; HU_BLEN_MAX_NEWTON + 1: the cap was hit */
};

template<bool LDS> __global__ __launch_bounds__(HU_SPR_WG) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_spr_score(HuSprArgs a) {
	extern __shared__ __attribute__((aligned(16))) double spr_sm[];
	const int64_t b = blockIdx.x, L = a.csLen;
	if(b >= a.nNodes) return;
	const int tid = threadIdx.x;
	const HuBlenModel& m = *a.m;
	const HuSprNode nd = a.nodes[b];
	double* red = spr_sm;                                              /* [3][HU_SPR_WG]; a record's four P(t) in its first 64 entries during its pass */
	double* R = LDS ? spr_sm + 3 * HU_SPR_WG : a.ratio + b * 3 * L;    /* [3][L] */
	double* stk = a.stack + b * a.slots * L * 4;
	const double* yv = a.up + (int64_t) nd.v * L * 4;
	const double t0 = nd.t0;
	const int64_t n = a.n;
	auto msg = [&](int64_t id) -> const double* { return id < n ? a.up + id * L * 4 : id < 2 * n ? a.down + (id - n) * L * 4 : stk + (id - 2 * n) * L * 4; };
	for(int32_t ri = 0; ri < nd.nRec; ++ri) {
		const HuSprRec rc = a.recs[nd.recOff - a.recBase + ri];
		if(tid < 64) red[tid] = hu_nni_pentry(m, tid < 16 ? rc.len0 : tid < 32 ? rc.len1 : tid < 48 ? rc.la : rc.lb, (tid >> 2) & 3, tid & 3);
		__syncthreads();
		const bool hasDst = rc.dst >= 0, hasT = rc.tnode >= 0;
		const double* s0 = hasDst ? msg(rc.src0) : a.up;
		const double* s1 = hasDst && rc.src1 >= 0 ? msg(rc.src1) : nullptr;
		double* dst = hasDst ? stk + (int64_t) rc.dst * L * 4 : nullptr;
		const bool ownA = hasDst && rc.sa == 2 * a.n + rc.dst;         /* the side just recomputed: taken from registers */
		const double* pa = hasT ? msg(rc.sa) : a.up;
		const double* pb = hasT ? msg(rc.sb) : a.up;
		HuBlenExp E;
		hu_blen_exp(m, t0, &E);
		/* the pass over the columns: the message of the step, the ratios of the target, and K, f' and f'' at t0 */
		double v[4] = {0.0, 0.0, 0.0, 0.0};                            /* K, log D, f', f'' */
		for(int64_t j = tid; j < L; j += HU_SPR_WG) {
			double Y[4] = {0.0, 0.0, 0.0, 0.0};
			if(hasDst) {
				double M[4], Z[4];
				blen_ld4(s0 + j * 4, M);
				hu_spr_conv(red, M, Y);
				if(s1) { blen_ld4(s1 + j * 4, M); hu_spr_conv(red + 16, M, Z); for(int i = 0; i < 4; ++i) Y[i] += Z[i]; }
				if(rc.acc) { blen_ld4(dst + j * 4, M); for(int i = 0; i < 4; ++i) Y[i] += M[i]; }
				blen_st4(dst + j * 4, Y);
			}
			if(hasT) {
				double B[4], V[4], r[3], K, g, h;
				if(!ownA) blen_ld4(pa + j * 4, Y);
				blen_ld4(pb + j * 4, B); blen_ld4(yv + j * 4, V);
				hu_spr_column(m, red + 32, Y, red + 48, B, V, r, &K);
				R[j] = r[0]; R[L + j] = r[1]; R[2 * L + j] = r[2];
				hu_blen_terms(E, r, &g, &h);
				v[0] += K; v[1] += log(hu_blen_den(E, r)); v[2] += g; v[3] += h;
			}
		}
		__syncthreads();                                               /* the P(t) are read no more: the scratch is the reduction's, or the next record's */
		if(!hasT) continue;
		blen_reduce<2>(red, v); blen_reduce<2>(red, v + 2);
		const int64_t o = nd.outOff - a.outBase + rc.out;
		if(tid == 0 && rc.dist == 0) a.f0[b] = v[0] + v[1];
		auto ratioAt = [&](int64_t j, double* r) { r[0] = R[j]; r[1] = R[L + j]; r[2] = R[2 * L + j]; };
		int it = 0;
		const double x = blen_solve_wg(m, t0, v[2], v[3], a.lo, a.hi, red, L, ratioAt, &it);
		const double w = blen_logden_wg(m, x, red, L, ratioAt);
		if(tid == 0) { a.tStar[o] = x; a.f[o] = v[0] + w; a.iters[o] = it; }
	}
}
