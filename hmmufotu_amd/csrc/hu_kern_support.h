// The kernels of the local branch supports.
// k_support_weights: one thread per replicate draws its cs_len columns (Philox4x32-10, hu_tree_support.h) and counts them in its own
// column b of the table Wt [cs_len][Bpad] of uint16, which the host zeroed: no atomics, and the table is replicate-minor, so that the
// lanes of k_nni_support, which hold neighbouring replicates, read neighbouring counts.
// k_nni_support: one workgroup per eligible edge, launched after k_nni_score with its t*_q.  Phase A is pass 1 of k_nni_score again,
// the same hu_nni_pentry and hu_nni_column with column j in thread j % HU_NNI_WG: instead of the nine ratios it leaves the pair
// (d^1_j, d^2_j), 16 bytes a column, in LDS (LDS = true, cs_len <= HU_SUPPORT_LDS_COLS) or in the edge's part of the ratio scratch of
// the scoring, and it sums K and log D down blen_reduce's tree as the scorer does, so that f^q(t*_q) comes out again to the bit.
// Phase B: a thread holds HU_SUPPORT_RPT neighbouring replicates and walks the columns in ascending order; per column one broadcast
// read of the pair and one 8-byte read of its four counts, which a wave reads as 512 contiguous bytes.  S is a multiply and then an
// add (-ffp-contract=off).  The supporting replicates are counted by an integer reduction; thread 0 is the one writer of the edge's
// outputs.  No floating-point atomics, no waiting for another workgroup, 64-bit indices.
#pragma once
#include <hip/hip_runtime.h>
#include "hu_kern_blen.h"
#include "hu_tree_support.h"

struct HuSupportArgs {
	const double* up; const double* down;     /* [n][csLen][4], log space */
	const HuNniEdge* edges;                    /* [nEdges], this launch's first edge at index 0 */
	const HuBlenModel* m;
	int64_t csLen, B, Bpad; int32_t n, nEdges;
	const double* tStar;                       /* [nEdges][3] */
	const uint16_t* Wt;                        /* [csLen][Bpad] */
	double* dScratch;                          /* LDS = false: the edge's 9 csLen doubles of the ratio scratch, of which 2 csLen are used */
	double* f2;                                /* [nEdges][3] */
	int32_t* count; int32_t* bad;              /* [nEdges]; bad: the columns whose l^0 is not finite */
	double* sums;                              /* [nEdges][B][2], or NULL */
};

__global__ __launch_bounds__(256) void k_support_weights(uint16_t* Wt, int64_t L, int64_t B, int64_t Bpad, uint64_t seed) {
	const int64_t b = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if(b >= B) return;
	for(int64_t i = 0; i < L; i += 4) {
		uint32_t col[4];
		hu_support_draw4(seed, (uint32_t) b, (uint32_t)(i / 4), (uint32_t) L, col);
		for(int k = 0; k < 4; ++k) if(i + k < L) Wt[(int64_t) col[k] * Bpad + b]++;      /* col < L: the high word of a product with L */
	}
}

/* the counts of a thread's RPT neighbouring replicates: one aligned read of 2 RPT bytes */
template<int RPT> struct alignas(2 * RPT) HuSupportCounts { uint16_t v[RPT]; };

/* RPT is HU_SUPPORT_RPT in the library; profiles/ubench/support_plain.hip measures the others.  Bpad is a multiple of RPT */
template<bool LDS, int RPT> __global__ __launch_bounds__(HU_NNI_WG) void k_nni_support(HuSupportArgs a) {
	extern __shared__ __attribute__((aligned(16))) double sup_sm[];
	const int64_t e = blockIdx.x, L = a.csLen;
	if(e >= a.nEdges) return;
	const int tid = threadIdx.x;
	const HuBlenModel& m = *a.m;
	const HuNniEdge& ed = a.edges[e];
	double* red = sup_sm;                                                /* [3][HU_NNI_WG]; the four P(t) in its first 64 entries during phase A */
	double* dBase = LDS ? sup_sm + 3 * HU_NNI_WG : a.dScratch + e * 9 * L;
	if(!LDS && (reinterpret_cast<uintptr_t>(dBase) & 15) != 0) ++dBase;    /* 9 L may be odd: the pairs are read 16 bytes at once, and 2 L + 1 <= 9 L */
	double2* Dp = reinterpret_cast<double2*>(dBase);                     /* [L] */
	if(tid < 64) red[tid] = hu_nni_pentry(m, ed.len[tid >> 4], (tid >> 2) & 3, tid & 3);
	__syncthreads();
	const double* src[4];
	for(int k = 0; k < 4; ++k) { const int64_t x = ed.msg[k]; src[k] = x < a.n ? a.up + x * L * 4 : a.down + (x - a.n) * L * 4; }
	HuBlenExp E[3];
	for(int q = 0; q < 3; ++q) hu_blen_exp(m, a.tStar[e * 3 + q], &E[q]);
	/* phase A: the pair of every column, and K and log D summed as the scorer sums them */
	double sK[3] = {0.0, 0.0, 0.0}, sD[3] = {0.0, 0.0, 0.0};
	int nBad = 0;
	for(int64_t j = tid; j < L; j += HU_NNI_WG) {
		double M[16], K[3], lD[3], d[2];
		for(int k = 0; k < 4; ++k) blen_ld4(src[k] + j * 4, M + k * 4);
		if(!hu_support_column(m, red, M, E, K, lD, d)) ++nBad;
		Dp[j] = make_double2(d[0], d[1]);
		for(int q = 0; q < 3; ++q) { sK[q] += K[q]; sD[q] += lD[q]; }
	}
	__syncthreads();                                                     /* the P(t) are read no more: the scratch is the reduction's */
	blen_reduce<3>(red, sK); blen_reduce<3>(red, sD);
	int32_t* ired = reinterpret_cast<int32_t*>(red);                     /* [HU_NNI_WG] */
	auto isum = [&](int v) {
		ired[tid] = v;
		__syncthreads();
		for(int s = HU_NNI_WG / 2; s > 0; s >>= 1) { if(tid < s) ired[tid] += ired[tid + s]; __syncthreads(); }
		const int r = ired[0];
		__syncthreads();
		return r;
	};
	nBad = isum(nBad);                                                   /* its barriers also order the pairs before phase B */
	const double f0 = sK[0] + sD[0], eta = hu_support_eta(f0);
	/* phase B: RPT replicates per thread, the columns in ascending order */
	int mine = 0;
	for(int64_t base = 0; base < a.Bpad; base += (int64_t) HU_NNI_WG * RPT) {
		const int64_t b0 = base + (int64_t) tid * RPT;
		if(b0 >= a.Bpad) continue;                                       /* Bpad is a multiple of RPT: b0 + RPT - 1 < Bpad */
		double S1[RPT], S2[RPT];
		for(int k = 0; k < RPT; ++k) S1[k] = S2[k] = 0.0;
		const uint16_t* wp = a.Wt + b0;
		for(int64_t j = 0; j < L; ++j) {
			const double2 d = Dp[j];
			const HuSupportCounts<RPT> w = *reinterpret_cast<const HuSupportCounts<RPT>*>(wp + j * a.Bpad);
			for(int k = 0; k < RPT; ++k) { const double x = (double) w.v[k]; S1[k] += x * d.x; S2[k] += x * d.y; }
		}
		for(int k = 0; k < RPT; ++k) if(b0 + k < a.B) {
			if(a.sums) { double* s = a.sums + (e * a.B + b0 + k) * 2; s[0] = S1[k]; s[1] = S2[k]; }
			if(hu_support_supports(S1[k], S2[k], eta)) ++mine;
		}
	}
	const int total = isum(mine);
	if(tid == 0) { for(int q = 0; q < 3; ++q) a.f2[e * 3 + q] = sK[q] + sD[q]; a.count[e] = total; a.bad[e] = nBad; }
}
