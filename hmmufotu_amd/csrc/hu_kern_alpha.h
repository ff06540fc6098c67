// Alpha diversity and rarefaction curves on the device (hmmufotu-amd-alpha).
//
// A draw (sample j, depth m, repeat r) is the column that hu_otu_subset(counts, m, uniform, seed + r) gives: the m reads of the sample
// smallest in (key, t) order, the keys those of hu_otu_key under the key of seed + r.  The draws are taken by the kernels of
// hu_kern_draw.h, a group of up to HU_AL_DT depths of one (j, r) from one key computation per read and pass, each draw into its copy of
// the sample's nonzero cells, each cell at its place in depth-first row order.  Here is what follows a draw:
//   k_al_whole     the whole sample as a draw: its cells are the differences of its prefixes.
//   k_al_stats     one workgroup per draw: S, F1, F2, Q as integer sums, A in a fixed order.
//   k_al_pd        one workgroup per draw: the draw's cells become the inclusive prefix of their presence, and a kept branch is present
//                  when the prefix rises over its interval of cells; the lengths are added in a fixed order.
// Device memory holds nothing per read and nothing of the shape [n_otu][draws]: per draw the sample's nnz cells.
//
// Order: thread x of the 256 adds items x, x + 256, ... in ascending order, and hu_al_tree adds the 256 partial sums; both are functions
// of the table and the tree alone.  Every index formed here comes from arrays the host built (hu_alpha_host.cpp, hu_alpha.hip) from a
// checked table: a slot is below nnz; a branch entry has lo < hi <= nnz.
#pragma once
#include "hu_common.h"
#include "hu_alpha.h"
#include "hu_kern_draw.h"

/* the sum of the 256 values of a workgroup in thread 0: within a wave v[l] += v[l + d], d = 32 .. 1, then (w0 + w1) + (w2 + w3) */
__device__ inline double hu_al_tree(double v, double* lds /* [HU_AL_WAVES] */) {
	#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
	if((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
	__syncthreads();
	return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}
__device__ inline uint64_t hu_al_isum(uint64_t v, uint64_t* lds /* [HU_AL_WAVES] */) {
	#pragma unroll
	for(int d = 32; d >= 1; d >>= 1) v += (uint64_t) __shfl_down((unsigned long long) v, d);
	if((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
	__syncthreads();
	return lds[0] + lds[1] + lds[2] + lds[3];
}

static __global__ __launch_bounds__(HU_AL_WG) void k_al_whole(const HuAlSample* smp, const HuAlDraw* draw, const uint32_t* prefix, const uint32_t* slot, uint32_t* out) {
	const HuAlDraw d = draw[blockIdx.x];
	if(d.m != 0) return;
	const HuAlSample s = smp[d.smp];
	const uint32_t *P = prefix + s.pfx0, *L = slot + (s.pfx0 - s.col);
	for(uint32_t c = threadIdx.x; c < s.nnz; c += HU_AL_WG) out[d.cell0 + L[c]] = P[c + 1] - P[c];
}

static __global__ __launch_bounds__(HU_AL_WG) void k_al_stats(const HuAlSample* smp, const HuAlDraw* draw, const uint32_t* out, HuAlStat* stat) {
	__shared__ uint64_t li[4][HU_AL_WAVES];
	__shared__ double la[HU_AL_WAVES];
	const HuAlDraw d = draw[blockIdx.x];
	const uint32_t nnz = smp[d.smp].nnz;
	const uint32_t* o = out + d.cell0;
	uint64_t S = 0, F1 = 0, F2 = 0, Q = 0;
	double A = 0.0;
	for(uint32_t c = threadIdx.x; c < nnz; c += HU_AL_WG) {
		const uint64_t n = o[c];
		S += n > 0; F1 += n == 1; F2 += n == 2; Q += n * n;
		if(n >= 2) A += (double) n * log((double) n);
	}
	S = hu_al_isum(S, li[0]); F1 = hu_al_isum(F1, li[1]); F2 = hu_al_isum(F2, li[2]); Q = hu_al_isum(Q, li[3]);
	A = hu_al_tree(A, la);
	if(threadIdx.x == 0) {
		HuAlStat st;
		st.Q = Q; st.A = A; st.PD = 0.0; st.S = (uint32_t) S; st.F1 = (uint32_t) F1; st.F2 = (uint32_t) F2; st.pad = 0;
		stat[blockIdx.x] = st;
	}
}

/* after k_al_stats: the draw's cells are overwritten by the inclusive prefix of their presence */
static __global__ __launch_bounds__(HU_AL_WG) void k_al_pd(const HuAlSample* smp, const HuAlBranch* br, const HuAlDraw* draw, uint32_t* out, HuAlStat* stat) {
	__shared__ uint32_t ws[HU_AL_WAVES];
	__shared__ double la[HU_AL_WAVES];
	const HuAlDraw d = draw[blockIdx.x];
	const HuAlSample s = smp[d.smp];
	uint32_t* o = out + d.cell0;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t carry = 0;
	for(uint32_t c0 = 0; c0 < s.nnz; c0 += HU_AL_WG) {
		const uint32_t c = c0 + threadIdx.x;
		const uint32_t v = c < s.nnz ? (o[c] > 0 ? 1u : 0u) : 0u, incl = hu_draw_wave_scan(v, lane);
		if(lane == 63) ws[w] = incl;
		__syncthreads();
		uint32_t off = 0, tot = 0;
		#pragma unroll
		for(int x = 0; x < HU_AL_WAVES; ++x) { if(x < w) off += ws[x]; tot += ws[x]; }
		if(c < s.nnz) o[c] = carry + off + incl;
		carry += tot;
		__syncthreads();
	}
	const HuAlBranch* E = br + s.br0;
	double acc = 0.0;
	for(uint32_t e = threadIdx.x; e < s.nBr; e += HU_AL_WG) {
		const HuAlBranch x = E[e];
		const uint32_t hi = o[x.hi - 1], lo = x.lo ? o[x.lo - 1] : 0u;
		acc += hi > lo ? x.b : 0.0;
	}
	acc = hu_al_tree(acc, la);
	if(threadIdx.x == 0) stat[blockIdx.x].PD = acc;
}
