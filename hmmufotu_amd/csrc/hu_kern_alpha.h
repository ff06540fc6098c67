// Alpha diversity and rarefaction curves on the device (hmmufotu-amd-alpha).
//
// A draw (sample j, depth m, repeat r) is the column that hu_otu_subset(counts, m, uniform, seed + r) gives: the m reads of the sample
// smallest in (key, t) order, the keys those of hu_otu_key under the key of seed + r.  The kept sets of one (j, r) are nested in m, so
// a group of up to HU_AL_DT depths shares every key computation: a workgroup takes one (group, chunk of reads) pair of the host's list,
// computes a read's key once per pass and serves all depths of the group with it.
//   k_al_hist      one digit of the radix select (hu_kern_otu.h's, per draw): one LDS histogram per depth of the group.
//   k_al_pick      one wave per draw: the digit in which the wanted rank falls; the histogram is cleared for the next pass.
//   k_al_ties      for the draws whose cut key is shared by more reads than are still wanted: the reads with that key per (chunk, wave) span;
//   k_al_tie_scan  turns a draw's counts into exclusive prefixes, one wave per draw.
//   k_al_take      recomputes the keys, decides each read for every depth of the group and counts it into the draw's copy of the
//                  sample's nonzero cells, each at its place in depth-first row order: cells are runs of lanes, one integer atomic per (round, run, depth) with a kept read.
//   k_al_whole     the whole sample as a draw: its cells are the differences of its prefixes.
//   k_al_stats     one workgroup per draw: S, F1, F2, Q as integer sums, A in a fixed order.
//   k_al_pd        one workgroup per draw: the draw's cells become the inclusive prefix of their presence, and a kept branch is present
//                  when the prefix rises over its interval of cells; the lengths are added in a fixed order.
// Device memory holds nothing per read and nothing of the shape [n_otu][draws]: per draw the sample's nnz cells.
//
// Order: thread x of the 256 adds items x, x + 256, ... in ascending order, and hu_al_tree adds the 256 partial sums; both are functions
// of the table and the tree alone.  Integer atomics elsewhere.  Every index formed here comes from arrays the host built
// (hu_alpha_host.cpp, hu_alpha.hip) from a checked table: prefix[cell + 1] of a valid read is read below the sample's last entry, which
// holds T; a slot is below nnz; a branch entry has lo < hi <= nnz.
#pragma once
#include "hu_common.h"
#include "hu_alpha.h"

__device__ inline uint32_t hu_al_wave_scan(uint32_t v, int lane) {     /* inclusive */
	#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d); if(lane >= d) v += u; }
	return v;
}
/* the reads of wave w of the chunk that starts at t0 */
__device__ inline void hu_al_span(uint32_t t0, uint32_t T, int chunkLen, int w, uint64_t& b, uint64_t& e) {
	const uint64_t end = min((uint64_t) t0 + (uint64_t) chunkLen, (uint64_t) T), len = end - t0, S = (len + HU_AL_WAVES - 1) / HU_AL_WAVES;
	b = min((uint64_t) t0 + (uint64_t) w * S, end); e = min(b + S, end);
}
/* the cell that owns read t: the largest c with P[c] <= t, for t < P[nnz] */
__device__ inline uint32_t hu_al_cell(const uint32_t* P, uint32_t nnz, uint32_t t) {
	uint32_t lo = 0, hi = nnz;
	while(hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if(P[mid] <= t) lo = mid; else hi = mid; }
	return lo;
}
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

static __global__ __launch_bounds__(HU_AL_WG) void k_al_hist(const HuAlSample* smp, const HuAlGroup* grp, const HuAlChunk* chunk, const HuAlSel* sel, uint32_t* hist,
		int keyBits, int chunkLen, int shift, int first) {
	__shared__ uint32_t h[HU_AL_DT][256];
	const HuAlChunk c = chunk[blockIdx.x];
	const HuAlGroup g = grp[c.g];
	const int d0 = blockIdx.y * HU_AL_DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(HU_AL_DT, (int) g.nd - d0);
	const uint32_t T = smp[g.smp].T, col = smp[g.smp].col;
	uint64_t pre[HU_AL_DT];
	#pragma unroll
	for(int i = 0; i < HU_AL_DT; ++i) { pre[i] = i < nd ? sel[g.draw0 + d0 + i].prefix : 0; h[i][threadIdx.x] = 0; }
	__syncthreads();
	const uint32_t key[2] = {g.k0, g.k1};
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) chunkLen, (uint64_t) T);
	for(uint64_t t = (uint64_t) c.t0 + threadIdx.x; t < end; t += HU_AL_WG) {
		const uint64_t k = hu_otu_key(key, t, col, keyBits);
		const uint32_t digit = (uint32_t)(k >> shift) & 255u;
		const uint64_t hi = first ? 0 : k >> (shift + 8);
		#pragma unroll
		for(int i = 0; i < HU_AL_DT; ++i) if(i < nd && (first || hi == pre[i])) atomicAdd(&h[i][digit], 1u);
	}
	__syncthreads();
	#pragma unroll
	for(int i = 0; i < HU_AL_DT; ++i) if(i < nd) {
		const uint32_t v = h[i][threadIdx.x];
		if(v) atomicAdd(&hist[(size_t)(g.draw0 + d0 + i) * 256 + threadIdx.x], v);
	}
}

static __global__ __launch_bounds__(64) void k_al_pick(const HuAlDraw* draw, HuAlSel* sel, uint32_t* hist) {
	const int a = blockIdx.x, lane = threadIdx.x;
	if(draw[a].m == 0) return;
	uint4* h4 = (uint4*)(hist + (size_t) a * 256);
	const uint4 v = h4[lane];
	h4[lane] = make_uint4(0, 0, 0, 0);
	const HuAlSel s = sel[a];
	const uint32_t sum = v.x + v.y + v.z + v.w, incl = hu_al_wave_scan(sum, lane);
	uint32_t cum = incl - sum;                                 /* reads in the bins below this lane's four */
	/* the bins hold the s.eq reads that carry the prefix, and 1 <= rank <= eq: exactly one lane has cum < rank <= incl */
	if(cum < s.rank && s.rank <= incl) {
		int d = 0;
		if(cum + v.x < s.rank) { cum += v.x; d = 1; if(cum + v.y < s.rank) { cum += v.y; d = 2; if(cum + v.z < s.rank) { cum += v.z; d = 3; } } }
		HuAlSel n;
		n.prefix = (s.prefix << 8) | (uint64_t)(lane * 4 + d); n.rank = s.rank - cum; n.eq = d == 0 ? v.x : d == 1 ? v.y : d == 2 ? v.z : v.w;
		sel[a] = n;
	}
}

static __global__ __launch_bounds__(HU_AL_WG) void k_al_ties(const HuAlSample* smp, const HuAlGroup* grp, const HuAlChunk* chunk, const HuAlDraw* draw, const HuAlSel* sel,
		uint32_t* tie, int keyBits, int chunkLen) {
	const HuAlChunk c = chunk[blockIdx.x];
	const HuAlGroup g = grp[c.g];
	const int d0 = blockIdx.y * HU_AL_DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(HU_AL_DT, (int) g.nd - d0);
	uint64_t K[HU_AL_DT]; bool act[HU_AL_DT]; uint32_t n[HU_AL_DT];
	bool any = false;
	#pragma unroll
	for(int i = 0; i < HU_AL_DT; ++i) {
		K[i] = 0; act[i] = false; n[i] = 0;
		if(i < nd) { const HuAlSel q = sel[g.draw0 + d0 + i]; K[i] = q.prefix; act[i] = q.rank != q.eq; any = any || act[i]; }
	}
	if(!any) return;                                            /* every read with a cut key is kept: their order does not matter */
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t col = smp[g.smp].col;
	uint64_t b, e;
	hu_al_span(c.t0, smp[g.smp].T, chunkLen, w, b, e);
	const uint32_t key[2] = {g.k0, g.k1};
	for(; b < e; b += 64) {
		const uint64_t t = b + lane;
		const bool valid = t < e;
		const uint64_t k = valid ? hu_otu_key(key, t, col, keyBits) : 0;
		#pragma unroll
		for(int i = 0; i < HU_AL_DT; ++i) if(act[i]) n[i] += (uint32_t) __popcll(__ballot(valid && k == K[i]));
	}
	const uint64_t at = ((uint64_t) blockIdx.x - g.chunk0) * HU_AL_WAVES + (uint64_t) w;
	#pragma unroll
	for(int i = 0; i < HU_AL_DT; ++i) if(act[i] && lane == 0) tie[draw[g.draw0 + d0 + i].tie0 + at] = n[i];
}

static __global__ __launch_bounds__(64) void k_al_tie_scan(const HuAlSample* smp, const HuAlDraw* draw, const HuAlSel* sel, uint32_t* tie, int chunkLen) {
	const int a = blockIdx.x, lane = threadIdx.x;
	const HuAlDraw d = draw[a];
	if(d.m == 0) return;
	const HuAlSel q = sel[a];
	if(q.rank == q.eq) return;
	const uint64_t n = (((uint64_t) smp[d.smp].T + (uint64_t) chunkLen - 1) / (uint64_t) chunkLen) * HU_AL_WAVES;
	uint32_t* x = tie + d.tie0;
	uint32_t carry = 0;
	for(uint64_t i0 = 0; i0 < n; i0 += 64) {
		const uint64_t i = i0 + lane;
		const uint32_t v = i < n ? x[i] : 0, incl = hu_al_wave_scan(v, lane);
		if(i < n) x[i] = carry + incl - v;
		carry += __shfl(incl, 63);
	}
}

static __global__ __launch_bounds__(HU_AL_WG) void k_al_take(const HuAlSample* smp, const HuAlGroup* grp, const HuAlChunk* chunk, const HuAlDraw* draw, const HuAlSel* sel,
		const uint32_t* tie, const uint32_t* prefix, const uint32_t* slot, uint32_t* out, int keyBits, int chunkLen) {
	const HuAlChunk c = chunk[blockIdx.x];
	const HuAlGroup g = grp[c.g];
	const int d0 = blockIdx.y * HU_AL_DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(HU_AL_DT, (int) g.nd - d0);
	const HuAlSample s = smp[g.smp];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t b, e;
	hu_al_span(c.t0, s.T, chunkLen, w, b, e);
	if(b >= e) return;
	const uint64_t at = ((uint64_t) blockIdx.x - g.chunk0) * HU_AL_WAVES + (uint64_t) w;
	uint64_t K[HU_AL_DT]; uint32_t rank[HU_AL_DT], seen[HU_AL_DT]; bool all[HU_AL_DT]; uint32_t* o[HU_AL_DT];
	#pragma unroll
	for(int i = 0; i < HU_AL_DT; ++i) {
		K[i] = 0; rank[i] = 0; seen[i] = 0; all[i] = true; o[i] = out;
		if(i < nd) {
			const HuAlSel q = sel[g.draw0 + d0 + i];
			const HuAlDraw d = draw[g.draw0 + d0 + i];
			K[i] = q.prefix; rank[i] = q.rank; all[i] = q.rank == q.eq; o[i] = out + d.cell0;
			if(!all[i]) seen[i] = tie[d.tie0 + at];            /* reads with the cut key before this span */
		}
	}
	const uint32_t *P = prefix + s.pfx0, *L = slot + (s.pfx0 - s.col);
	const uint32_t key[2] = {g.k0, g.k1};
	const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0;  /* the lanes under this one */
	uint32_t cur = hu_al_cell(P, s.nnz, (uint32_t) min(b + lane, (uint64_t) s.T - 1));
	for(; b < e; b += 64) {                                     /* lane 0 has a read in every round */
		const uint64_t t = b + lane;
		const bool valid = t < e;
		uint64_t k = ~0ull;
		if(valid) {
			while(P[cur + 1] <= (uint32_t) t) ++cur;
			k = hu_otu_key(key, t, s.col, keyBits);
		}
		/* a cell is a run of lanes: its first lane counts the kept reads of the run */
		const uint32_t prev = __shfl_up(cur, 1);
		const bool lead = valid && (lane == 0 || prev != cur);
		const uint64_t lm = __ballot(lead);
		const uint64_t above = lane == 63 ? 0 : lm >> (lane + 1);
		const int next = above ? lane + __ffsll((unsigned long long) above) : 64;
		const uint64_t run = (next == 64 ? ~0ull : (1ull << next) - 1) & ~below;
		const uint32_t to = lead ? L[cur] : 0;
		#pragma unroll
		for(int i = 0; i < HU_AL_DT; ++i) if(i < nd) {
			const bool eq = valid && k == K[i];
			const uint64_t eqm = __ballot(eq);
			const bool take = valid && (k < K[i] || (eq && (all[i] || seen[i] + (uint32_t) __popcll(eqm & below) < rank[i])));
			seen[i] += (uint32_t) __popcll(eqm);
			const uint64_t tm = __ballot(take);
			if(lead) { const uint32_t cnt = (uint32_t) __popcll(tm & run); if(cnt) atomicAdd(&o[i][to], cnt); }
		}
	}
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
		const uint32_t v = c < s.nnz ? (o[c] > 0 ? 1u : 0u) : 0u, incl = hu_al_wave_scan(v, lane);
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
