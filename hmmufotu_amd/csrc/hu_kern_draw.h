// The uniform draw without replacement on the device (hmmufotu-subset, src/OTUTable.cpp:166-209), for hu_otu_subset,
// hu_alpha and hu_unifrac_rarefied.
//
// Read t of sample j has a 64-bit key, a function of (seed, t, j) alone (hu_otu_key), and the m reads smallest in (key, t) order are
// kept.  That is a selection, done by a radix select on keys that are recomputed in every pass and never stored: device memory holds
// the prefixes of a sample's nonzero cells, one 256-bin histogram per draw and the output, nothing per read.  The kept sets of one
// (sample, key) are nested in m, so a group of draws shares every key computation: a workgroup takes one (group, chunk of reads) pair of
// the host's list and up to DT depths of the group (blockIdx.y the further ones), so one grid covers all samples however ragged their
// totals.  DT is 1 where every group has one draw (hu_otu_subset, hu_unifrac_rarefied) and 8 for hu_alpha's curves.
//   k_draw_hist      one digit (8 bits, from the top): every read whose higher digits equal the prefix found so far is counted in an LDS
//                    histogram per depth, and one integer atomic per nonempty bin per workgroup goes to the draw's histogram.
//   k_draw_pick      one wave per draw: the digit in which the wanted rank falls, the rank that is left inside that bin, the bin's
//                    size; the histogram is cleared for the next pass.  No host round trip between passes.
// After the last digit the cut key K of a draw is known, and `rank` of the `eq` reads that have exactly that key are still to be
// taken: the ones with the lowest t.  When rank == eq (always, unless keys tie) every read with key <= K is kept.  Otherwise
//   k_draw_ties      counts the reads with key K per (chunk, wave) span, and
//   k_draw_tie_scan  turns the counts of a draw into exclusive prefixes, one wave per draw,
// so that a read with key K is kept when fewer than `rank` such reads precede it: a prefix count over the ties, no serial scan.
//   k_draw_take      recomputes the keys, decides each read for every depth and counts it into the draw's copy of the sample's nonzero
//                    cells, at the cell's slot (a null slot map: in table order).  A wave takes a contiguous span of its chunk, 64
//                    consecutive reads per round; a lane finds the cell of its first read by binary search of the prefixes and walks
//                    from there.  Cells are contiguous runs of lanes, so the kept reads of a run are one population count, and the
//                    last run of a round is carried into the next: one global atomic per (wave, cell, depth), not per read.
//
// Integer atomics only: every result is a sum of counts and does not depend on the chunk, the grid or the order of arrival.  Every
// index formed here comes from arrays the host built from a checked table: prefix[cell + 1] of a valid read is read below the sample's
// last entry, which holds T; a slot is below nnz.
// Every kernel has internal linkage: each translation unit that draws keeps its own copy.
#pragma once
#include "hu_common.h"
#include "hu_otu_table.h"
#include "hu_draw.h"

__device__ inline uint32_t hu_draw_wave_scan(uint32_t v, int lane) {     /* inclusive */
	#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d); if(lane >= d) v += u; }
	return v;
}
/* the reads of wave w of the chunk that starts at t0 */
__device__ inline void hu_draw_span(uint32_t t0, uint32_t T, int chunkLen, int w, uint64_t& b, uint64_t& e) {
	const uint64_t end = min((uint64_t) t0 + (uint64_t) chunkLen, (uint64_t) T), len = end - t0, S = (len + HU_DRAW_WAVES - 1) / HU_DRAW_WAVES;
	b = min((uint64_t) t0 + (uint64_t) w * S, end); e = min(b + S, end);
}
/* the cell that owns read t: the largest c with P[c] <= t, for t < P[nnz] */
__device__ inline uint32_t hu_draw_cell(const uint32_t* P, uint32_t nnz, uint32_t t) {
	uint32_t lo = 0, hi = nnz;
	while(hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if(P[mid] <= t) lo = mid; else hi = mid; }
	return lo;
}

/* what the kernels read and write: the host's lists, the selection state, and the cells */
struct HuDrawDev {
	const HuAlSample* smp; const HuAlDraw* draw; const HuAlGroup* grp; const HuAlChunk* chunk;
	HuAlSel* sel; uint32_t *hist, *tie;                        /* [draws], [draws][256] zero between calls, 4 per (draw, chunk) */
	const uint32_t *prefix, *slot; uint32_t* out;              /* slot null: the identity */
	int keyBits, chunkLen;
};

template<int DT> static __global__ __launch_bounds__(HU_DRAW_WG) void k_draw_hist(const HuDrawDev v, int shift, int first) {
	__shared__ uint32_t h[DT][256];
	const HuAlChunk c = v.chunk[blockIdx.x];
	const HuAlGroup g = v.grp[c.g];
	const int d0 = blockIdx.y * DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(DT, (int) g.nd - d0);
	const uint32_t T = v.smp[g.smp].T, col = v.smp[g.smp].col;
	uint64_t pre[DT];
	#pragma unroll
	for(int i = 0; i < DT; ++i) { pre[i] = i < nd ? v.sel[g.draw0 + d0 + i].prefix : 0; h[i][threadIdx.x] = 0; }
	__syncthreads();
	const uint32_t key[2] = {g.k0, g.k1};
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) v.chunkLen, (uint64_t) T);
	for(uint64_t t = (uint64_t) c.t0 + threadIdx.x; t < end; t += HU_DRAW_WG) {
		const uint64_t k = hu_otu_key(key, t, col, v.keyBits);
		const uint32_t digit = (uint32_t)(k >> shift) & 255u;
		const uint64_t hi = first ? 0 : k >> (shift + 8);
		#pragma unroll
		for(int i = 0; i < DT; ++i) if(i < nd && (first || hi == pre[i])) atomicAdd(&h[i][digit], 1u);
	}
	__syncthreads();
	#pragma unroll
	for(int i = 0; i < DT; ++i) if(i < nd) {
		const uint32_t n = h[i][threadIdx.x];
		if(n) atomicAdd(&v.hist[(size_t)(g.draw0 + d0 + i) * 256 + threadIdx.x], n);
	}
}

static __global__ __launch_bounds__(64) void k_draw_pick(const HuAlDraw* draw, HuAlSel* sel, uint32_t* hist) {
	const int a = blockIdx.x, lane = threadIdx.x;
	if(draw[a].m == 0) return;
	uint4* h4 = (uint4*)(hist + (size_t) a * 256);
	const uint4 v = h4[lane];
	h4[lane] = make_uint4(0, 0, 0, 0);
	const HuAlSel s = sel[a];
	const uint32_t sum = v.x + v.y + v.z + v.w, incl = hu_draw_wave_scan(sum, lane);
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

template<int DT> static __global__ __launch_bounds__(HU_DRAW_WG) void k_draw_ties(const HuDrawDev v) {
	const HuAlChunk c = v.chunk[blockIdx.x];
	const HuAlGroup g = v.grp[c.g];
	const int d0 = blockIdx.y * DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(DT, (int) g.nd - d0);
	uint64_t K[DT]; bool act[DT]; uint32_t n[DT];
	bool any = false;
	#pragma unroll
	for(int i = 0; i < DT; ++i) {
		K[i] = 0; act[i] = false; n[i] = 0;
		if(i < nd) { const HuAlSel q = v.sel[g.draw0 + d0 + i]; K[i] = q.prefix; act[i] = q.rank != q.eq; any = any || act[i]; }
	}
	if(!any) return;                                            /* every read with a cut key is kept: their order does not matter */
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t col = v.smp[g.smp].col;
	uint64_t b, e;
	hu_draw_span(c.t0, v.smp[g.smp].T, v.chunkLen, w, b, e);
	const uint32_t key[2] = {g.k0, g.k1};
	for(; b < e; b += 64) {
		const uint64_t t = b + lane;
		const bool valid = t < e;
		const uint64_t k = valid ? hu_otu_key(key, t, col, v.keyBits) : 0;
		#pragma unroll
		for(int i = 0; i < DT; ++i) if(act[i]) n[i] += (uint32_t) __popcll(__ballot(valid && k == K[i]));
	}
	const uint64_t at = ((uint64_t) blockIdx.x - g.chunk0) * HU_DRAW_WAVES + (uint64_t) w;
	#pragma unroll
	for(int i = 0; i < DT; ++i) if(act[i] && lane == 0) v.tie[v.draw[g.draw0 + d0 + i].tie0 + at] = n[i];
}

static __global__ __launch_bounds__(64) void k_draw_tie_scan(const HuAlSample* smp, const HuAlDraw* draw, const HuAlSel* sel, uint32_t* tie, int chunkLen) {
	const int a = blockIdx.x, lane = threadIdx.x;
	const HuAlDraw d = draw[a];
	if(d.m == 0) return;
	const HuAlSel q = sel[a];
	if(q.rank == q.eq) return;
	const uint64_t n = (((uint64_t) smp[d.smp].T + (uint64_t) chunkLen - 1) / (uint64_t) chunkLen) * HU_DRAW_WAVES;
	uint32_t* x = tie + d.tie0;
	uint32_t carry = 0;
	for(uint64_t i0 = 0; i0 < n; i0 += 64) {
		const uint64_t i = i0 + lane;
		const uint32_t v = i < n ? x[i] : 0, incl = hu_draw_wave_scan(v, lane);
		if(i < n) x[i] = carry + incl - v;
		carry += __shfl(incl, 63);
	}
}

template<int DT> static __global__ __launch_bounds__(HU_DRAW_WG) void k_draw_take(const HuDrawDev v) {
	const HuAlChunk c = v.chunk[blockIdx.x];
	const HuAlGroup g = v.grp[c.g];
	const int d0 = blockIdx.y * DT;
	if(d0 >= (int) g.nd) return;
	const int nd = min(DT, (int) g.nd - d0);
	const HuAlSample s = v.smp[g.smp];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t b, e;
	hu_draw_span(c.t0, s.T, v.chunkLen, w, b, e);
	if(b >= e) return;
	const uint64_t at = ((uint64_t) blockIdx.x - g.chunk0) * HU_DRAW_WAVES + (uint64_t) w;
	uint64_t K[DT]; uint32_t rank[DT], seen[DT], carry[DT]; bool all[DT]; uint32_t* o[DT];
	#pragma unroll
	for(int i = 0; i < DT; ++i) {
		K[i] = 0; rank[i] = 0; seen[i] = 0; carry[i] = 0; all[i] = true; o[i] = v.out;
		if(i < nd) {
			const HuAlSel q = v.sel[g.draw0 + d0 + i];
			const HuAlDraw d = v.draw[g.draw0 + d0 + i];
			K[i] = q.prefix; rank[i] = q.rank; all[i] = q.rank == q.eq; o[i] = v.out + d.cell0;
			if(!all[i]) seen[i] = v.tie[d.tie0 + at];             /* reads with the cut key before this span */
		}
	}
	const uint32_t *P = v.prefix + s.pfx0, *L = v.slot ? v.slot + (s.pfx0 - s.col) : nullptr;
	const uint32_t key[2] = {g.k0, g.k1};
	const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0;  /* the lanes under this one */
	uint32_t cur = hu_draw_cell(P, s.nnz, (uint32_t) min(b + lane, (uint64_t) s.T - 1));
	uint32_t carryTo = 0xffffffffu;                             /* the slot of the round before's last run, whose counts carry[] are not yet added */
	for(; b < e; b += 64) {                                     /* lane 0 has a read in every round */
		const uint64_t t = b + lane;
		const bool valid = t < e;
		uint64_t k = ~0ull;
		if(valid) {
			while(P[cur + 1] <= (uint32_t) t) ++cur;
			k = hu_otu_key(key, t, s.col, v.keyBits);
		}
		/* a cell is a run of lanes: its first lane counts the kept reads of the run */
		const uint32_t prev = __shfl_up(cur, 1);
		const bool lead = valid && (lane == 0 || prev != cur);
		const uint64_t lm = __ballot(lead);
		const uint64_t above = lane == 63 ? 0 : lm >> (lane + 1);
		const int next = above ? lane + __ffsll((unsigned long long) above) : 64;
		const uint64_t run = (next == 64 ? ~0ull : (1ull << next) - 1) & ~below;
		const uint32_t to = lead ? (L ? L[cur] : cur) : 0;
		const int last = 63 - __clzll((long long) lm);
		const bool flush = (uint32_t) __shfl(to, 0) != carryTo;   /* this round begins in another cell than the one before ended in */
		#pragma unroll
		for(int i = 0; i < DT; ++i) if(DT == 1 || i < nd) {
			const bool eq = valid && k == K[i];
			const uint64_t eqm = __ballot(eq);
			const bool take = valid && (k < K[i] || (eq && (all[i] || seen[i] + (uint32_t) __popcll(eqm & below) < rank[i])));
			seen[i] += (uint32_t) __popcll(eqm);
			const uint64_t tm = __ballot(take);
			if(flush) { if(lane == 0 && carry[i]) atomicAdd(&o[i][carryTo], carry[i]); carry[i] = 0; }
			const uint32_t cnt = lead ? (uint32_t) __popcll(tm & run) + (lane == 0 ? carry[i] : 0) : 0;
			if(above && cnt) atomicAdd(&o[i][to], cnt);          /* cnt != 0: a lead lane; above: not the round's last run, which is carried */
			carry[i] = __shfl(cnt, last);
		}
		carryTo = __shfl(to, last);
	}
	#pragma unroll
	for(int i = 0; i < DT; ++i) if(lane == 0 && carry[i]) atomicAdd(&o[i][carryTo], carry[i]);
}

/* the launches of a draw, in two parts so that a caller can time them apart and set its whole samples in between.  nDraw draws from
 * sel[0] on, nChunk chunks, groups of maxNd draws at the most; v.hist is zero on entry and on return */
#define HU_DRAW_TRY(launch) do { launch; const hipError_t e_ = hipGetLastError(); if(e_ != hipSuccess) return e_; } while(0)
template<int DT> static hipError_t hu_draw_select(const HuDrawDev& v, unsigned nDraw, unsigned nChunk, unsigned maxNd) {
	if(nChunk == 0) return hipSuccess;
	const dim3 grid(nChunk, (maxNd + DT - 1) / DT);
	const int passes = (v.keyBits + 7) / 8;                     /* the key is below 2^key_bits: its top digit may be a short one */
	for(int p = 0; p < passes; ++p) {
		HU_DRAW_TRY((k_draw_hist<DT><<<grid, HU_DRAW_WG>>>(v, 8 * (passes - 1 - p), p == 0)));
		HU_DRAW_TRY((k_draw_pick<<<nDraw, 64>>>(v.draw, v.sel, v.hist)));
	}
	HU_DRAW_TRY((k_draw_ties<DT><<<grid, HU_DRAW_WG>>>(v)));
	HU_DRAW_TRY((k_draw_tie_scan<<<nDraw, 64>>>(v.smp, v.draw, v.sel, v.tie, v.chunkLen)));
	return hipSuccess;
}
#undef HU_DRAW_TRY
template<int DT> static hipError_t hu_draw_take(const HuDrawDev& v, unsigned nChunk, unsigned maxNd) {
	if(nChunk == 0) return hipSuccess;
	k_draw_take<DT><<<dim3(nChunk, (maxNd + DT - 1) / DT), HU_DRAW_WG>>>(v);
	return hipGetLastError();
}
