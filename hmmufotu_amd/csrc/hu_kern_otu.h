// Rarefying every sample of an OTU table on the device (hmmufotu-subset, src/OTUTable.cpp:166-209).
//
// Uniform, without replacement: read t of sample j has a 64-bit key, a function of (seed, t, j) alone (hu_otu_key), and the `size` reads
// smallest in (key, t) order are kept.  That is a selection, done by a radix select on keys that are recomputed in every pass and never
// stored: device memory holds the prefixes of a sample's nonzero cells, one 256-bin histogram per sample and the output, nothing per read.
//   k_otu_hist   one digit (8 bits, from the top): a workgroup takes one (sample, chunk of reads) pair of the host's chunk list, so one
//                grid covers all samples however ragged their totals; every read whose higher digits equal the prefix found so far is
//                counted in an LDS histogram, and one integer atomic per nonempty bin per workgroup goes to the sample's histogram.
//   k_otu_pick   one wave per sample: the digit in which the wanted rank falls, the rank that is left inside that bin, the bin's size;
//                the histogram is cleared for the next pass.  No host round trip between passes.
// After the last digit the cut key K of a sample is known, and `rank` of the `eq` reads that have exactly that key are still to be
// taken: the ones with the lowest t.  When rank == eq (always, unless keys tie) every read with key <= K is kept.  Otherwise
//   k_otu_ties      counts the reads with key K per (chunk, wave) span, and
//   k_otu_tie_scan  turns the counts of a sample into exclusive prefixes, one wave per sample,
// so that a read with key K is kept when fewer than `rank` such reads precede it: a prefix count over the ties, no serial scan.
//   k_otu_take   recomputes the keys, decides each read and counts it for the OTU that owns it.  A wave takes a contiguous span of its
//                chunk, 64 consecutive reads per round; a lane finds the cell of its first read by binary search of the prefixes and
//                walks from there.  Cells are contiguous runs of lanes, so the kept reads of a run are one population count, and the
//                last run of a round is carried into the next: one global atomic per (wave, cell), not per read.
// Multinomial, with replacement (k_otu_multinom): a lane per draw; the read it names (hu_otu_draw) is looked up by binary search.
//
// Integer atomics only: every result is a sum of counts and does not depend on the chunk, the grid or the order of arrival.  Every
// index formed here comes from arrays the host built (hu_otu_subset.cpp) from a checked table: prefix[cell + 1] of a valid read is read
// below the sample's last entry, which holds T.
#pragma once
#include "hu_common.h"
#include "hu_otu_table.h"

#define HU_OTU_WG 256
#define HU_OTU_WAVES 4

struct HuOtuSample {
	uint64_t cell0;            /* the first of its nonzero cells in out[] */
	uint64_t pfx0;             /* the first of its nnz + 1 prefixes in prefix[]: P[c] = reads before cell c, P[nnz] = T */
	uint64_t chunk0;           /* the first of its chunks in the chunk list */
	uint32_t nnz, T, col, nChunk;
};
struct HuOtuSel { uint64_t prefix; uint32_t rank, eq; };     /* digits found so far; reads still wanted among the `eq` that carry them */
struct HuOtuChunk { uint32_t a, t0; };                      /* active sample, first read (first draw) */

/* the reads of wave w of a chunk */
__device__ inline void hu_otu_span(const HuOtuChunk& c, uint32_t T, int chunkLen, int w, uint64_t& b, uint64_t& e) {
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) chunkLen, (uint64_t) T), len = end - c.t0, S = (len + HU_OTU_WAVES - 1) / HU_OTU_WAVES;
	b = min((uint64_t) c.t0 + (uint64_t) w * S, end); e = min(b + S, end);
}
/* the cell that owns read t: the largest c with P[c] <= t, for t < P[nnz] */
__device__ inline uint32_t hu_otu_cell(const uint32_t* P, uint32_t nnz, uint32_t t) {
	uint32_t lo = 0, hi = nnz;
	while(hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if(P[mid] <= t) lo = mid; else hi = mid; }
	return lo;
}
__device__ inline uint32_t hu_otu_wave_scan(uint32_t v, int lane) {     /* inclusive */
	#pragma unroll
	for(int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d); if(lane >= d) v += u; }
	return v;
}

__global__ __launch_bounds__(HU_OTU_WG) void k_otu_hist(const HuOtuSample* smp, const HuOtuChunk* chunk, const HuOtuSel* sel, uint32_t* hist,
		uint32_t k0, uint32_t k1, int keyBits, int chunkLen, int shift, int first) {
	__shared__ uint32_t h[256];
	const HuOtuChunk c = chunk[blockIdx.x];
	const uint32_t T = smp[c.a].T, col = smp[c.a].col;
	const uint64_t pre = sel[c.a].prefix;
	h[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t key[2] = {k0, k1};
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) chunkLen, (uint64_t) T);
	for(uint64_t t = (uint64_t) c.t0 + threadIdx.x; t < end; t += HU_OTU_WG) {
		const uint64_t k = hu_otu_key(key, t, col, keyBits);
		if(first || (k >> (shift + 8)) == pre) atomicAdd(&h[(k >> shift) & 255], 1u);
	}
	__syncthreads();
	const uint32_t v = h[threadIdx.x];
	if(v) atomicAdd(&hist[(size_t) c.a * 256 + threadIdx.x], v);
}

__global__ __launch_bounds__(64) void k_otu_pick(HuOtuSel* sel, uint32_t* hist) {
	const int a = blockIdx.x, lane = threadIdx.x;
	uint4* h4 = (uint4*)(hist + (size_t) a * 256);
	const uint4 v = h4[lane];
	h4[lane] = make_uint4(0, 0, 0, 0);
	const HuOtuSel s = sel[a];
	const uint32_t sum = v.x + v.y + v.z + v.w, incl = hu_otu_wave_scan(sum, lane);
	uint32_t cum = incl - sum;                                 /* reads in the bins below this lane's four */
	/* the bins hold the s.eq reads that carry the prefix, and 1 <= rank <= eq: exactly one lane has cum < rank <= incl */
	if(cum < s.rank && s.rank <= incl) {
		const uint32_t b[4] = {v.x, v.y, v.z, v.w};
		int d = 0;
		while(d < 3 && cum + b[d] < s.rank) { cum += b[d]; ++d; }
		HuOtuSel n;
		n.prefix = (s.prefix << 8) | (uint64_t)(lane * 4 + d); n.rank = s.rank - cum; n.eq = b[d];
		sel[a] = n;
	}
}

__global__ __launch_bounds__(HU_OTU_WG) void k_otu_ties(const HuOtuSample* smp, const HuOtuChunk* chunk, const HuOtuSel* sel, uint32_t* tie,
		uint32_t k0, uint32_t k1, int keyBits, int chunkLen) {
	const HuOtuChunk c = chunk[blockIdx.x];
	const HuOtuSel q = sel[c.a];
	if(q.rank == q.eq) return;                                 /* every read with the cut key is kept: their order does not matter */
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t col = smp[c.a].col;
	uint64_t b, e;
	hu_otu_span(c, smp[c.a].T, chunkLen, w, b, e);
	const uint32_t key[2] = {k0, k1};
	uint32_t n = 0;
	for(; b < e; b += 64) {
		const uint64_t t = b + lane;
		n += __popcll(__ballot(t < e && hu_otu_key(key, t, col, keyBits) == q.prefix));
	}
	if(lane == 0) tie[(size_t) blockIdx.x * HU_OTU_WAVES + w] = n;
}

__global__ __launch_bounds__(64) void k_otu_tie_scan(const HuOtuSample* smp, const HuOtuSel* sel, uint32_t* tie) {
	const int a = blockIdx.x, lane = threadIdx.x;
	const HuOtuSel q = sel[a];
	if(q.rank == q.eq) return;
	const uint64_t n = (uint64_t) smp[a].nChunk * HU_OTU_WAVES;
	uint32_t* x = tie + smp[a].chunk0 * HU_OTU_WAVES;
	uint32_t carry = 0;
	for(uint64_t i0 = 0; i0 < n; i0 += 64) {
		const uint64_t i = i0 + lane;
		const uint32_t v = i < n ? x[i] : 0, incl = hu_otu_wave_scan(v, lane);
		if(i < n) x[i] = carry + incl - v;
		carry += __shfl(incl, 63);
	}
}

__global__ __launch_bounds__(HU_OTU_WG) void k_otu_take(const HuOtuSample* smp, const HuOtuChunk* chunk, const HuOtuSel* sel, const uint32_t* tie,
		const uint32_t* prefix, uint32_t* out, uint32_t k0, uint32_t k1, int keyBits, int chunkLen) {
	const HuOtuChunk c = chunk[blockIdx.x];
	const HuOtuSample s = smp[c.a];
	const HuOtuSel q = sel[c.a];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t b, e;
	hu_otu_span(c, s.T, chunkLen, w, b, e);
	if(b >= e) return;
	const bool all = q.rank == q.eq;
	uint32_t seen = all ? 0 : tie[(size_t) blockIdx.x * HU_OTU_WAVES + w];     /* reads with the cut key before this span */
	const uint32_t* P = prefix + s.pfx0;
	uint32_t* o = out + s.cell0;
	const uint32_t key[2] = {k0, k1};
	const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0;                 /* the lanes under this one */
	uint32_t cur = hu_otu_cell(P, s.nnz, (uint32_t) min(b + lane, (uint64_t) s.T - 1));
	uint32_t carryCell = 0xffffffffu, carryCnt = 0;                           /* the last cell of the round before, not yet added */
	for(; b < e; b += 64) {                                                    /* lane 0 has a read in every round */
		const uint64_t t = b + lane;
		const bool valid = t < e;
		uint64_t k = ~0ull;
		if(valid) {
			while(P[cur + 1] <= (uint32_t) t) ++cur;
			k = hu_otu_key(key, t, s.col, keyBits);
		}
		const bool eq = valid && k == q.prefix;
		const uint64_t eqm = __ballot(eq);
		const bool take = valid && (k < q.prefix || (eq && (all || seen + (uint32_t) __popcll(eqm & below) < q.rank)));
		seen += (uint32_t) __popcll(eqm);
		/* a cell is a run of lanes: its first lane counts the kept reads of the run */
		const uint32_t prev = __shfl_up(cur, 1);
		const bool lead = valid && (lane == 0 || prev != cur);
		const uint64_t lm = __ballot(lead), tm = __ballot(take);
		if((uint32_t) __shfl(cur, 0) != carryCell) { if(lane == 0 && carryCnt) atomicAdd(&o[carryCell], carryCnt); carryCnt = 0; }
		uint32_t cnt = 0;
		if(lead) {
			const uint64_t above = lane == 63 ? 0 : lm >> (lane + 1);
			const int next = above ? lane + __ffsll((unsigned long long) above) : 64;
			const uint64_t run = (next == 64 ? ~0ull : (1ull << next) - 1) & ~below;
			cnt = (uint32_t) __popcll(tm & run) + (lane == 0 ? carryCnt : 0);
			if(above && cnt) atomicAdd(&o[cur], cnt);
		}
		const int last = 63 - __clzll((long long) lm);
		carryCell = __shfl(cur, last); carryCnt = __shfl(cnt, last);
	}
	if(lane == 0 && carryCnt) atomicAdd(&o[carryCell], carryCnt);
}

__global__ __launch_bounds__(HU_OTU_WG) void k_otu_multinom(const HuOtuSample* smp, const HuOtuChunk* chunk, const uint32_t* prefix, uint32_t* out,
		uint32_t k0, uint32_t k1, int chunkLen, uint32_t size) {
	const HuOtuChunk c = chunk[blockIdx.x];
	const HuOtuSample s = smp[c.a];
	const int lane = threadIdx.x & 63;
	const uint32_t* P = prefix + s.pfx0;
	uint32_t* o = out + s.cell0;
	const uint32_t key[2] = {k0, k1};
	const uint64_t end = min((uint64_t) c.t0 + (uint64_t) chunkLen, (uint64_t) size);
	for(uint64_t base = c.t0; base < end; base += HU_OTU_WG) {
		const uint64_t m = base + threadIdx.x;
		const bool valid = m < end;
		uint32_t cell = 0xffffffffu;
		if(valid) cell = hu_otu_cell(P, s.nnz, (uint32_t) hu_otu_draw(key, m, s.col, s.T));
		/* a wave whose draws all fall into one cell (a sample that one OTU holds) adds once */
		const uint64_t vm = __ballot(valid);
		if(!vm) continue;
		const int firstLane = __ffsll((unsigned long long) vm) - 1;
		const uint32_t c0 = __shfl(cell, firstLane);
		if(__ballot(valid && cell == c0) == vm) { if(lane == firstLane) atomicAdd(&o[c0], (uint32_t) __popcll(vm)); }
		else if(valid) atomicAdd(&o[cell], 1u);
	}
}
