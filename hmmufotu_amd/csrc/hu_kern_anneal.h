// HIP kernels of the primer scan of hmmufotu-anneal (gfx950, wave64).  Included by hu_engine.hip.
//
//   k_anneal_masks  the chosen alignment row of each primer -> accept masks in SCAN ORDER over the quads its region touches
//   k_anneal_scan   SeqUtils::pDist(aln.align, node seq, csStart - 1, csEnd - 1) <= maxDist for every node
//                   (src/hmmufotu-anneal.cpp:270-277, src/SeqUtils.cpp:77-85), summed into hit counts of nodes and leaves
//
// The match rule is DegenAlphabet::isMatch(char, int8_t) (src/DegenAlphabet.cpp:70-76): an alignment character accepts a set of the
// six node codes {A, C, G, T, gap (-2), invalid (-1)}, hu_anneal_accept below.  The denominator of the distance is the region's length
// (every column counts, gaps included), so a node is a hit when its mismatch count is at most a per-primer integer threshold
// computed on the host with the reference's own double expression (hu_anneal_max_mismatch).
#pragma once
#include "hu_common.h"

#define HU_ANNEAL_TILE 8      /* primers per workgroup: wave-uniform, their masks come in through the scalar cache */
#define HU_ANNEAL_PLANES 7    /* accept A, C, G, T, gap, invalid; region */

/* the accept set of alignment character c: bit 0..3 = node code 0..3, bit 4 = node code -2 (gap), bit 5 = node code -1 (invalid).
 * encode(c) is the IUPACNucl sym_map (a degenerate letter encodes as the first base of its expansion), and the expansion adds the
 * rest.  Lower-case letters (the inserts buildGlobalAlign writes, src/BandedHMMP7.cpp:1046) and every other byte encode to -1.  The
 * reference indexes its 128-entry sym_map with a signed char, so bytes >= 128 are undefined there; they count as invalid here. */
__host__ __device__ inline uint32_t hu_anneal_accept(unsigned char c) {
	switch(c) {
	case 'A': return 0x01; case 'C': return 0x02; case 'G': return 0x04; case 'T': case 'U': return 0x08;
	case 'M': return 0x03; case 'R': return 0x05; case 'W': return 0x09; case 'S': return 0x06; case 'Y': return 0x0a; case 'K': return 0x0c;
	case 'V': return 0x07; case 'H': return 0x0b; case 'D': return 0x0d; case 'B': return 0x0e; case 'N': return 0x0f;
	case '-': case '.': case '_': return 0x10;
	default: return 0x20;
	}
}

/* (m & a) | (~m & b), one v_bfi_b32 */
__device__ inline uint32_t hu_bsel(uint32_t m, uint32_t a, uint32_t b) { return (m & a) | (~m & b); }

/* Masks of one tile of primers over the quads its regions touch, quads listed per tile as
 *     tileQ[tile * (WQ + 2) + {0: first mask quad of the tile, 1: nq, 2 ..: the quads}]
 *     masks[((tileQ[.. + 0] + qi) * T + t) * 32 + p * 4 + w]        p = plane (HU_ANNEAL_PLANES), w = word of the quad
 * Grid (tiles, most quads of any tile), 128 threads: a thread owns one scan position of the quad. */
__global__ __launch_bounds__(128) void k_anneal_masks(HuDbDev db, const char* __restrict__ rows, const int32_t* __restrict__ rowOf,
		const int2* __restrict__ region, int n, const int32_t* __restrict__ tileQ, uint32_t* __restrict__ masks) {
	constexpr int T = HU_ANNEAL_TILE;
	const int tile = blockIdx.x, qi = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
	const int32_t* tq = tileQ + (size_t) tile * (db.WQ + 2);
	if(qi >= tq[1]) return;
	const int q = tq[2 + qi];
	const int c = db.posCol[(size_t) q * 128 + tid];
	uint32_t* __restrict__ out = masks + (size_t)(tq[0] + qi) * T * 32;
	for(int t = 0; t < T; ++t) {
		const int s = tile * T + t;
		const int row = s < n ? rowOf[s] : -1;
		bool in = false;
		uint32_t acc = 0;
		if(row >= 0 && c >= 0) {
			const int2 rg = region[s];
			in = c >= rg.x && c <= rg.y;
			if(in) acc = hu_anneal_accept((unsigned char) rows[(size_t) row * db.csLen + c]);
		}
		for(int p = 0; p < HU_ANNEAL_PLANES; ++p) {
			const unsigned long long m = __ballot(p < 6 ? ((acc >> p) & 1u) : in);
			if(lane == 0) {
				uint32_t* o = out + (size_t) t * 32 + p * 4 + (tid >> 6) * 2;
				o[0] = (uint32_t) m; o[1] = (uint32_t)(m >> 32);
			}
		}
	}
}

/* One lane per node, HU_ANNEAL_TILE primers per workgroup.  Per (node, primer, 32 sites): the node's code class from its planes
 * (b0, b1 = base code, v = is a base; inv = code -1 where the database has such codes, else v = 0 is a gap) selects the accept mask
 * of its class, and the mismatches are the region bits that it leaves out: 5 bit-selects, an and-not and a population count.
 * Grid: x = primer tile (fastest: consecutive workgroups re-use one node block from L2, as in k_seed_pdist2), y = node block of 256.
 * hits[s * 2 + {0: nodes, 1: leaves}] takes one atomic per wave and primer. */
template<bool INV>
__global__ __launch_bounds__(256) void k_anneal_scan(HuDbDev db, const uint4* __restrict__ invPlane, const unsigned long long* __restrict__ leafMask,
		const uint32_t* __restrict__ masks, const int32_t* __restrict__ tileQ, const int32_t* __restrict__ thr, int n,
		unsigned long long* __restrict__ hits) {
	constexpr int T = HU_ANNEAL_TILE;
	const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
	const int node = blockIdx.y * 256 + tid;
	const int32_t* tq = tileQ + (size_t) tile * (db.WQ + 2);
	const int m0 = tq[0], nq = tq[1];
	const size_t np = (size_t) db.nNodesPad;
	uint32_t d[T];
#pragma unroll
	for(int t = 0; t < T; ++t) d[t] = 0;
	for(int qi = 0; qi < nq; ++qi) {
		const int q = tq[2 + qi];
		const uint4 p0 = db.planes[((size_t) q * 3 + 0) * np + node], p1 = db.planes[((size_t) q * 3 + 1) * np + node], pv = db.planes[((size_t) q * 3 + 2) * np + node];
		const uint4 pi = INV ? invPlane[(size_t) q * np + node] : make_uint4(0, 0, 0, 0);
		const uint32_t b0[4] = {p0.x, p0.y, p0.z, p0.w}, b1[4] = {p1.x, p1.y, p1.z, p1.w}, v[4] = {pv.x, pv.y, pv.z, pv.w}, iv[4] = {pi.x, pi.y, pi.z, pi.w};
		const uint32_t* __restrict__ m = masks + (size_t)(m0 + qi) * T * 32;
#pragma unroll
		for(int t = 0; t < T; ++t) {
			const uint32_t* mt = m + t * 32;
#pragma unroll
			for(int w = 0; w < 4; ++w) {
				const uint32_t lo = hu_bsel(b0[w], mt[4 + w], mt[w]);             /* b1 = 0: C if b0 else A */
				const uint32_t hi = hu_bsel(b0[w], mt[12 + w], mt[8 + w]);        /* b1 = 1: T if b0 else G */
				const uint32_t base = hu_bsel(b1[w], hi, lo);
				const uint32_t none = INV ? hu_bsel(iv[w], mt[20 + w], mt[16 + w]) : mt[16 + w];
				const uint32_t match = hu_bsel(v[w], base, none);
				d[t] += __popc(mt[24 + w] & ~match);
			}
		}
	}
	const bool real = node < db.nNodes;
	const bool leaf = real && ((leafMask[node >> 6] >> lane) & 1ull);
#pragma unroll
	for(int t = 0; t < T; ++t) {
		const int s = tile * T + t;
		if(s >= n) break;
		const bool hit = real && (int32_t) d[t] <= thr[s];
		const unsigned long long bh = __ballot(hit), bl = __ballot(hit && leaf);
		if(lane == 0 && bh) {
			atomicAdd(&hits[(size_t) s * 2], (unsigned long long) __popcll(bh));
			if(bl) atomicAdd(&hits[(size_t) s * 2 + 1], (unsigned long long) __popcll(bl));
		}
	}
}
