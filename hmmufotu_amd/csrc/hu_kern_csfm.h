// Kernels behind the .csfm writer: the suffix array of the concatenated text by prefix doubling over a hand-written
// least-significant-digit radix sort of (64-bit key, 32-bit position) pairs, and the pass that reads the BWT, the sample marks and the
// sampled suffix-array values off it (CSFMIndex::buildBWT, src/CSFMIndex.cpp:327-368).  gfx950, wave64.
//
// The sort.  One pass orders the pairs by one 8-bit digit of the key and keeps the order they had (stable), so the passes from the lowest
// digit up order them by the whole key.  A TILE is HU_SA_TILE consecutive pairs and belongs to ONE WAVE, which walks it in rows of 64:
//   k_sa_hist     the tile's count of every digit value, filed digit-major: hist[digit * nTiles + tile];
//   k_sa_scan_*   one exclusive scan of that array: hist[digit * nTiles + tile] becomes the first output slot of the tile's pairs with that
//                 digit — behind every smaller digit of every tile and the same digit of every earlier tile;
//   k_sa_scatter  the tile's 256 cursors start at those slots; row after row, a pair goes to its digit's cursor plus the number of
//                 lanes below it in the row with the same digit, and the lowest such lane moves the cursor past the row's share.
// The place of a pair inside its digit is therefore its order in the tile — rows in order, lanes in order, found with ballots — and never
// the arrival order of an atomic; the kernels hold no atomic at all.  A wave owns its cursors (1 KiB of LDS), so no barrier between waves
// is needed either: a row costs eight ballots, one LDS read-modify-write on the leaders and one shuffle.
#pragma once
#include "hu_common.h"

#define HU_SA_TILE 4096          /* pairs per wave tile: 64 rows of 64 */
#define HU_SA_H0 21              /* symbols in the round-0 key, 3 bits each */

/* the place of this lane's pair among the pairs of its digit met so far by the wave: cnt[d] (LDS, this wave's 256 cursors) before the
 * row, plus the lanes below this one in the row that hold the same digit.  Moves cnt[d] past the row.  Called by all 64 lanes. */
__device__ inline uint32_t sa_digit_place(uint32_t d, bool valid, uint32_t* cnt) {
	const int lane = threadIdx.x & 63;
	unsigned long long m = __ballot(valid);
#pragma unroll
	for(int b = 0; b < 8; ++b) {
		const bool bit = (d >> b) & 1u;
		const unsigned long long bal = __ballot(bit);
		m &= bit ? bal : ~bal;
	}
	const unsigned long long below = m & ((1ull << lane) - 1ull);
	const bool leader = valid && below == 0;
	uint32_t base = 0;
	if(leader) { base = cnt[d]; cnt[d] = base + (uint32_t) __popcll(m); }      /* the leaders of a row hold distinct digits */
	__builtin_amdgcn_wave_barrier();
	__threadfence_block();
	base = __shfl(base, valid ? __ffsll((long long) m) - 1 : lane);
	return base + (uint32_t) __popcll(below);
}

__global__ __launch_bounds__(256) void k_sa_hist(const uint64_t* __restrict__ key, size_t n, int shift, uint32_t nTiles, uint32_t* __restrict__ hist) {
	__shared__ uint32_t cnt[4][256];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const size_t tile = (size_t) blockIdx.x * 4 + wave;
	if(tile >= nTiles) return;                                   /* wave-uniform; no workgroup barrier below */
	uint32_t* c = cnt[wave];
	for(int d = lane; d < 256; d += 64) c[d] = 0;
	__builtin_amdgcn_wave_barrier();
	__threadfence_block();
	const size_t base = tile * HU_SA_TILE;
	for(int r = 0; r < HU_SA_TILE / 64; ++r) {
		const size_t i = base + (size_t) r * 64 + lane;
		if(base + (size_t) r * 64 >= n) break;
		const bool valid = i < n;
		const uint32_t d = valid ? (uint32_t)(key[i] >> shift) & 255u : 0u;
		(void) sa_digit_place(d, valid, c);
	}
	__builtin_amdgcn_wave_barrier();
	__threadfence_block();
	for(int d = lane; d < 256; d += 64) hist[(size_t) d * nTiles + tile] = c[d];
}

__global__ __launch_bounds__(256) void k_sa_scatter(const uint64_t* __restrict__ key, const uint32_t* __restrict__ pos, size_t n, int shift, uint32_t nTiles,
		const uint32_t* __restrict__ start, uint64_t* __restrict__ keyOut, uint32_t* __restrict__ posOut) {
	__shared__ uint32_t cnt[4][256];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const size_t tile = (size_t) blockIdx.x * 4 + wave;
	if(tile >= nTiles) return;
	uint32_t* c = cnt[wave];
	for(int d = lane; d < 256; d += 64) c[d] = start[(size_t) d * nTiles + tile];
	__builtin_amdgcn_wave_barrier();
	__threadfence_block();
	const size_t base = tile * HU_SA_TILE;
	for(int r = 0; r < HU_SA_TILE / 64; ++r) {
		const size_t i = base + (size_t) r * 64 + lane;
		if(base + (size_t) r * 64 >= n) break;
		const bool valid = i < n;
		const uint64_t k = valid ? key[i] : 0ull;
		const uint32_t p = valid ? pos[i] : 0u;
		const uint32_t at = sa_digit_place((uint32_t)(k >> shift) & 255u, valid, c);
		if(valid && at < n) { keyOut[at] = k; posOut[at] = p; }  /* at < n holds by construction: the cursors are an exclusive scan of counts that sum to n */
	}
}

/* ---- scans over m counters (m < 2^32, sums < 2^32), tiles of 1,024, in the shape of cs_block_scan (hu_kern_rank.h): the tiles' sums, their
 * exclusive scan by one workgroup (the grand total goes to tileSum[nTiles]), every tile scanned behind its offset */
__device__ inline uint32_t sa_block_scan(uint32_t v, uint32_t* wsum /* LDS [16] */, uint32_t& total) { /* inclusive, 1,024 threads */
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
	for(int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(v, o); if(lane >= o) v += t; }
	if(lane == 63) wsum[wave] = v;
	__syncthreads();
	uint32_t before = 0, tot = 0;
#pragma unroll
	for(int w = 0; w < 16; ++w) { const uint32_t t = wsum[w]; if(w < wave) before += t; tot += t; }
	total = tot;
	__syncthreads();
	return v + before;
}
__global__ __launch_bounds__(1024) void k_sa_scan_sums(size_t m, const uint32_t* __restrict__ v, uint32_t* __restrict__ tileSum) {
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	uint32_t tot;
	(void) sa_block_scan(i < m ? v[i] : 0u, wsum, tot);
	if(threadIdx.x == 0) tileSum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_sa_scan_tiles(size_t nTiles, uint32_t* __restrict__ tileSum /* [nTiles + 1] */) {
	__shared__ uint32_t wsum[16];
	uint32_t carry = 0;
	for(size_t base = 0; base < nTiles; base += 1024) {
		const size_t i = base + threadIdx.x;
		const uint32_t v = i < nTiles ? tileSum[i] : 0u;
		uint32_t tot;
		const uint32_t inc = sa_block_scan(v, wsum, tot);
		if(i < nTiles) tileSum[i] = carry + inc - v;
		carry += tot;
	}
	if(threadIdx.x == 0) tileSum[nTiles] = carry;
}
__global__ __launch_bounds__(1024) void k_sa_scan_apply(size_t m, uint32_t* __restrict__ v, const uint32_t* __restrict__ tileOff) { /* exclusive, in place */
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	const uint32_t x = i < m ? v[i] : 0u;
	uint32_t tot;
	const uint32_t inc = sa_block_scan(x, wsum, tot);
	if(i < m) v[i] = tileOff[blockIdx.x] + inc - x;
}

/* ---- prefix doubling.  Round 0: the first HU_SA_H0 symbols of every suffix in one key, symbol s as s + 1 and 0 beyond the end of the
 * text, so that a suffix that is a prefix of another gets the smaller key. */
__global__ __launch_bounds__(256) void k_sa_key0(const uint8_t* __restrict__ text, size_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ pos) {
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if(i >= n) return;
	uint64_t k = 0;
#pragma unroll
	for(int s = 0; s < HU_SA_H0; ++s) k = (k << 3) | (i + s < n ? (uint64_t) text[i + s] + 1u : 0ull);
	key[i] = k; pos[i] = (uint32_t) i;
}
/* round r: the pair (rank of the first h symbols, rank of the next h symbols + 1, or 0 when the suffix ends before them) */
__global__ __launch_bounds__(256) void k_sa_key(const uint32_t* __restrict__ rank, size_t n, size_t h, uint64_t* __restrict__ key, uint32_t* __restrict__ pos) {
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if(i >= n) return;
	const uint32_t lo = i + h < n ? rank[i + h] + 1u : 0u;
	key[i] = ((uint64_t) rank[i] << 32) | lo; pos[i] = (uint32_t) i;
}
/* ranks from the sorted keys: a head flag wherever the key changes, an inclusive scan of the flags, rank = scan - 1 */
__device__ inline uint32_t sa_head(const uint64_t* key, size_t i, size_t n) { return i < n && (i == 0 || key[i] != key[i - 1]) ? 1u : 0u; }
__global__ __launch_bounds__(1024) void k_sa_head_sums(const uint64_t* __restrict__ key, size_t n, uint32_t* __restrict__ tileSum) {
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	uint32_t tot;
	(void) sa_block_scan(sa_head(key, i, n), wsum, tot);
	if(threadIdx.x == 0) tileSum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_sa_rank(const uint64_t* __restrict__ key, const uint32_t* __restrict__ pos, size_t n, const uint32_t* __restrict__ tileOff,
		uint32_t* __restrict__ rank) {
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	uint32_t tot;
	const uint32_t inc = sa_block_scan(sa_head(key, i, n), wsum, tot);
	if(i < n) { const uint32_t p = pos[i]; if(p < n) rank[p] = tileOff[blockIdx.x] + inc - 1u; }
}

/* ---- the BWT, the marks of the sampled rows (one bit per row, 64 rows per word, row i at bit i & 63) and the number of marks per 1,024 rows;
 * then the sampled values, compacted in row order behind the scanned tile counts */
__global__ __launch_bounds__(1024) void k_csfm_bwt(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa, size_t n, uint8_t* __restrict__ bwt,
		unsigned long long* __restrict__ marks, uint32_t* __restrict__ tileSum) {
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	uint32_t s = 0; bool mk = false;
	if(i < n) {
		s = sa[i];
		bwt[i] = (s == 0 || s >= n) ? (uint8_t) 0 : text[s - 1];
		mk = (s & 3u) == 0;
	}
	const unsigned long long b = __ballot(mk);
	if((threadIdx.x & 63) == 0 && i < n) marks[i >> 6] = b;
	uint32_t tot;
	(void) sa_block_scan(mk ? 1u : 0u, wsum, tot);
	if(threadIdx.x == 0) tileSum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_csfm_samples(const uint32_t* __restrict__ sa, size_t n, const uint32_t* __restrict__ tileOff, size_t cap, uint32_t* __restrict__ sampled) {
	__shared__ uint32_t wsum[16];
	const size_t i = (size_t) blockIdx.x * 1024 + threadIdx.x;
	const uint32_t s = i < n ? sa[i] : 1u;
	const bool mk = i < n && (s & 3u) == 0;
	uint32_t tot;
	const uint32_t inc = sa_block_scan(mk ? 1u : 0u, wsum, tot);
	const size_t at = (size_t) tileOff[blockIdx.x] + inc - 1u;
	if(mk && at < cap) sampled[at] = s;
}
