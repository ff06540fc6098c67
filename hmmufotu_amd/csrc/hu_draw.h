// The uniform draw without replacement that hu_otu_subset, hu_alpha and hu_unifrac_rarefied share: the records that the
// host builds and the kernels of hu_kern_draw.h read, the helper that appends to the lists, and the host's selection.  No HIP headers: a
// plain C++ compiler reads this file (hu_otu_table.cpp, hu_alpha_host.cpp).
//
// Read t of sample j has a 64-bit key, a function of (seed, t, j) alone (hu_otu_key, hu_otu_table.h); a draw of m reads keeps the m
// smallest in (key, t) order.  The records carry hu_alpha's names, which came first.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#define HU_DRAW_WG 256           /* threads of a workgroup of the draw kernels */
#define HU_DRAW_WAVES 4          /* its waves: a chunk's reads are four spans, and a draw has four tie counts per chunk */

/* a sample: its nnz + 1 prefixes (P[c] = reads before nonzero cell c in table order, P[nnz] = T), its nnz slots from pfx0 - col on (the
 * place of cell c in depth-first row order, in which a draw's cells are kept) and its branch entries; a caller without a slot map
 * (hu_otu_subset) keeps a draw's cells in table order and leaves br0 and nBr 0 */
struct HuAlSample { uint64_t pfx0, br0; uint32_t nnz, T, col, nBr; };
/* a resident draw: its nnz cells in out[], its tie counts (4 per chunk of its sample), its sample, its depth (0: the whole sample) */
struct HuAlDraw { uint64_t cell0, tie0; uint32_t smp, m; };
/* the draws draw0 .. draw0 + nd - 1 of one (sample, key) in ascending depth; (k0, k1) is the Philox key */
struct HuAlGroup { uint64_t chunk0; uint32_t smp, k0, k1, draw0, nd, nChunk; };
struct HuAlChunk { uint32_t g, t0; };                         /* group, first read (k_otu_multinom: first draw) */
struct HuAlSel { uint64_t prefix; uint32_t rank, eq; };       /* digits found so far; reads still wanted among the `eq` that carry them */

/* appends a group of nd draws from draw0 on under the key of `seed`, and its chunks: `work` reads (or draws), perChunk to a workgroup */
inline void hu_draw_add_group(std::vector<HuAlGroup>& grp, std::vector<HuAlChunk>& chunk, uint32_t smp, uint64_t seed, uint32_t draw0, uint32_t nd,
		uint64_t work, uint64_t perChunk) {
	const uint32_t nChunk = (uint32_t)((work + perChunk - 1) / perChunk);
	grp.push_back(HuAlGroup{chunk.size(), smp, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw0, nd, nChunk});
	for(uint32_t c = 0; c < nChunk; ++c) chunk.push_back(HuAlChunk{(uint32_t)(grp.size() - 1), (uint32_t)(c * perChunk)});
}

/* the host's selection of m out of the reads whose keys are keys[] (1 <= m <= keys.size(); the order of keys[] is lost): the key that
 * has rank m, and how many of the reads that carry it are kept, the first `need` in read order */
inline void hu_draw_cut(std::vector<uint64_t>& keys, uint64_t m, uint64_t& cut, uint64_t& need) {
	std::nth_element(keys.begin(), keys.begin() + (size_t)(m - 1), keys.end());
	cut = keys[(size_t)(m - 1)];
	need = m;
	for(uint64_t r = 0; r + 1 < m; ++r) need -= keys[(size_t) r] < cut;
}
/* the walk in read order: cell c holds the reads up to end(c), key(t) is read t's key, and put(c, kept) receives the cell's kept reads */
template<class End, class Key, class Put> inline void hu_draw_walk(uint64_t cut, uint64_t need, uint64_t nCell, End end, Key key, Put put) {
	uint64_t t = 0;
	for(uint64_t c = 0; c < nCell; ++c) {
		uint64_t kept = 0;
		for(const uint64_t e = end(c); t < e; ++t) {
			const uint64_t k = key(t);
			if(k < cut) ++kept;
			else if(k == cut && need > 0) { ++kept; --need; }
		}
		put(c, kept);
	}
}
