// hu_alpha without a device: the checks, the plan of a call, the host path, the metrics and the curve's mean and
// deviation.  No HIP headers: a plain C++ compiler builds this file (tests/san/alpha_driver.cpp).  The host path restates the
// definition of include/hmmufotu_amd.h in plain loops: a draw is the column hu_otu_subset gives, by the same selection; PD is added in the
// order of k_al_pd (hu_kern_alpha.h), A in ascending cell order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "hu_alpha.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_alpha_default_opts(hu_alpha_opts* o) {
	if(!o) return;
	o->host = 0; o->chunk = HU_OTU_CHUNK; o->key_bits = 64; o->reserved = 0; o->draw_chunk = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_alpha_need(int64_t n_sample, int64_t n_cell, int64_t n_entry, int64_t max_nnz, int64_t max_chunk, int64_t n_draw) {
	if(n_sample < 0 || n_cell < 0 || n_entry < 0 || max_nnz < 0 || max_chunk < 0 || n_draw < 0) return -1;
	return 32 * n_sample + 4 * (2 * n_cell + n_sample) + 16 * n_entry + n_draw * (1136 + 4 * max_nnz + 24 * max_chunk) + (1 << 20);
}

extern "C" void hu_alpha_metrics(hu_alpha_rec* r) {
	if(!r) return;
	const double N = (double) r->reads;
	const int64_t F1 = (int64_t) r->F1, F2 = (int64_t) r->F2;
	r->observed = (double) r->S; r->singles = (double) r->F1; r->doubles = (double) r->F2;
	r->chao1 = (double) r->S + (double) F1 * (double)(F1 - 1) / (2.0 * (double)(F2 + 1));
	r->shannon = r->S <= 1 ? 0.0 : std::max(0.0, std::log(N) - r->A / N);
	r->simpson = 1.0 - (double) r->Q / (N * N);
	r->goods_coverage = 1.0 - (double) r->F1 / N;
	r->faith_pd = r->PD;
}

extern "C" int hu_alpha_curve(int64_t n, const double* x, double* mean, double* sd) {
	if(n < 1 || !x || !mean || !sd) { hu_set_error("hu_alpha_curve: bad argument"); return HU_ERR_ARG; }
	double s = 0.0;
	for(int64_t i = 0; i < n; ++i) s += x[i];
	const double mu = s / (double) n;
	double q = 0.0;
	for(int64_t i = 0; i < n; ++i) { const double d = x[i] - mu; q += d * d; }
	*mean = mu;
	*sd = n > 1 ? std::sqrt(q / (double)(n - 1)) : std::numeric_limits<double>::quiet_NaN();
	return HU_OK;
}

int hu_al_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, uint64_t seed, const hu_alpha_opts* opts, HuAlPlan& pl) {
	hu_alpha_opts o;
	hu_alpha_default_opts(&o);
	if(opts) o = *opts;
	if(n_sample < 1) { hu_set_error("%s: a table without samples", fn); return HU_ERR_ARG; }
	if(n_otu < 0 || n_otu >= 0x7fffffffll || n_sample >= 0x7fffffffll || (n_otu > 0 && !counts) || n_depth < 0 || (n_depth > 0 && !depths)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(o.chunk < 1 || o.chunk > (1 << 24)) { hu_set_error("%s: chunk %d: 1 .. %d reads per workgroup", fn, o.chunk, 1 << 24); return HU_ERR_ARG; }
	if(o.key_bits < 1 || o.key_bits > 64) { hu_set_error("%s: key_bits %d: 1 .. 64", fn, o.key_bits); return HU_ERR_ARG; }
	if(o.draw_chunk < 0) { hu_set_error("%s: draw_chunk %lld below 0", fn, (long long) o.draw_chunk); return HU_ERR_ARG; }
	if(o.mem_budget < 0) { hu_set_error("%s: mem_budget %lld below 0", fn, (long long) o.mem_budget); return HU_ERR_ARG; }
	if(reps < 0) { hu_set_error("%s: reps %lld below 0", fn, (long long) reps); return HU_ERR_ARG; }
	if(reps == 0 && n_depth > 0) { hu_set_error("%s: %lld depths and no repeat: reps must be at least 1", fn, (long long) n_depth); return HU_ERR_ARG; }
	for(int64_t i = 0; i < n_depth; ++i) {
		if(depths[i] == 0) { hu_set_error("%s: depth %lld is 0: a draw keeps at least one read", fn, (long long) i); return HU_ERR_ARG; }
		if(i > 0 && depths[i] <= depths[i - 1]) { hu_set_error("%s: the depths must ascend strictly: %llu follows %llu", fn, (unsigned long long) depths[i], (unsigned long long) depths[i - 1]); return HU_ERR_ARG; }
	}
	if(n_depth > 0 && ((double) n_depth * (double) reps * (double) n_sample > 2147483648.0)) {
		hu_set_error("%s: %lld depths x %lld repeats x %lld samples: more than 2^31 draws", fn, (long long) n_depth, (long long) reps, (long long) n_sample); return HU_ERR_ARG; }
	std::vector<uint64_t> total;
	int rc = hu_otu_cells_check(fn, n_otu, n_sample, counts, total);
	if(rc != HU_OK) return rc;
	for(int64_t j = 0; j < n_sample; ++j) if(total[(size_t) j] == 0) {
		hu_set_error("%s: sample %lld has no reads: hmmufotu-amd-subset drops such samples", fn, (long long) j); return HU_ERR_ARG; }
	const size_t M = (size_t) n_otu, S = (size_t) n_sample;
	HuUfPlan up;
	if(tree) {
		hu_unifrac_opts uo;
		hu_unifrac_default_opts(&uo);
		uo.method = HU_UF_UNWEIGHTED; uo.host = 1;
		rc = hu_uf_plan(fn, tree, n_otu, n_sample, otu_node, counts, &uo, up);
		if(rc != HU_OK) return rc;
	}
	pl.M = n_otu; pl.S = n_sample; pl.hasTree = tree != nullptr; pl.B = tree ? up.B : 0; pl.nDepth = n_depth; pl.reps = reps;
	pl.host = o.host != 0; pl.chunk = o.chunk; pl.keyBits = o.key_bits; pl.drawChunk = o.draw_chunk; pl.budget = o.mem_budget; pl.seed = seed;
	pl.depth.assign(depths, depths + n_depth);
	pl.smp.assign(S, HuAlSample{0, 0, 0, 0, 0, 0});
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) if(counts[i * S + j] > 0) ++pl.smp[j].nnz;
	uint64_t nCell = 0;
	pl.maxNnz = 0; pl.maxChunk = 0;
	for(size_t j = 0; j < S; ++j) {
		HuAlSample& s = pl.smp[j];
		s.pfx0 = nCell + j; s.T = (uint32_t) total[j]; s.col = (uint32_t) j;
		nCell += s.nnz;
		pl.maxNnz = std::max<int64_t>(pl.maxNnz, s.nnz);
		pl.maxChunk = std::max<int64_t>(pl.maxChunk, (int64_t)((total[j] + (uint64_t) o.chunk - 1) / (uint64_t) o.chunk));
	}
	pl.prefix.assign((size_t) nCell + S, 0); pl.slot.assign((size_t) nCell, 0);
	std::vector<uint32_t> pos((size_t) nCell), fill(S, 0), run(S, 0), at(M * S);
	/* in depth-first order: where each nonzero cell lies among its sample's */
	for(size_t q = 0; q < M; ++q) {
		const size_t i = tree ? (size_t) up.perm[q] : q;
		for(size_t j = 0; j < S; ++j) if(counts[i * S + j] > 0) { pos[(size_t) pl.smp[j].pfx0 - j + fill[j]] = (uint32_t) q; at[i * S + j] = fill[j]++; }
	}
	/* in table order, which numbers the reads: the prefixes, and each cell's place in the depth-first order */
	std::fill(fill.begin(), fill.end(), 0u);
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) {
		const double v = counts[i * S + j];
		if(!(v > 0)) continue;
		pl.prefix[(size_t) pl.smp[j].pfx0 + fill[j]] = run[j]; pl.slot[(size_t) pl.smp[j].pfx0 - j + fill[j]] = at[i * S + j];
		++fill[j]; run[j] += (uint32_t) v;
	}
	for(size_t j = 0; j < S; ++j) pl.prefix[(size_t) pl.smp[j].pfx0 + pl.smp[j].nnz] = pl.smp[j].T;
	/* the branch entries of a sample: the kept branches whose interval of rows holds one of its nonzero cells, in branch order */
	pl.br.clear(); pl.brK.clear();
	for(size_t j = 0; j < S; ++j) {
		HuAlSample& s = pl.smp[j];
		s.br0 = pl.br.size();
		const uint32_t *p0 = pos.data() + ((size_t) s.pfx0 - j), *p1 = p0 + s.nnz;
		for(size_t k = 0; k < (size_t) pl.B; ++k) {
			const uint32_t lo = (uint32_t)(std::lower_bound(p0, p1, (uint32_t) up.lo[k]) - p0), hi = (uint32_t)(std::lower_bound(p0, p1, (uint32_t) up.hi[k]) - p0);
			if(hi > lo) { pl.br.push_back(HuAlBranch{up.b[k], lo, hi}); pl.brK.push_back((uint32_t) k); }
		}
		s.nBr = (uint32_t)(pl.br.size() - s.br0);
	}
	pl.unit.clear();
	for(size_t j = 0; j < S; ++j) pl.unit.push_back(HuAlUnit{(int32_t) j, -1, 0});
	for(size_t j = 0; j < S; ++j) for(int64_t r = 0; r < reps; ++r) for(int64_t d = 0; d < n_depth; ++d)
		if(pl.depth[(size_t) d] <= total[j]) pl.unit.push_back(HuAlUnit{(int32_t) j, (int32_t) d, (int32_t) r});
	return HU_OK;
}

/* S, F1, F2, Q, A and PD of one column: n [nnz] the nonzero cells of sample s in depth-first row order */
static HuAlStat al_stats(const HuAlPlan& pl, const HuAlSample& s, const uint32_t* n, std::vector<uint32_t>& W) {
	HuAlStat st; memset(&st, 0, sizeof(st));
	for(uint32_t c = 0; c < s.nnz; ++c) {
		const uint64_t v = n[c];
		st.S += v > 0; st.F1 += v == 1; st.F2 += v == 2; st.Q += v * v;
		if(v >= 2) st.A += (double) v * std::log((double) v);
	}
	st.PD = std::numeric_limits<double>::quiet_NaN();
	if(!pl.hasTree) return st;
	/* W[c]: the cells 0 .. c with a read; thread x of k_al_pd adds the entries x, x + 256, ...; then the tree over the 256 sums */
	W.resize(s.nnz);
	uint32_t w = 0;
	for(uint32_t c = 0; c < s.nnz; ++c) { w += n[c] > 0; W[c] = w; }
	double part[HU_AL_WG];
	for(int x = 0; x < HU_AL_WG; ++x) {
		double acc = 0.0;
		for(uint64_t e = (uint64_t) x; e < s.nBr; e += HU_AL_WG) {
			const HuAlBranch& b = pl.br[(size_t)(s.br0 + e)];
			acc += W[b.hi - 1] > (b.lo ? W[b.lo - 1] : 0u) ? b.b : 0.0;
		}
		part[x] = acc;
	}
	for(int wv = 0; wv < HU_AL_WAVES; ++wv) for(int d = 32; d >= 1; d >>= 1) for(int l = 0; l < d; ++l) part[wv * 64 + l] += part[wv * 64 + l + d];
	st.PD = (part[0] + part[64]) + (part[128] + part[192]);
	return st;
}

void hu_al_host(const HuAlPlan& pl, std::vector<HuAlStat>& stat) {
	stat.resize(pl.unit.size());
	std::vector<uint32_t> cells, W;
	std::vector<uint64_t> keys, work;
	for(size_t u = 0; u < pl.unit.size();) {
		const HuAlUnit& un = pl.unit[u];
		const HuAlSample& s = pl.smp[(size_t) un.smp];
		const uint32_t *P = pl.prefix.data() + s.pfx0, *L = pl.slot.data() + (s.pfx0 - s.col);
		cells.resize(s.nnz);
		if(un.depth < 0) {
			for(uint32_t c = 0; c < s.nnz; ++c) cells[L[c]] = P[c + 1] - P[c];
			stat[u++] = al_stats(pl, s, cells.data(), W);
			continue;
		}
		/* the draws of one (sample, repeat): the keys once, then every depth by hu_otu_subset_host's selection (hu_draw.h) */
		const uint64_t sd = pl.seed + (uint64_t) un.rep;
		const uint32_t key[2] = {(uint32_t)(sd & 0xffffffffu), (uint32_t)(sd >> 32)};
		keys.resize(s.T);
		for(uint64_t t = 0; t < s.T; ++t) keys[(size_t) t] = hu_otu_key(key, t, s.col, pl.keyBits);
		for(; u < pl.unit.size() && pl.unit[u].smp == un.smp && pl.unit[u].rep == un.rep && pl.unit[u].depth >= 0; ++u) {
			const uint64_t m = pl.depth[(size_t) pl.unit[u].depth];
			if(m >= s.T) { for(uint32_t c = 0; c < s.nnz; ++c) cells[L[c]] = P[c + 1] - P[c]; }
			else {
				work = keys;
				uint64_t cut, need;
				hu_draw_cut(work, m, cut, need);
				hu_draw_walk(cut, need, s.nnz, [&](uint64_t c) { return (uint64_t) P[c + 1]; }, [&](uint64_t t) { return keys[(size_t) t]; },
					[&](uint64_t c, uint64_t kept) { cells[L[c]] = (uint32_t) kept; });
			}
			stat[u] = al_stats(pl, s, cells.data(), W);
		}
	}
}

void hu_al_fill(const HuAlPlan& pl, const std::vector<HuAlStat>& stat, hu_alpha_rec* whole, hu_alpha_rec* draws) {
	const double nan = std::numeric_limits<double>::quiet_NaN();
	const size_t nDraw = (size_t) pl.S * (size_t) pl.nDepth * (size_t) pl.reps;
	if(draws) for(size_t i = 0; i < nDraw; ++i) {
		hu_alpha_rec& r = draws[i];
		r.reads = r.S = r.F1 = r.F2 = r.Q = 0;
		r.A = r.PD = r.observed = r.singles = r.doubles = r.chao1 = r.shannon = r.simpson = r.goods_coverage = r.faith_pd = nan;
	}
	for(size_t u = 0; u < pl.unit.size(); ++u) {
		const HuAlUnit& un = pl.unit[u];
		if(un.depth >= 0 && !draws) continue;
		hu_alpha_rec& r = un.depth < 0 ? whole[un.smp] : draws[((size_t) un.smp * (size_t) pl.nDepth + (size_t) un.depth) * (size_t) pl.reps + (size_t) un.rep];
		const HuAlStat& st = stat[u];
		r.reads = un.depth < 0 ? pl.smp[(size_t) un.smp].T : pl.depth[(size_t) un.depth];
		r.S = st.S; r.F1 = st.F1; r.F2 = st.F2; r.Q = st.Q; r.A = st.A; r.PD = pl.hasTree ? st.PD : nan;
		hu_alpha_metrics(&r);
	}
}

extern "C" int hu_alpha_sizes(const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, const hu_alpha_opts* opts, int64_t* out) try {
	const char* fn = "hu_alpha_sizes";
	if(!out) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuAlPlan pl;
	const int rc = hu_al_plan(fn, tree, n_otu, n_sample, otu_node, counts, n_depth, depths, reps, 0, opts, pl);
	if(rc != HU_OK) return rc;
	out[0] = (int64_t) pl.prefix.size() - pl.S; out[1] = (int64_t) pl.br.size(); out[2] = pl.maxNnz; out[3] = pl.maxChunk;
	out[4] = (int64_t) pl.unit.size(); out[5] = pl.B;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_alpha_sizes"); }
