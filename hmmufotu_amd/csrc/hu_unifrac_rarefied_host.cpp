// hu_unifrac_rarefied without a device: the checks, the plan of a call, the host path and the recurrence of the mean.
// No HIP headers: a plain C++ compiler builds this file (tests/san/unifrac_rarefied_driver.cpp).  The host path restates the definition
// of include/hmmufotu_amd.h by the names it uses: a draw is hu_otu_subset's host selection on the original table, its distances are
// hu_unifrac's host path on the kept columns, and the mean is hu_ur_step in ascending draw order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "hu_unifrac_rarefied.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_unifrac_rarefied_default_opts(hu_unifrac_rarefied_opts* o) {
	if(!o) return;
	o->method = HU_UF_WEIGHTED; o->host = 0; o->alpha = 0.5; o->slab = 0; o->chunk = HU_OTU_CHUNK; o->key_bits = 64; o->draw_chunk = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_unifrac_rarefied_need(int64_t n_sample, int64_t n_kept, int64_t n_cell, int64_t n_entry, int64_t max_nnz, int64_t max_chunk,
		int64_t n_branch, int64_t slab, int64_t draw_chunk, int32_t want_draws) {
	if(n_sample < 0 || n_kept < 0 || n_cell < 0 || n_entry < 0 || max_nnz < 0 || max_chunk < 0 || n_branch < 0 || slab < 1 || draw_chunk < 0) return -1;
	const int64_t Sp = (n_kept + HU_UF_TILE - 1) / HU_UF_TILE * HU_UF_TILE, tiles = hu_uf_tiles(n_kept), slabs = (n_branch + slab - 1) / slab;
	const int64_t table = 32 * n_sample + 4 * (2 * n_cell + n_sample) + 20 * n_entry + 8 * n_branch;
	const int64_t perDraw = n_kept * (1096 + 4 * max_nnz + 24 * max_chunk) + 8 * n_branch * Sp + 65536 * slabs * tiles;
	return table + draw_chunk * perDraw + (want_draws ? draw_chunk : 0) * 8 * n_kept * n_kept + 16 * n_kept * n_kept + (1 << 20);
}

int hu_ur_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, uint64_t seed, const hu_unifrac_rarefied_opts* opts, HuUrPlan& pl) {
	hu_unifrac_rarefied_opts o;
	hu_unifrac_rarefied_default_opts(&o);
	if(opts) o = *opts;
	if(depth == 0) { hu_set_error("%s: the depth is 0: a draw keeps at least one read", fn); return HU_ERR_ARG; }
	if(reps < 1 || reps > HU_UFR_MAX_REPS) { hu_set_error("%s: %lld repeats: 1 .. %d", fn, (long long) reps, HU_UFR_MAX_REPS); return HU_ERR_ARG; }
	hu_unifrac_opts uo;
	hu_unifrac_default_opts(&uo);
	uo.method = o.method; uo.alpha = o.alpha; uo.slab = o.slab; uo.host = 1;
	int rc = hu_uf_plan(fn, tree, n_otu, n_sample, otu_node, counts, &uo, pl.uf);
	if(rc != HU_OK) return rc;
	hu_alpha_opts ao;
	hu_alpha_default_opts(&ao);
	ao.host = o.host; ao.chunk = o.chunk; ao.key_bits = o.key_bits; ao.draw_chunk = o.draw_chunk; ao.mem_budget = o.mem_budget;
	rc = hu_al_plan(fn, tree, n_otu, n_sample, otu_node, counts, 0, nullptr, 0, seed, &ao, pl.al);
	if(rc != HU_OK) return rc;
	const size_t M = (size_t) n_otu, S = (size_t) n_sample;
	pl.nSample = n_sample; pl.reps = reps; pl.depth = depth; pl.seed = seed; pl.host = o.host != 0; pl.drawChunk = o.draw_chunk; pl.budget = o.mem_budget;
	pl.total.resize(S); pl.keptCol.clear();
	for(size_t j = 0; j < S; ++j) { pl.total[j] = pl.al.smp[j].T; if(pl.total[j] >= depth) pl.keptCol.push_back((int32_t) j); }
	pl.Sk = (int64_t) pl.keptCol.size();
	std::vector<uint64_t> desc(pl.total);
	std::sort(desc.begin(), desc.end(), [](uint64_t a, uint64_t b) { return a > b; });
	pl.maxDepth2 = S >= 2 ? desc[1] : 0;
	if(pl.Sk < 2) {
		if(S < 2) hu_set_error("%s: the table has %zu sample: distances need 2", fn, S);
		else hu_set_error("%s: %lld sample(s) have %llu reads or more: distances need 2; the largest depth that keeps 2 samples is %llu", fn, (long long) pl.Sk,
			(unsigned long long) depth, (unsigned long long) pl.maxDepth2);
		return HU_ERR_ARG;
	}
	if(!tree) {
		/* the identity tree: every row is its own branch of length 1, so a sample's entries are its nonzero cells in table order, where
		 * hu_al_plan keeps the cells of a table without a tree */
		pl.al.br.clear(); pl.al.brK.clear();
		for(size_t j = 0; j < S; ++j) {
			HuAlSample& s = pl.al.smp[j];
			s.br0 = pl.al.br.size();
			uint32_t c = 0;
			for(size_t i = 0; i < M; ++i) if(counts[i * S + j] > 0) { pl.al.br.push_back(HuAlBranch{1.0, c, c + 1}); pl.al.brK.push_back((uint32_t) i); ++c; }
			s.nBr = c;
		}
	}
	pl.uf.S = pl.Sk;
	pl.uf.L = o.slab > 0 ? o.slab : hu_unifrac_default_slab(pl.Sk, pl.uf.B);
	pl.uf.nSlab = pl.uf.B > 0 ? (pl.uf.B + pl.uf.L - 1) / pl.uf.L : 0;
	if(pl.uf.nSlab > 65535) { hu_set_error("%s: %lld slabs of %lld branches: more than a grid holds, raise the slab", fn, (long long) pl.uf.nSlab, (long long) pl.uf.L); return HU_ERR_ARG; }
	return HU_OK;
}

void hu_ur_host(const HuUrPlan& pl, const double* counts, double* mean, double* m2, double* draws) {
	const size_t M = (size_t) pl.uf.M, S = (size_t) pl.nSample, Sk = (size_t) pl.Sk, B = (size_t) pl.uf.B;
	std::vector<double> sub(M * S), X(M * Sk), P(B * Sk), D(Sk * Sk);
	std::fill(mean, mean + Sk * Sk, 0.0); std::fill(m2, m2 + Sk * Sk, 0.0);
	for(int64_t r = 0; r < pl.reps; ++r) {
		hu_otu_subset_host((int64_t) M, (int64_t) S, counts, pl.total, pl.depth, HU_OTU_UNIFORM, pl.seed + (uint64_t) r, pl.al.keyBits, sub.data());
		for(size_t i = 0; i < M; ++i) for(size_t a = 0; a < Sk; ++a) X[i * Sk + a] = sub[i * S + (size_t) pl.keptCol[a]];
		hu_uf_host_embed(pl.uf, X.data(), P.data());
		hu_uf_host_pairs(pl.uf, P.data(), D.data(), nullptr);
		if(draws) std::copy(D.begin(), D.end(), draws + (size_t) r * Sk * Sk);
		for(size_t e = 0; e < Sk * Sk; ++e) hu_ur_step(D[e], (double)(r + 1), mean[e], m2[e]);
	}
}

void hu_ur_sd(int64_t n, int64_t reps, const double* m2, double* sd) {
	const double nan = std::numeric_limits<double>::quiet_NaN();
	for(int64_t e = 0; e < n; ++e) sd[e] = reps > 1 ? std::sqrt(m2[e] / (double)(reps - 1)) : nan;
}

extern "C" int hu_unifrac_rarefied_sizes(const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, const hu_unifrac_rarefied_opts* opts, int64_t* out) try {
	const char* fn = "hu_unifrac_rarefied_sizes";
	if(!out) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuUrPlan pl;
	const int rc = hu_ur_plan(fn, tree, n_otu, n_sample, otu_node, counts, depth, reps, 0, opts, pl);
	if(rc != HU_OK) return rc;
	out[0] = pl.Sk; out[1] = (int64_t) pl.al.prefix.size() - pl.al.S; out[2] = (int64_t) pl.al.br.size(); out[3] = pl.al.maxNnz; out[4] = pl.al.maxChunk;
	out[5] = pl.uf.B; out[6] = pl.uf.L; out[7] = (int64_t) pl.maxDepth2;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_unifrac_rarefied_sizes"); }
