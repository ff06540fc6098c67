// The host half of hu_unifrac_rarefied (hu_unifrac_rarefied_host.cpp: the checks, the plan, the host path, the recurrence) with
// hu_alpha_host.cpp, hu_unifrac_host.cpp and hu_otu_table.cpp (the subset's host selection) under AddressSanitizer + UBSan, as a
// stand-alone program: random trees and tables of degenerate shapes.
//   unifrac_rarefied_driver <trials>
// Checked on every result: the lists the device kernels index with (a branch entry's cells inside the sample's, its branch below B, the
// entries of a sample in ascending branch number); every draw symmetric with a zero diagonal and inside its method's range; the mean
// between the smallest and the largest draw; sd >= 0, NaN for one repeat; with the depth at every sample's total, each draw equal to
// the host path of hu_unifrac on the table bit for bit and sd exactly 0.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_unifrac_rarefied.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

struct Case { std::vector<int32_t> parent, node; std::vector<double> blen, counts; int64_t M, S; };

static void make_tree(std::mt19937_64& g, int n, bool chain, Case& c) {
	c.parent.assign((size_t) n, -1); c.blen.assign((size_t) n, 0.0);
	for(int v = 1; v < n; ++v) { c.parent[(size_t) v] = chain ? v - 1 : (int32_t)(g() % (uint64_t) v); c.blen[(size_t) v] = 1e-5 + (double)(g() % 1000) / 997.0; }
}

static void fill(std::mt19937_64& g, Case& c, int64_t M, int64_t S, int top) {
	c.M = M; c.S = S; c.counts.assign((size_t)(M * S), 0.0);
	for(int64_t j = 0; j < S; ++j) {
		for(int64_t i = 0; i < M; ++i) if(g() % 3 == 0) c.counts[(size_t)(i * S + j)] = (double)(g() % (uint64_t) top);
		c.counts[(size_t)((int64_t)(g() % (uint64_t) M) * S + j)] += 1.0;        /* no sample without reads */
	}
}

static int run(const Case& c, int method, double alpha, int keyBits, uint64_t seed, int64_t reps, uint64_t depth, int64_t slab) {
	const bool tree = method < HU_UF_BRAY_CURTIS;
	hu_unifrac_rarefied_opts o;
	hu_unifrac_rarefied_default_opts(&o);
	o.method = method; o.alpha = alpha; o.host = 1; o.key_bits = keyBits; o.chunk = 64; o.slab = slab;
	hu_unifrac_tree t; t.n_nodes = (int32_t) c.parent.size(); t.parent = c.parent.data(); t.blen = c.blen.data();
	HuUrPlan pl;
	const int rc = hu_ur_plan("driver", tree ? &t : nullptr, c.M, c.S, tree ? c.node.data() : nullptr, c.counts.data(), depth, reps, seed, &o, pl);
	int64_t keep = 0;
	std::vector<uint64_t> tot((size_t) c.S, 0);
	for(int64_t i = 0; i < c.M; ++i) for(int64_t j = 0; j < c.S; ++j) tot[(size_t) j] += (uint64_t) c.counts[(size_t)(i * c.S + j)];
	for(uint64_t x : tot) keep += x >= depth;
	if(keep < 2) { if(rc != HU_ERR_ARG) FAIL("%lld kept samples were taken", (long long) keep); return 0; }
	if(rc != HU_OK) FAIL("plan refused M %lld S %lld depth %llu", (long long) c.M, (long long) c.S, (unsigned long long) depth);
	if(pl.Sk != keep || pl.al.br.size() != pl.al.brK.size()) FAIL("kept %lld of %lld", (long long) pl.Sk, (long long) keep);
	for(const HuAlSample& s : pl.al.smp) for(uint32_t e = 0; e < s.nBr; ++e) {
		const HuAlBranch& b = pl.al.br[(size_t) s.br0 + e];
		const uint32_t k = pl.al.brK[(size_t) s.br0 + e];
		if(!(b.lo < b.hi && b.hi <= s.nnz) || (int64_t) k >= pl.uf.B || (e > 0 && k <= pl.al.brK[(size_t) s.br0 + e - 1]) || b.b != pl.uf.b[k])
			FAIL("sample %u entry %u: cells [%u, %u) of %u, branch %u of %lld", s.col, e, b.lo, b.hi, s.nnz, k, (long long) pl.uf.B);
	}
	if(hu_unifrac_rarefied_need(c.S, pl.Sk, (int64_t) pl.al.prefix.size() - c.S, (int64_t) pl.al.br.size(), pl.al.maxNnz, pl.al.maxChunk, pl.uf.B, pl.uf.L, 1, 1) < (1 << 20))
		FAIL("need");
	const size_t K = (size_t) pl.Sk, R = (size_t) reps;
	std::vector<double> mean(K * K), m2(K * K), sd(K * K), draws(R * K * K);
	hu_ur_host(pl, c.counts.data(), mean.data(), m2.data(), draws.data());
	hu_ur_sd((int64_t)(K * K), reps, m2.data(), sd.data());
	const bool norm = method != HU_UF_WEIGHTED_RAW;
	for(size_t i = 0; i < K; ++i) for(size_t j = 0; j < K; ++j) {
		double lo = INFINITY, hi = -INFINITY;
		for(size_t r = 0; r < R; ++r) {
			const double d = draws[(r * K + i) * K + j];
			if(memcmp(&d, &draws[(r * K + j) * K + i], 8) != 0 || (i == j && d != 0.0) || !(d >= 0) || (norm && !(d <= 1.0 + 1e-12))) FAIL("draw %zu pair (%zu, %zu): %g", r, i, j, d);
			lo = std::min(lo, d); hi = std::max(hi, d);
		}
		const double mu = mean[i * K + j], s = sd[i * K + j];
		if(memcmp(&mu, &mean[j * K + i], 8) != 0 || memcmp(&s, &sd[j * K + i], 8) != 0) FAIL("pair (%zu, %zu) is not its mirrored copy", i, j);
		if(!(mu >= lo - 1e-12 && mu <= hi + 1e-12) || (i == j && mu != 0.0)) FAIL("pair (%zu, %zu): mean %g outside [%g, %g]", i, j, mu, lo, hi);
		if(R == 1 ? s == s : !(s >= 0 && (i != j || s == 0.0))) FAIL("pair (%zu, %zu): sd %g over %zu draws", i, j, s, R);
	}
	bool whole = true;
	for(uint64_t x : tot) whole = whole && x == depth;
	if(whole) {
		hu_unifrac_opts uo; hu_unifrac_default_opts(&uo);
		uo.method = method; uo.alpha = alpha; uo.host = 1; uo.slab = slab;
		HuUfPlan up;
		if(hu_uf_plan("driver", tree ? &t : nullptr, c.M, c.S, tree ? c.node.data() : nullptr, c.counts.data(), &uo, up) != HU_OK) FAIL("hu_uf_plan");
		std::vector<double> P((size_t) up.B * (size_t) up.S), D(K * K);
		hu_uf_host_embed(up, c.counts.data(), P.data()); hu_uf_host_pairs(up, P.data(), D.data(), nullptr);
		for(size_t r = 0; r < R; ++r) if(memcmp(D.data(), draws.data() + r * K * K, K * K * 8) != 0) FAIL("draw %zu at every sample's total is not hu_unifrac of the table", r);
		if(memcmp(D.data(), mean.data(), K * K * 8) != 0) FAIL("the mean of equal draws is not the draw");
		if(R > 1) for(double s : sd) if(s != 0.0) FAIL("sd %g of equal draws", s);
	}
	return 0;
}

int main(int argc, char** argv) {
	const int trials = argc > 1 ? atoi(argv[1]) : 20;
	std::mt19937_64 g(20241021);
	int done = 0;
	static const int methods[] = {HU_UF_UNWEIGHTED, HU_UF_WEIGHTED, HU_UF_WEIGHTED_RAW, HU_UF_GENERALIZED, HU_UF_BRAY_CURTIS, HU_UF_JACCARD};
	auto depths = [](const Case& c) {
		std::vector<uint64_t> tot((size_t) c.S, 0);
		for(int64_t i = 0; i < c.M; ++i) for(int64_t j = 0; j < c.S; ++j) tot[(size_t) j] += (uint64_t) c.counts[(size_t)(i * c.S + j)];
		std::sort(tot.begin(), tot.end());
		return std::vector<uint64_t>{1, tot[0], tot[0] + 1, tot.back(), tot.back() + 1};
	};
	/* chains that keep exactly B branches, slabs of 32 and the default; keys that tie */
	for(int B : {1, 31, 32, 33, 65}) for(int S : {2, 3, 5}) for(int kb : {64, 4}) {
		Case c;
		make_tree(g, B + 5, true, c);
		const int64_t M = std::min(B, 6);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back(i == 0 ? B : (int32_t)(g() % (uint64_t)(B + 1)));
		fill(g, c, M, S, 50);
		for(uint64_t m : depths(c)) if(run(c, methods[done % 4], 0.5, kb, 7 + (uint64_t) done, 1 + done % 3, m, done % 2 ? 32 : 0)) return 1;
		++done;
	}
	/* one OTU; only the root; two rows on one node with the root and an empty row; a seed whose repeats wrap at 2^64; equal totals */
	{
		Case c;
		make_tree(g, 9, false, c);
		c.node = {5}; fill(g, c, 1, 3, 50);
		for(uint64_t m : depths(c)) if(run(c, HU_UF_WEIGHTED, 0.5, 64, 1, 2, m, 0)) return 1;
		c.node = {0}; fill(g, c, 1, 2, 50);
		for(uint64_t m : depths(c)) if(run(c, HU_UF_UNWEIGHTED, 0.5, 64, 1, 2, m, 0)) return 1;
		c.node = {4, 4, 0, 7}; fill(g, c, 4, 5, 50);
		for(int64_t j = 0; j < 5; ++j) c.counts[(size_t)(3 * 5 + j)] = 0.0;
		for(int64_t j = 0; j < 5; ++j) c.counts[(size_t) j] += 1.0;
		for(int m : methods) for(uint64_t d : depths(c)) if(run(c, m, m == HU_UF_GENERALIZED ? 0.3 : 0.5, 8, ~0ull - 1, 3, d, 0)) return 1;
		for(int64_t j = 0; j < 5; ++j) { c.counts[(size_t) j] = 9.0 - (double) j; c.counts[(size_t)(5 + j)] = 8.0; c.counts[(size_t)(10 + j)] = (double) j; c.counts[(size_t)(15 + j)] = 0.0; }   /* 17 reads each */
		for(int m : methods) if(run(c, m, 0.5, 64, 3, 3, 17, 0) || run(c, m, 0.5, 64, 3, 1, 17, 2)) return 1;
		done += 4;
	}
	for(int tr = 0; tr < trials; ++tr) {
		Case c;
		const int n = 1 + (int)(g() % 200);
		make_tree(g, n, g() % 4 == 0, c);
		const int64_t M = 1 + (int64_t)(g() % 120), S = 1 + (int64_t)(g() % 8);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back((int32_t)(g() % (uint64_t) n));
		fill(g, c, M, S, g() % 2 ? 4 : 40);
		const std::vector<uint64_t> d = depths(c);
		const int m = methods[g() % 6];
		if(run(c, m, m == HU_UF_GENERALIZED ? (double)(g() % 5) / 4.0 : 0.5, g() % 3 == 0 ? 6 : 64, g(), 1 + (int64_t)(g() % 3), d[g() % d.size()], g() % 3 == 0 ? 1 + (int64_t)(g() % 40) : 0)) return 1;
		++done;
	}
	/* what the plan refuses */
	{
		Case c; make_tree(g, 4, false, c); c.node = {2, 3}; fill(g, c, 2, 3, 50);
		hu_unifrac_tree t; t.n_nodes = 4; t.parent = c.parent.data(); t.blen = c.blen.data();
		HuUrPlan pl;
		hu_unifrac_rarefied_opts o; hu_unifrac_rarefied_default_opts(&o); o.host = 1;
		if(hu_ur_plan("driver", &t, 2, 3, c.node.data(), c.counts.data(), 0, 1, 1, &o, pl) != HU_ERR_ARG) FAIL("a depth of 0 was taken");
		if(hu_ur_plan("driver", &t, 2, 3, c.node.data(), c.counts.data(), 1, 0, 1, &o, pl) != HU_ERR_ARG) FAIL("no repeat was taken");
		if(hu_ur_plan("driver", &t, 2, 3, c.node.data(), c.counts.data(), 1, HU_UFR_MAX_REPS + 1, 1, &o, pl) != HU_ERR_ARG) FAIL("too many repeats were taken");
		if(hu_ur_plan("driver", &t, 2, 1, c.node.data(), c.counts.data(), 1, 1, 1, &o, pl) != HU_ERR_ARG) FAIL("one sample was taken");
		o.method = HU_UF_JACCARD;
		if(hu_ur_plan("driver", &t, 2, 3, c.node.data(), c.counts.data(), 1, 1, 1, &o, pl) != HU_ERR_ARG) FAIL("jaccard with a tree was taken");
		o.method = HU_UF_WEIGHTED; c.counts[0] = 1.5;
		if(hu_ur_plan("driver", &t, 2, 3, c.node.data(), c.counts.data(), 1, 1, 1, &o, pl) != HU_ERR_ARG) FAIL("a fraction was taken");
	}
	printf("%d cases\n", done);
	return 0;
}
