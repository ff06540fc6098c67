// The host half of hu_unifrac (hu_unifrac_host.cpp: the checks, the plan, the host path) with the table code of hu_otu_table.cpp
// under AddressSanitizer + UBSan, as a stand-alone program: random trees and tables of every degenerate shape.
//   unifrac_driver <trials>
// Checked on every result: finite, symmetric bit for bit, a zero diagonal, the normalised methods within [0, 1], identical columns
// at distance 0, and the same bits from two slab sizes that both hold every branch (L >= B).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_unifrac.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

struct Case { std::vector<int32_t> parent, node; std::vector<double> blen, counts; int64_t M, S; };

/* a random tree of n nodes (parent < child), or a chain */
static void make_tree(std::mt19937_64& g, int n, bool chain, Case& c) {
	c.parent.assign((size_t) n, -1); c.blen.assign((size_t) n, 0.0);
	for(int v = 1; v < n; ++v) { c.parent[(size_t) v] = chain ? v - 1 : (int32_t)(g() % (uint64_t) v); c.blen[(size_t) v] = 1e-5 + (double)(g() % 1000) / 997.0; }
}

static int run(const Case& c, int method, double alpha, int64_t slab, bool tree, int64_t wantB, std::vector<double>* keep) {
	hu_unifrac_opts o;
	hu_unifrac_default_opts(&o);
	o.method = method; o.alpha = alpha; o.slab = slab; o.host = 1;
	hu_unifrac_tree t; t.n_nodes = (int32_t) c.parent.size(); t.parent = c.parent.data(); t.blen = c.blen.data();
	HuUfPlan pl;
	if(hu_uf_plan("driver", tree ? &t : nullptr, c.M, c.S, tree ? c.node.data() : nullptr, c.counts.data(), &o, pl) != HU_OK) FAIL("plan refused M %lld S %lld", (long long) c.M, (long long) c.S);
	if(wantB >= 0 && pl.B != wantB) FAIL("B %lld, expected %lld", (long long) pl.B, (long long) wantB);
	const size_t S = (size_t) c.S;
	std::vector<double> P((size_t) pl.B * S), dist(S * S, -1.0), pd(S, -1.0);
	hu_uf_host_embed(pl, c.counts.data(), P.data());
	for(double p : P) if(!(p >= 0 && p <= 1)) FAIL("p %g outside [0, 1]", p);
	hu_uf_host_pairs(pl, P.data(), dist.data(), pd.data());
	for(size_t i = 0; i < S; ++i) {
		if(dist[i * S + i] != 0.0) FAIL("diagonal %g", dist[i * S + i]);
		if(!(pd[i] >= 0) || !std::isfinite(pd[i])) FAIL("pd %g", pd[i]);
		for(size_t j = 0; j < S; ++j) {
			const double d = dist[i * S + j];
			if(!std::isfinite(d) || d < 0 || memcmp(&d, &dist[j * S + i], 8) != 0) FAIL("d(%zu, %zu) = %g, d(j, i) = %g", i, j, d, dist[j * S + i]);
			if(method != HU_UF_WEIGHTED_RAW && d > 1 + 1e-12) FAIL("d(%zu, %zu) = %g above 1", i, j, d);
		}
	}
	if(keep) *keep = dist;
	return 0;
}

static void fill(std::mt19937_64& g, Case& c, int64_t M, int64_t S, bool twin) {
	c.M = M; c.S = S; c.counts.assign((size_t)(M * S), 0.0);
	for(int64_t j = 0; j < S; ++j) {
		for(int64_t i = 0; i < M; ++i) if(g() % 3 == 0) c.counts[(size_t)(i * S + j)] = (double)(g() % 50);
		c.counts[(size_t)((int64_t)(g() % (uint64_t) M) * S + j)] += 1.0;        /* no sample without reads */
	}
	if(twin && S >= 2) for(int64_t i = 0; i < M; ++i) c.counts[(size_t)(i * S + 1)] = 3.0 * c.counts[(size_t)(i * S)];
}

int main(int argc, char** argv) {
	const int trials = argc > 1 ? atoi(argv[1]) : 20;
	std::mt19937_64 g(20240611);
	static const int methods[] = {HU_UF_UNWEIGHTED, HU_UF_WEIGHTED, HU_UF_WEIGHTED_RAW, HU_UF_GENERALIZED};
	int done = 0;
	/* the shapes at which tiles, chunks and slabs end: chains that keep exactly B branches, S around one tile */
	static const int Bs[] = {1, 31, 32, 33}, Ss[] = {1, 2, 63, 64, 65};
	for(int B : Bs) for(int S : Ss) for(int m : methods) {
		Case c;
		make_tree(g, B + 5, true, c);
		const int64_t M = std::min(B, 4);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back(i == 0 ? B : (int32_t)(g() % (uint64_t)(B + 1)));   /* the deepest row fixes B */
		fill(g, c, M, S, true);
		std::vector<double> a, b;
		if(run(c, m, m == HU_UF_GENERALIZED ? 0.25 : 0.5, 0, true, B, &a)) return 1;
		if(run(c, m, m == HU_UF_GENERALIZED ? 0.25 : 0.5, 1000000, true, B, &b)) return 1;
		if(memcmp(a.data(), b.data(), a.size() * 8) != 0) FAIL("the default slab and one of 1000000, both above B, differ at B %d S %d method %d", B, S, m);
		if(S >= 2 && m != HU_UF_WEIGHTED_RAW && a[1] != 0.0) FAIL("a column and its triple at distance %g", a[1]);
		if(run(c, m, m == HU_UF_GENERALIZED ? 1.0 : 0.5, 7, true, B, nullptr)) return 1;
		++done;
	}
	/* one OTU; only the root; two rows on one node */
	for(int m : methods) {
		Case c;
		make_tree(g, 9, false, c);
		c.node = {5}; fill(g, c, 1, 3, false);
		if(run(c, m, 0.5, 0, true, -1, nullptr)) return 1;
		c.node = {0}; fill(g, c, 1, 2, false);
		std::vector<double> d;
		if(run(c, m, 0.5, 0, true, 0, &d)) return 1;
		if(d[1] != 0.0) FAIL("both samples on the root alone at distance %g", d[1]);
		c.node = {4, 4, 0}; fill(g, c, 3, 5, false);
		if(run(c, m, 0.5, 3, true, -1, nullptr)) return 1;
		++done;
	}
	for(int tr = 0; tr < trials; ++tr) {
		Case c;
		const int n = 1 + (int)(g() % 300);
		make_tree(g, n, g() % 4 == 0, c);
		const int64_t M = 1 + (int64_t)(g() % 40), S = 1 + (int64_t)(g() % 70);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back((int32_t)(g() % (uint64_t) n));
		fill(g, c, M, S, g() % 2 == 0);
		const int64_t slab = g() % 3 == 0 ? 0 : 1 + (int64_t)(g() % 70);
		for(int m : methods) if(run(c, m, m == HU_UF_GENERALIZED ? (double)(g() % 5) / 4.0 : 0.5, slab, true, -1, nullptr)) return 1;
		if(run(c, HU_UF_BRAY_CURTIS, 0.5, slab, false, M, nullptr) || run(c, HU_UF_JACCARD, 0.5, slab, false, M, nullptr)) return 1;
		++done;
	}
	/* the table code feeds the same path: a table made from arrays, its counts handed on */
	{
		const char* otus[] = {"3", "1"}; const char* taxa[] = {"a", ""}; const char* smp[] = {"s 1", "s2"};
		const double cnt[] = {1, 0, 0, 2};
		hu_otu_table* t = nullptr;
		if(hu_otu_table_new(2, 2, otus, taxa, smp, cnt, &t) != HU_OK) FAIL("hu_otu_table_new");
		Case c; c.M = 2; c.S = 2; c.counts.assign(hu_otu_table_counts(t), hu_otu_table_counts(t) + 4);
		hu_otu_table_free(t);
		std::vector<double> d;
		if(run(c, HU_UF_BRAY_CURTIS, 0.5, 0, false, 2, &d)) return 1;
		if(d[1] != 1.0) FAIL("disjoint samples at %g", d[1]);
	}
	/* what the plan refuses */
	{
		Case c; make_tree(g, 4, false, c); c.node = {9}; fill(g, c, 1, 1, false);
		hu_unifrac_opts o; hu_unifrac_default_opts(&o);
		hu_unifrac_tree t; t.n_nodes = 4; t.parent = c.parent.data(); t.blen = c.blen.data();
		HuUfPlan pl;
		if(hu_uf_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), &o, pl) != HU_ERR_ARG) FAIL("a node outside the tree was taken");
		c.node = {2}; c.parent = {1, 2, 1, 0}; t.parent = c.parent.data();
		if(hu_uf_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), &o, pl) != HU_ERR_ARG) FAIL("a tree without a root was taken");
		c.parent = {-1, 2, 1, 0}; t.parent = c.parent.data();
		if(hu_uf_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), &o, pl) != HU_ERR_ARG) FAIL("a cycle was taken");
		c.parent = {-1, 0, 1, 0}; t.parent = c.parent.data(); c.counts = {0.0};
		if(hu_uf_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), &o, pl) != HU_ERR_ARG) FAIL("a sample without reads was taken");
	}
	printf("%d cases\n", done);
	return 0;
}
