// The host half of the NNI search (hmmufotu_amd/csrc/hu_nni_host.cpp with hu_blen_host.cpp: the checks, the eligible edges, the scores,
// apply, the selection with its halving, the round loop and the Newick writer from arrays) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_tree_nni.py builds and runs it).  Two small trees, one with a trifurcating top node and one with
// a bifurcating root and a node with four children; the pulley principle is held on every eligible edge, and a swap and its inverse
// restore the arrays.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_nni.h"

static char g_err[1024];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }

#define REQUIRE(c) do { if(!(c)) { fprintf(stderr, "line %d: %s failed (%s)\n", __LINE__, #c, g_err); exit(1); } } while(0)

/* JC69: lam = 0, -4/3 x 3; U the Hadamard matrix, U1 = U^T / 4, so U1's first row is pi */
static HuBlenModel jc69() {
	const double H[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
	double U1[16], lam[4] = {0, -4.0 / 3, -4.0 / 3, -4.0 / 3};
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) U1[k * 4 + i] = H[i * 4 + k] / 4;
	HuBlenModel m;
	hu_blen_model_set(&m, H, lam, U1);
	return m;
}

/* leaf rows: a base row, and per group of leaves a set of columns where the group's leaves share another base, so that the groups are
 * what a likelihood search puts together */
static std::vector<int8_t> rows_for(const std::vector<int32_t>& parent, int32_t L, unsigned seed, const std::vector<std::vector<int32_t>>& groups) {
	const size_t n = parent.size();
	std::vector<char> inner(n, 0);
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) inner[(size_t) parent[i]] = 1;
	std::mt19937 rng(seed);
	std::vector<int8_t> base((size_t) L), seq(n * (size_t) L, (int8_t) -2);
	for(auto& b : base) b = (int8_t)(rng() & 3);
	for(size_t i = 0; i < n; ++i) if(!inner[i]) for(int32_t j = 0; j < L; ++j) {
		const unsigned x = rng() % 100;
		seq[i * (size_t) L + (size_t) j] = x < 4 ? (int8_t)(rng() & 3) : x < 7 ? (int8_t) -2 : base[(size_t) j];
	}
	for(size_t g = 0; g < groups.size(); ++g) for(int32_t j = (int32_t) g; j < L; j += (int32_t) groups.size() + 1) {
		const int8_t b = (int8_t)((base[(size_t) j] + 1 + (int) (rng() % 3)) & 3);
		for(int32_t leaf : groups[g]) seq[(size_t) leaf * (size_t) L + (size_t) j] = b;
	}
	return seq;
}

static void child_arrays(const std::vector<int32_t>& parent, std::vector<int32_t>* off, std::vector<int32_t>* idx) {
	const size_t n = parent.size();
	off->assign(n + 1, 0); idx->assign(n - 1, 0);
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) (*off)[(size_t) parent[i] + 1]++;
	for(size_t i = 0; i < n; ++i) (*off)[i + 1] += (*off)[i];
	std::vector<int32_t> fill(off->begin(), off->end() - 1);
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) (*idx)[(size_t) fill[(size_t) parent[i]]++] = (int32_t) i;
}

static int g_searches = 0;

/* one tree through the scores, apply with its inverse, the writer and a short search */
static void run(const std::vector<int32_t>& parent0, int32_t L, const std::vector<int8_t>& seq, int wantEdges, int64_t wantSkipped) {
	const int32_t n = (int32_t) parent0.size();
	const HuBlenModel m = jc69();
	hu_nni_opts o;
	hu_nni_default_opts(&o);
	o.blen.host = 1; o.blen.max_rounds = 30; o.nni_rounds = 4;
	std::vector<int32_t> parent = parent0, off, idx;
	std::vector<double> blen((size_t) n, 0.1);
	child_arrays(parent, &off, &idx);
	const int32_t cap = n / 2;
	std::vector<int32_t> node((size_t) cap); std::vector<double> ts((size_t) cap * 3), f((size_t) cap * 3), f0((size_t) cap);
	int32_t E = -1; int64_t skipped = -1;
	REQUIRE(hu_nni_host_scores_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, cap, &E, &skipped, node.data(), ts.data(), f.data(), f0.data()) == HU_OK);
	REQUIRE(E == wantEdges && skipped == wantSkipped);
	/* the pulley principle: f^0 at the current length is the tree's log-likelihood on every edge */
	HuBlenTopo tp;
	REQUIRE(hu_blen_check("driver", &o.blen, n, L, parent.data(), blen.data(), seq.data(), 0, &tp) == HU_OK);
	std::vector<double> up((size_t) n * (size_t) L * 4);
	hu_blen_host_sweep(tp, m, parent.data(), L, blen.data(), seq.data(), up.data(), nullptr);
	const double ll = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4);
	for(int32_t e = 0; e < E; ++e) {
		REQUIRE(std::fabs(f0[(size_t) e] - ll) <= 1e-12 * std::fabs(ll));
		for(int q = 0; q < 3; ++q) REQUIRE(ts[(size_t) e * 3 + q] >= 0 && ts[(size_t) e * 3 + q] <= 10 && f[(size_t) e * 3] >= f0[(size_t) e] - 1e-9);
	}
	/* a swap gives the predicted log-likelihood; the swap of the same pair back restores parent and the order of children */
	std::vector<HuNniEdge> edges; int64_t sk2 = 0;
	hu_nni_edges(tp, parent.data(), blen.data(), &edges, &sk2);
	REQUIRE((int32_t) edges.size() == E && sk2 == skipped);
	for(int32_t e = 0; e < E; ++e) for(int q = 1; q <= 2; ++q) {
		std::vector<int32_t> p2 = parent, i2 = idx; std::vector<double> b2 = blen;
		REQUIRE(hu_tree_nni_apply(n, p2.data(), b2.data(), off.data(), i2.data(), node[(size_t) e], q, ts[(size_t) e * 3 + q]) == HU_OK);
		HuBlenTopo t2;
		REQUIRE(hu_blen_check("driver", &o.blen, n, L, p2.data(), b2.data(), seq.data(), 0, &t2) == HU_OK);
		hu_blen_host_sweep(t2, m, p2.data(), L, b2.data(), seq.data(), up.data(), nullptr);
		const double l2 = hu_blen_host_loglik(m, L, up.data() + (size_t) t2.root * L * 4);
		REQUIRE(std::fabs(l2 - f[(size_t) e * 3 + q]) <= 1e-12 * std::fabs(l2));
		std::vector<const char*> names((size_t) n, "x y");
		const int64_t len = hu_newick_from_arrays(n, p2.data(), off.data(), i2.data(), names.data(), b2.data(), nullptr, 0);
		REQUIRE(len > 0);
		std::string text((size_t) len + 1, '\0');
		REQUIRE(hu_newick_from_arrays(n, p2.data(), off.data(), i2.data(), names.data(), b2.data(), &text[0], len + 1) == len);
		REQUIRE(text[(size_t) len - 2] == ';' && text.find("'x y'") != std::string::npos);
		/* back: on an inner edge the moved subtree is the sibling now, so one of the two arrangements exchanges the same pair again; at the
		 * root the other side's smaller subtree may be another one */
		const HuNniEdge& ed = edges[(size_t) e];
		bool restored = false;
		for(int q2 = 1; q2 <= 2 && !restored; ++q2) {
			std::vector<int32_t> p3 = p2, i3 = i2; std::vector<double> b3 = b2;
			REQUIRE(hu_tree_nni_apply(n, p3.data(), b3.data(), off.data(), i3.data(), node[(size_t) e], q2, ed.t0) == HU_OK);
			restored = p3 == parent && i3 == idx;
		}
		REQUIRE(restored || ed.kind != HU_NNI_INNER);
	}
	REQUIRE(hu_tree_nni_apply(n, parent.data(), blen.data(), off.data(), idx.data(), tp.root, 1, 0.1) == HU_ERR_ARG);
	REQUIRE(hu_tree_nni_apply(n, parent.data(), blen.data(), off.data(), idx.data(), E ? node[0] : 1, 3, 0.1) == HU_ERR_ARG);
	/* a short search */
	std::vector<hu_nni_round> rec(4); std::vector<int32_t> swaps((size_t) 4 * (size_t) cap * 3);
	o.rounds = rec.data(); o.rounds_cap = 4; o.swaps = swaps.data(); o.swaps_cap = 4 * cap;
	double sec[4] = {0, 0, 0, 0};
	REQUIRE(hu_nni_host_search_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), off.data(), idx.data(), m, sec) == HU_OK);
	REQUIRE(o.ll_final >= o.ll_start && o.stop >= 0 && o.stop <= 2 && o.n_rounds <= 4 && o.skipped == wantSkipped);
	for(int32_t r = 0; r < o.n_rounds; ++r) REQUIRE(rec[(size_t) r].ll > (r ? rec[(size_t) r - 1].ll : o.ll_start) && rec[(size_t) r].applied >= 1 && rec[(size_t) r].applied <= rec[(size_t) r].taken);
	HuBlenTopo t3;
	REQUIRE(hu_blen_check("driver", &o.blen, n, L, parent.data(), blen.data(), seq.data(), 0, &t3) == HU_OK);
	for(int32_t v = 0; v < n; ++v) REQUIRE(t3.childOff[v + 1] - t3.childOff[v] == tp.childOff[v + 1] - tp.childOff[v]);
	printf("search: %d round(s), %lld swap(s), stop %d, ll %.6f -> %.6f\n", o.n_rounds, (long long) o.n_swaps, o.stop, o.ll_start, o.ll_final);
	++g_searches;
}

int main() {
	/* a trifurcating top node: 0 = {1, 2, 7}, 2 = {3, 4}, 4 = {5, 6}, 7 = {8, 9}; the leaves 1, 3, 5, 6, 8, 9.  The rows put 3 with 8 and
	 * 5 with 9, so the start is no optimum */
	const std::vector<int32_t> tri = {-1, 0, 0, 2, 2, 4, 4, 0, 7, 7};
	run(tri, 97, rows_for(tri, 97, 5u, {{3, 8}, {5, 9}}), 3, 0);
	/* a bifurcating root with two inner children, 0 = {1, 6}, 1 = {2, 5}, 2 = {3, 4}, 6 = {7, 8}, and a node with four children,
	 * 8 = {9, 10, 11, 12}: the edge above 8 is skipped */
	const std::vector<int32_t> bi = {-1, 0, 1, 2, 2, 1, 0, 6, 6, 8, 8, 8, 8};
	run(bi, 257, rows_for(bi, 257, 6u, {{3, 7}, {4, 5}}), 2, 1);
	/* the selection on a made-up gain list: five edges in a chain 1 - 2 - 3 - 4 - 5 and three apart from it */
	{
		std::vector<HuNniEdge> edges(8);
		const int32_t ends[8][2] = {{2, 1}, {3, 2}, {4, 3}, {5, 4}, {10, 9}, {12, 11}, {14, 13}, {16, 15}};
		for(int i = 0; i < 8; ++i) { memset(&edges[(size_t) i], 0, sizeof(HuNniEdge)); edges[(size_t) i].u = ends[i][0]; edges[(size_t) i].v = ends[i][1]; }
		const double gain[8] = {5.0, 7.0, 6.0, 0.5, 0.5, 1e-4, NAN, 3.0};
		std::vector<int32_t> order, taken;
		hu_nni_select(edges, gain, 1e-3, &order, &taken);
		/* by gain, ties by the smaller u; the edge below the bar and the one without a value are no candidates */
		REQUIRE((order == std::vector<int32_t>{1, 2, 0, 7, 3, 4}));
		/* 3-2 first; 4-3 and 2-1 share a node with it; 16-15, then 5-4 and 10-9 */
		REQUIRE((taken == std::vector<int32_t>{1, 7, 3, 4}));
		taken = {1, 7, 3, 4, 0};
		std::string trace = "halving: 5";
		while(hu_nni_halve(&taken)) { trace += " -> " + std::to_string(taken.size()); REQUIRE(taken[0] == 1); }
		REQUIRE(taken.size() == 1);
		printf("%s\n", trace.c_str());
	}
	/* the refusals */
	{
		hu_nni_opts o;
		hu_nni_default_opts(&o);
		REQUIRE(o.nni_rounds == 20 && o.min_gain == 1e-3 && o.blen.max_rounds == 50);
		HuBlenTopo tp;
		std::vector<int8_t> seq(tri.size() * 3, (int8_t) 0);
		std::vector<double> b(tri.size(), 0.1);
		REQUIRE(hu_nni_check("driver", &o, (int32_t) tri.size(), 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_OK);
		REQUIRE(hu_nni_check("driver", &o, (int32_t) tri.size(), 3, tri.data(), b.data(), seq.data(), 4, &tp) == HU_ERR_ARG);
		o.nni_rounds = 0;
		REQUIRE(hu_nni_check("driver", &o, (int32_t) tri.size(), 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.nni_rounds = 1; o.min_gain = 0;
		REQUIRE(hu_nni_check("driver", &o, (int32_t) tri.size(), 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.min_gain = 1e-3; o.blen.mem_budget = 100;
		REQUIRE(hu_nni_check("driver", &o, (int32_t) tri.size(), 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_NOMEM);
		REQUIRE(hu_nni_need(10, 3) == hu_blen_need(10, 3) + 160 * 4);
		REQUIRE(hu_nni_need(10, HU_NNI_LDS_COLS + 1) == hu_blen_need(10, HU_NNI_LDS_COLS + 1) + 160 * 4 + 72 * 4 * (int64_t)(HU_NNI_LDS_COLS + 1));
	}
	printf("searches: %d\n", g_searches);
	return 0;
}
