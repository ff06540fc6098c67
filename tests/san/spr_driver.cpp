// The host half of the SPR search (hmmufotu_amd/csrc/hu_spr_host.cpp with hu_nni_host.cpp and hu_blen_host.cpp: the checks, the walks, the
// scores, apply with its refusals, the selection with its halving and the round loop) as a stand-alone program for AddressSanitizer +
// UBSan (tests/test_tree_spr.py builds and runs it).  Two small trees, one with a trifurcating top node and one with a bifurcating root
// and a node with four children; the pulley principle is held on every prunable node, the slab must not show in the scores, and a move
// and its inverse restore the arrays.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_spr.h"

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

/* leaf rows: a base row, and per group of leaves a set of columns where the group's leaves share another base */
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

static int g_searches = 0, g_refusals = 0;

/* one tree through the scores at three radii and slabs, apply with its inverse and a short search */
static void run(const std::vector<int32_t>& parent0, int32_t L, const std::vector<int8_t>& seq, size_t wantPruned, int64_t wantSkipped) {
	const int32_t n = (int32_t) parent0.size();
	const HuBlenModel m = jc69();
	hu_spr_opts o;
	hu_spr_default_opts(&o);
	o.blen.host = 1; o.blen.max_rounds = 30; o.spr_rounds = 3;
	std::vector<int32_t> parent = parent0, off, idx;
	std::vector<double> blen((size_t) n, 0.1);
	child_arrays(parent, &off, &idx);
	HuBlenTopo tp;
	REQUIRE(hu_blen_check("driver", &o.blen, n, L, parent.data(), blen.data(), seq.data(), 0, &tp) == HU_OK);
	std::vector<double> up((size_t) n * (size_t) L * 4);
	hu_blen_host_sweep(tp, m, parent.data(), L, blen.data(), seq.data(), up.data(), nullptr);
	const double ll = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4);
	HuSprScores far;
	for(int radius : {1, 2, HU_SPR_MAX_RADIUS}) {
		HuSprScores sc, one, cnt;
		o.radius = radius; o.slab = 0;
		REQUIRE(hu_spr_host_scores_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, false, &sc) == HU_OK);
		REQUIRE(sc.v.size() == wantPruned && sc.skipped == wantSkipped && sc.off.size() == wantPruned + 1 && (size_t) sc.off.back() == sc.w.size());
		REQUIRE(hu_spr_host_scores_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, true, &cnt) == HU_OK);
		REQUIRE(cnt.off == sc.off && cnt.v == sc.v);
		/* the pulley principle, and a slab of one node against the default */
		for(size_t i = 0; i < sc.v.size(); ++i) REQUIRE(std::fabs(sc.f0[i] - ll) <= 1e-12 * std::fabs(ll) && sc.baseF[i] >= sc.f0[i] - 1e-9);
		for(size_t k = 0; k < sc.w.size(); ++k) REQUIRE(sc.t[k] >= 0 && sc.t[k] <= 10 && sc.dist[k] >= 1 && sc.dist[k] <= radius && sc.w[k] != tp.root);
		o.slab = 1;
		REQUIRE(hu_spr_host_scores_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, false, &one) == HU_OK);
		REQUIRE(one.w == sc.w && one.dist == sc.dist && one.t == sc.t && one.f == sc.f && one.baseT == sc.baseT && one.baseF == sc.baseF && one.f0 == sc.f0);
		far = sc;
	}
	printf("slabs agree\n");
	/* a move gives the predicted log-likelihood; v back into the edge of s restores parent and the order of children */
	for(size_t i = 0; i < far.v.size(); ++i) for(int64_t k = far.off[i]; k < far.off[i + 1]; ++k) {
		const int32_t v = far.v[i], p = parent[v];
		const int32_t s = tp.childIdx[tp.childOff[p]] == v ? tp.childIdx[tp.childOff[p] + 1] : tp.childIdx[tp.childOff[p]];
		std::vector<int32_t> p2 = parent, i2 = idx; std::vector<double> b2 = blen;
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), off.data(), i2.data(), v, far.w[(size_t) k], far.t[(size_t) k]) == HU_OK);
		HuBlenTopo t2;
		REQUIRE(hu_blen_check("driver", &o.blen, n, L, p2.data(), b2.data(), seq.data(), 0, &t2) == HU_OK);
		hu_blen_host_sweep(t2, m, p2.data(), L, b2.data(), seq.data(), up.data(), nullptr);
		const double l2 = hu_blen_host_loglik(m, L, up.data() + (size_t) t2.root * L * 4);
		REQUIRE(std::fabs(l2 - far.f[(size_t) k]) <= 1e-12 * std::fabs(l2));
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), off.data(), i2.data(), v, s, 0.1) == HU_OK);
		REQUIRE(p2 == parent && i2 == idx);
	}
	/* the refusals of apply: the top node, a node that is not prunable, v itself, the edge where v hangs */
	if(!far.v.empty()) {
		const int32_t v = far.v[0], p = parent[v];
		const int32_t s = tp.childIdx[tp.childOff[p]] == v ? tp.childIdx[tp.childOff[p] + 1] : tp.childIdx[tp.childOff[p]];
		std::vector<int32_t> p2 = parent; std::vector<double> b2 = blen;
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), nullptr, nullptr, tp.root, s, 0.1) == HU_ERR_ARG);
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), nullptr, nullptr, v, tp.root, 0.1) == HU_ERR_ARG);
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), nullptr, nullptr, v, v, 0.1) == HU_ERR_ARG);
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), nullptr, nullptr, v, s, 0.1) == HU_ERR_ARG);
		REQUIRE(hu_tree_spr_apply(n, p2.data(), b2.data(), nullptr, nullptr, v, p, -1.0) == HU_ERR_ARG);
		REQUIRE(p2 == parent && b2 == blen);
		g_refusals = 5;
	}
	/* a short search */
	std::vector<hu_spr_round> rec(3); std::vector<int32_t> moves((size_t) 3 * (size_t) n * 5);
	o.radius = 3; o.slab = 2; o.rounds = rec.data(); o.rounds_cap = 3; o.moves = moves.data(); o.moves_cap = 3 * n;
	double sec[4] = {0, 0, 0, 0};
	REQUIRE(hu_spr_host_search_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), off.data(), idx.data(), m, sec) == HU_OK);
	REQUIRE(o.ll_final >= o.ll_start && o.stop >= 0 && o.stop <= 2 && o.n_rounds <= 3 && o.n_moves >= 1);
	for(int32_t r = 0; r < o.n_rounds; ++r) REQUIRE(rec[(size_t) r].ll > (r ? rec[(size_t) r - 1].ll : o.ll_start) && rec[(size_t) r].applied >= 1 && rec[(size_t) r].applied <= rec[(size_t) r].taken);
	for(int64_t k = 0; k < o.n_moves; ++k) REQUIRE(moves[(size_t) k * 5] >= 1 && moves[(size_t) k * 5 + 4] >= 1 && moves[(size_t) k * 5 + 4] <= 3);
	HuBlenTopo t3;
	REQUIRE(hu_blen_check("driver", &o.blen, n, L, parent.data(), blen.data(), seq.data(), 0, &t3) == HU_OK);
	for(int32_t v = 0; v < n; ++v) REQUIRE(t3.childOff[v + 1] - t3.childOff[v] == tp.childOff[v + 1] - tp.childOff[v]);
	std::vector<const char*> names((size_t) n, "x");
	REQUIRE(hu_newick_from_arrays(n, parent.data(), off.data(), idx.data(), names.data(), blen.data(), nullptr, 0) > 0);
	printf("search: %d round(s), %lld move(s), stop %d, ll %.6f -> %.6f\n", o.n_rounds, (long long) o.n_moves, o.stop, o.ll_start, o.ll_final);
	++g_searches;
}

int main() {
	/* a trifurcating top node: 0 = {1, 2, 7}, 2 = {3, 4}, 4 = {5, 6}, 7 = {8, 9}; the leaves 1, 3, 5, 6, 8, 9.  The rows put 3 with 8 and
	 * 5 with 9, so the start is no optimum.  The children of the top node are not pruned */
	const std::vector<int32_t> tri = {-1, 0, 0, 2, 2, 4, 4, 0, 7, 7};
	run(tri, 97, rows_for(tri, 97, 5u, {{3, 8}, {5, 9}}), 6, 3);
	/* a bifurcating root with two inner children, 0 = {1, 6}, 1 = {2, 5}, 2 = {3, 4}, 6 = {7, 8}, and a node with four children,
	 * 8 = {9, 10, 11, 12}: its children are not pruned, and the walks of the others pass through it */
	const std::vector<int32_t> bi = {-1, 0, 1, 2, 2, 1, 0, 6, 6, 8, 8, 8, 8};
	run(bi, 257, rows_for(bi, 257, 6u, {{3, 7}, {4, 5}}), 6, 6);
	/* the refusals of the checks, and the need */
	{
		hu_spr_opts o;
		hu_spr_default_opts(&o);
		REQUIRE(o.radius == 5 && o.spr_rounds == 10 && o.min_gain == 1e-3 && o.blen.max_rounds == 50);
		HuBlenTopo tp;
		std::vector<int8_t> seq(tri.size() * 3, (int8_t) 0);
		std::vector<double> b(tri.size(), 0.1);
		const int32_t n = (int32_t) tri.size();
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_OK);
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 4, &tp) == HU_ERR_ARG);
		o.radius = 0;
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.radius = HU_SPR_MAX_RADIUS + 1;
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.radius = 2; o.spr_rounds = 0;
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.spr_rounds = 1; o.min_gain = 0;
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.min_gain = 1e-3; o.blen.mem_budget = 100;
		REQUIRE(hu_spr_check("driver", &o, n, 3, tri.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_NOMEM);
		REQUIRE(hu_spr_need(10, 3, 2) == hu_blen_need(10, 3) + 9 * (32 + 96 * 10 + 2 * 32 * 3));
	}
	printf("refusals: %d\nsearches: %d\n", g_refusals, g_searches);
	return 0;
}
