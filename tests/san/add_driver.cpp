// The host half of the insertion of new sequences (hmmufotu_amd/csrc/hu_add_host.cpp with hu_blen_host.cpp: the checks, the scores, the
// best edges, apply with its refusals and the round loop) as a stand-alone program for AddressSanitizer + UBSan (tests/test_tree_add.py
// builds and runs it).  Three leaves plus one query at one column, a tree with a bifurcating root and a node with four children at 257
// columns with a query of gaps only, five leaves at one column, and two queries that want one edge: the predicted f is held to the
// log-likelihood of the grown arrays, and a search must leave a tree with every query as a leaf.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_add.h"

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

static void child_arrays(const std::vector<int32_t>& parent, size_t n, std::vector<int32_t>* off, std::vector<int32_t>* idx) {
	for(size_t i = 0; i <= n; ++i) (*off)[i] = 0;
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) (*off)[(size_t) parent[i] + 1]++;
	for(size_t i = 0; i < n; ++i) (*off)[i + 1] += (*off)[i];
	std::vector<int32_t> fill(off->begin(), off->begin() + (long) n);
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) (*idx)[(size_t) fill[(size_t) parent[i]]++] = (int32_t) i;
}

static int g_searches = 0, g_refusals = 0;

/* the leaves' rows: independent random bases with a few gaps; the queries: the row of leaf near[k] with one column in twenty changed, or
 * gaps only where near[k] < 0 */
static int run(const std::vector<int32_t>& parent0, int32_t L, const std::vector<int32_t>& near, unsigned seed) {
	const int32_t n = (int32_t) parent0.size(), q = (int32_t) near.size();
	const size_t N = (size_t) n + 2 * (size_t) q, sL = (size_t) L;
	const HuBlenModel m = jc69();
	std::mt19937 rng(seed);
	std::vector<char> inner((size_t) n, 0);
	for(int32_t i = 0; i < n; ++i) if(parent0[(size_t) i] >= 0) inner[(size_t) parent0[(size_t) i]] = 1;
	std::vector<int8_t> seq(N * sL, (int8_t) -2), qs((size_t) q * sL, (int8_t) -2);
	for(int32_t i = 0; i < n; ++i) if(!inner[(size_t) i]) for(size_t j = 0; j < sL; ++j) seq[(size_t) i * sL + j] = rng() % 20 == 0 ? (int8_t) -2 : (int8_t)(rng() & 3);
	for(int32_t k = 0; k < q; ++k) if(near[(size_t) k] >= 0) for(size_t j = 0; j < sL; ++j)
		qs[(size_t) k * sL + j] = rng() % 20 == 0 ? (int8_t)(rng() & 3) : seq[(size_t) near[(size_t) k] * sL + j];
	std::vector<int32_t> parent(parent0), off(N + 1, 0), idx(N - 1, 0), node((size_t) q, -1);
	parent.resize(N, -1);
	std::vector<double> blen(N, 0.0);
	for(int32_t i = 0; i < n; ++i) blen[(size_t) i] = parent[(size_t) i] >= 0 ? 0.1 + 0.01 * i : 0.0;
	child_arrays(parent, (size_t) n, &off, &idx);
	hu_add_opts o;
	hu_add_default_opts(&o);
	o.blen.host = 1; o.blen.max_rounds = 30;
	/* the scores: no NaN, the root's entries, the best edge, and the predicted f against the log-likelihood of the grown arrays */
	std::vector<double> ts((size_t) q * (size_t) n), f((size_t) q * (size_t) n), bt((size_t) q), bf((size_t) q);
	std::vector<int32_t> bw((size_t) q);
	REQUIRE(hu_add_host_scores_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, q, qs.data(), ts.data(), f.data(), bw.data(), bt.data(), bf.data()) == HU_OK);
	HuBlenTopo tp;
	REQUIRE(hu_blen_check("driver", &o.blen, n, L, parent.data(), blen.data(), seq.data(), 0, &tp) == HU_OK);
	for(int32_t k = 0; k < q; ++k) {
		REQUIRE(ts[(size_t) k * n + tp.root] == 0.0 && f[(size_t) k * n + tp.root] == -INFINITY && bw[(size_t) k] != tp.root && bw[(size_t) k] >= 0 && bw[(size_t) k] < n);
		for(int32_t w = 0; w < n; ++w) if(w != tp.root) {
			const double x = f[(size_t) k * n + w], t = ts[(size_t) k * n + w];
			REQUIRE(std::isfinite(x) && t >= 0 && t <= 10 && x <= bf[(size_t) k]);
		}
		REQUIRE(bf[(size_t) k] == f[(size_t) k * n + bw[(size_t) k]] && bt[(size_t) k] == ts[(size_t) k * n + bw[(size_t) k]]);
		if(near[(size_t) k] >= 0 && L > 50) REQUIRE(bw[(size_t) k] == near[(size_t) k]);
		/* grown by hand on copies with room for two nodes */
		std::vector<int32_t> p2(parent.begin(), parent.begin() + n + 2), o2(off.begin(), off.begin() + n + 3), i2(idx.begin(), idx.begin() + n + 1);
		std::vector<double> b2(blen.begin(), blen.begin() + n + 2);
		std::vector<int8_t> s2(seq.begin(), seq.begin() + (long)((size_t)(n + 2) * sL));
		REQUIRE(hu_add_apply("driver", n, p2.data(), b2.data(), o2.data(), i2.data(), bw[(size_t) k], bt[(size_t) k], 0.0, 10.0) == HU_OK);
		REQUIRE(p2[(size_t) n + 1] == n && p2[(size_t) bw[(size_t) k]] == n && o2[(size_t) n + 2] == n + 1 && i2[(size_t) n - 1] == bw[(size_t) k] && i2[(size_t) n] == n + 1);
		memcpy(s2.data() + (size_t)(n + 1) * sL, qs.data() + (size_t) k * sL, sL);
		HuBlenTopo t2;
		REQUIRE(hu_blen_check("driver", &o.blen, n + 2, L, p2.data(), b2.data(), s2.data(), 0, &t2) == HU_OK);
		std::vector<double> up((size_t)(n + 2) * sL * 4);
		hu_blen_host_sweep(t2, m, p2.data(), L, b2.data(), s2.data(), up.data(), nullptr);
		const double ll = hu_blen_host_loglik(m, L, up.data() + (size_t) t2.root * sL * 4);
		REQUIRE(std::fabs(ll - bf[(size_t) k]) <= 1e-12 * std::fabs(ll));
	}
	/* the search, with a slab and a tile of one against the default */
	std::vector<hu_add_round> rounds((size_t) q);
	std::vector<hu_add_insert> ins((size_t) q);
	o.rounds = rounds.data(); o.rounds_cap = q; o.inserts = ins.data(); o.inserts_cap = q;
	double sec[4] = {0, 0, 0, 0};
	std::vector<int32_t> pB(parent), oB(off), iB(idx), nodeB(node);
	std::vector<double> bB(blen);
	std::vector<int8_t> sB(seq);
	REQUIRE(hu_add_host_search_entry("driver", &o, n, L, q, parent.data(), blen.data(), seq.data(), off.data(), idx.data(), qs.data(), node.data(), m, sec) == HU_OK);
	REQUIRE(o.n_inserted == q && o.n_rounds >= 1 && o.n_rounds <= q && std::isfinite(o.ll_final));
	const int roundsTaken = o.n_rounds;
	HuBlenTopo tf;
	REQUIRE(hu_blen_check("driver", &o.blen, (int32_t) N, L, parent.data(), blen.data(), seq.data(), 0, &tf) == HU_OK);
	for(int32_t k = 0; k < q; ++k) {
		const int32_t v = node[(size_t) k];
		REQUIRE(v > n && v < (int32_t) N && tf.childOff[(size_t) v] == tf.childOff[(size_t) v + 1] && memcmp(seq.data() + (size_t) v * sL, qs.data() + (size_t) k * sL, sL) == 0);
	}
	REQUIRE(off[N] == (int32_t) N - 1);
	o.slab = 1; o.tile = 1;
	REQUIRE(hu_add_host_search_entry("driver", &o, n, L, q, pB.data(), bB.data(), sB.data(), oB.data(), iB.data(), qs.data(), nodeB.data(), m, sec) == HU_OK);
	REQUIRE(pB == parent && bB == blen && iB == idx && nodeB == node);
	g_searches++;
	return roundsTaken;
}

static void refusals() {
	std::vector<int32_t> parent = {-1, 0, 0, 0, -1, -1}, off(7, 0), idx(5, 0);
	std::vector<double> blen = {0, 0.1, 0.1, 0.1, 0, 0};
	child_arrays(parent, 4, &off, &idx);
	const std::vector<int32_t> p0 = parent;
	for(int32_t w : {0, 4}) { REQUIRE(hu_add_apply("driver", 4, parent.data(), blen.data(), off.data(), idx.data(), w, 0.1, 0.0, 10.0) == HU_ERR_ARG); g_refusals++; }
	for(double t : {-0.1, 10.5}) { REQUIRE(hu_add_apply("driver", 4, parent.data(), blen.data(), off.data(), idx.data(), 1, t, 0.0, 10.0) == HU_ERR_ARG); g_refusals++; }
	REQUIRE(parent == p0);
	hu_add_opts o;
	hu_add_default_opts(&o);
	o.blen.host = 1;
	std::vector<int8_t> seq = {-2, -2, 0, 1, 2, 3, 1, 1}, qs = {0, 4};
	HuBlenTopo tp;
	REQUIRE(hu_add_check("driver", &o, 4, 2, parent.data(), blen.data(), seq.data(), 1, qs.data(), true, 0, &tp) == HU_ERR_ARG); g_refusals++;
	qs[1] = 3; o.blen.mem_budget = 1000;
	REQUIRE(hu_add_check("driver", &o, 4, 2, parent.data(), blen.data(), seq.data(), 1, qs.data(), true, 0, &tp) == HU_ERR_NOMEM && strstr(g_err, "1000 bytes")); g_refusals++;
	o.blen.mem_budget = 0;
	REQUIRE(hu_add_check("driver", &o, 4, 2, parent.data(), blen.data(), seq.data(), 1, qs.data(), true, 0, &tp) == HU_OK);
}

int main() {
	run({-1, 0, 0, 0}, 1, {1}, 1);                                                  /* three leaves plus one query, one column */
	run({-1, 0, 0, 1, 1, 2, 2, 2, 2}, 257, {5, -1, 3}, 2);                          /* a node with four children, a query of gaps only */
	run({-1, 0, 0, 1, 1, 2, 2, 0}, 1, {3, -1}, 3);                                  /* five leaves at one column */
	const int r = run({-1, 0, 0, 1, 1, 2, 2}, 257, {3, 3}, 4);                      /* two queries on one edge */
	REQUIRE(r == 2);
	printf("two on one edge: %d rounds\n", r);
	refusals();
	printf("searches: %d\nrefusals: %d\n", g_searches, g_refusals);
	return 0;
}
