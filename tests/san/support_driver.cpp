// The host half of the local branch supports (hmmufotu_amd/csrc/hu_support_host.cpp with hu_nni_host.cpp and hu_blen_host.cpp: the
// checks, the weights, the per-column values, the sums and the counts) as a stand-alone program for AddressSanitizer + UBSan
// (tests/test_tree_support.py builds and runs it): the weights at one column and at 65,535, a three-leaf tree, a polytomy, one replicate
// and 257, and the refusals.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_support.h"

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

/* leaf rows around a base row: 4 % of the cells another base, 3 % gaps */
static std::vector<int8_t> rows_for(const std::vector<int32_t>& parent, int32_t L, unsigned seed) {
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
	return seq;
}

static int g_trees = 0;

static void run(const std::vector<int32_t>& parent, int32_t L, int32_t B, int wantEdges, int64_t wantSkipped, bool withSums) {
	const int32_t n = (int32_t) parent.size();
	const HuBlenModel m = jc69();
	const std::vector<int8_t> seq = rows_for(parent, L, 11u + (unsigned) n);
	hu_support_opts o;
	hu_support_default_opts(&o);
	REQUIRE(o.replicates == 1000 && o.seed == 1);
	o.blen.host = 1; o.replicates = B; o.seed = 0x100000003ull;
	std::vector<double> blen((size_t) n, 0.1);
	const int32_t cap = n / 2 > 0 ? n / 2 : 1;
	std::vector<int32_t> node((size_t) cap), count((size_t) cap, -1); std::vector<double> ts((size_t) cap * 3), f((size_t) cap * 3), sums((size_t) cap * (size_t) B * 2);
	int32_t E = -1; int64_t skipped = -1; double sec[4];
	REQUIRE(hu_support_host_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, cap, &E, &skipped, node.data(), ts.data(), f.data(), count.data(),
		withSums ? sums.data() : nullptr, sec) == HU_OK);
	REQUIRE(E == wantEdges && skipped == wantSkipped);
	for(int32_t e = 0; e < E; ++e) {
		REQUIRE(count[(size_t) e] >= 0 && count[(size_t) e] <= B);
		if(!withSums) continue;
		int32_t c = 0;
		const double eta = hu_support_eta(f[(size_t) e * 3]);
		for(int32_t b = 0; b < B; ++b) {
			const double* s = &sums[((size_t) e * (size_t) B + (size_t) b) * 2];
			REQUIRE(!std::isnan(s[0]) && !std::isnan(s[1]));
			c += hu_support_supports(s[0], s[1], eta) ? 1 : 0;
		}
		REQUIRE(c == count[(size_t) e]);
	}
	/* a smaller budget than the need is refused with both numbers; the need itself passes */
	o.blen.mem_budget = hu_support_need(n, L, B);
	REQUIRE(hu_support_host_entry("driver", &o, n, L, parent.data(), blen.data(), seq.data(), m, cap, &E, &skipped, node.data(), ts.data(), f.data(), count.data(), nullptr, sec) == HU_OK);
	++g_trees;
}

int main() {
	/* the weights: one column, and the widest alignment a count of 16 bits holds */
	int weights = 0;
	{
		std::vector<uint16_t> w(5);
		REQUIRE(hu_support_weights(1, 5, 7, w.data()) == HU_OK);
		for(uint16_t x : w) REQUIRE(x == 1);
		++weights;
		std::vector<uint16_t> big((size_t) 2 * 65535);
		REQUIRE(hu_support_weights(65535, 2, 7, big.data()) == HU_OK);
		for(int b = 0; b < 2; ++b) { int64_t s = 0; for(int j = 0; j < 65535; ++j) s += big[(size_t) b * 65535 + (size_t) j]; REQUIRE(s == 65535); }
		std::vector<uint16_t> one(65535);
		REQUIRE(hu_support_weights(65535, 1, 7, one.data()) == HU_OK && memcmp(one.data(), big.data(), 65535 * 2) == 0);
		++weights;
	}
	printf("weights: %d\n", weights);
	/* three leaves: no eligible edge; a polytomy: its edge is skipped; a bifurcating root over two cherries with one replicate; eleven
	 * leaves under a trifurcating top node with 257 replicates and their sums */
	run({-1, 0, 0, 0}, 9, 4, 0, 0, true);
	run({-1, 0, 1, 2, 2, 1, 1, 0}, 40, 3, 0, 1, true);
	run({-1, 0, 1, 1, 0, 4, 4}, 33, 1, 1, 0, true);
	run({-1, 0, 1, 2, 2, 1, 5, 5, 0, 8, 8, 10, 10, 0, 13, 13, 15, 15, 17, 17}, 70, 257, 8, 0, true);
	printf("trees: %d\n", g_trees);
	/* the refusals */
	int refusals = 0;
	{
		const std::vector<int32_t> parent = {-1, 0, 1, 1, 0, 4, 4};
		const std::vector<int8_t> seq = rows_for(parent, 20, 3);
		const HuBlenModel m = jc69();
		std::vector<double> blen(7, 0.1), ts(9), f(9);
		std::vector<int32_t> node(3), count(3);
		int32_t E; int64_t skipped; double sec[4];
		hu_support_opts o;
		auto call = [&](int32_t cap) { return hu_support_host_entry("driver", &o, 7, 20, parent.data(), blen.data(), seq.data(), m, cap, &E, &skipped, node.data(), ts.data(), f.data(), count.data(), nullptr, sec); };
		hu_support_default_opts(&o); o.blen.host = 1; o.replicates = 0;
		REQUIRE(call(3) == HU_ERR_ARG && strstr(g_err, "replicates")); ++refusals;
		o.replicates = HU_SUPPORT_MAX_REPLICATES + 1;
		REQUIRE(call(3) == HU_ERR_ARG); ++refusals;
		o.replicates = 10; o.blen.mem_budget = 1000;
		REQUIRE(call(3) == HU_ERR_NOMEM && strstr(g_err, "budget is 1000 bytes")); ++refusals;
		o.blen.mem_budget = 0;
		REQUIRE(call(0) == HU_ERR_ARG && strstr(g_err, "eligible edges")); ++refusals;
		std::vector<uint16_t> w(4);
		REQUIRE(hu_support_weights(0, 1, 1, w.data()) == HU_ERR_ARG && hu_support_weights(65536, 1, 1, w.data()) == HU_ERR_ARG && hu_support_weights(4, 0, 1, w.data()) == HU_ERR_ARG
			&& hu_support_weights(4, 1, 1, nullptr) == HU_ERR_ARG); ++refusals;
		REQUIRE(call(3) == HU_OK && E == 1);
	}
	printf("refusals: %d\n", refusals);
	return 0;
}
