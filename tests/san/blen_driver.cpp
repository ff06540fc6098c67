// The host half of the branch-length fit (hmmufotu_amd/csrc/hu_blen_host.cpp: the checks, the host sweep, the step and the round loop)
// as a stand-alone program for AddressSanitizer + UBSan (tests/test_tree_blen.py builds and runs it): three leaves, a node with four
// children, 1 and 257 columns, rows without a symbol and identical rows, the refusals.  Every case also holds the pulley principle:
// f_u at the branch's own length is the tree's log-likelihood for every u.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_blen.h"

static char g_err[1024];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }

static int g_cases = 0;
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

/* one tree through the checks, the scores, the step and the rounds */
static void run(const std::vector<int32_t>& parent, int32_t L, const std::vector<int8_t>& seq, double start, double lo, double hi, int rounds) {
	const int32_t n = (int32_t) parent.size();
	const HuBlenModel m = jc69();
	hu_blen_opts o;
	hu_blen_default_opts(&o);
	o.min_len = lo; o.max_len = hi; o.max_rounds = rounds; o.host = 1;
	std::vector<hu_blen_round> rec((size_t) rounds);
	o.rounds = rec.data(); o.rounds_cap = rounds;
	std::vector<double> blen((size_t) n, start);
	HuBlenTopo tp;
	REQUIRE(hu_blen_check("driver", &o, n, L, parent.data(), blen.data(), seq.data(), 0, &tp) == HU_OK);
	const size_t cells = (size_t) n * (size_t) L * 4;
	std::vector<double> up(cells), down(cells), ts((size_t) n), f((size_t) n), d1((size_t) n), d2((size_t) n);
	std::vector<uint8_t> capped((size_t) n);
	hu_blen_host_sweep(tp, m, parent.data(), L, blen.data(), seq.data(), up.data(), down.data());
	const double ll = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4);
	REQUIRE(std::isfinite(ll));
	const int64_t nCap = hu_blen_host_step(tp, m, L, blen.data(), up.data(), down.data(), lo, hi, ts.data(), f.data(), d1.data(), d2.data(), capped.data());
	REQUIRE(nCap == 0);
	for(int32_t u = 0; u < n; ++u) if(u != tp.root) {
		REQUIRE(std::fabs(f[(size_t) u] - ll) <= 1e-10 * std::fabs(ll) + 1e-12);
		REQUIRE(ts[(size_t) u] >= lo && ts[(size_t) u] <= hi);
	}
	HuBlenOps ops;
	ops.sweep = [&](const double* b, bool withDown) { hu_blen_host_sweep(tp, m, parent.data(), L, b, seq.data(), up.data(), withDown ? down.data() : nullptr); return HU_OK; };
	ops.loglik = [&](double* out) { *out = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4); return HU_OK; };
	ops.step = [&](const double* b, double* t, int64_t* c) { *c = hu_blen_host_step(tp, m, L, b, up.data(), down.data(), lo, hi, t, nullptr, nullptr, nullptr, nullptr); return HU_OK; };
	double sec[4] = {0, 0, 0, 0};
	REQUIRE(hu_blen_rounds("driver", &o, n, tp.root, blen.data(), ops, sec) == HU_OK);
	REQUIRE(o.ll_final >= o.ll_start && o.n_rounds <= rounds && o.stop >= 0 && o.stop <= 2);
	for(int32_t r = 1; r < o.n_rounds; ++r) REQUIRE(rec[(size_t) r].ll > rec[(size_t) r - 1].ll);
	for(int32_t u = 0; u < n; ++u) if(u != tp.root) REQUIRE(blen[(size_t) u] >= lo && blen[(size_t) u] <= hi);
	++g_cases;
}

static std::vector<int8_t> rows_for(const std::vector<int32_t>& parent, int32_t L, unsigned seed, int gapRow, int copyFrom, int copyTo) {
	const size_t n = parent.size();
	std::vector<char> inner(n, 0);
	for(size_t i = 0; i < n; ++i) if(parent[i] >= 0) inner[(size_t) parent[i]] = 1;
	std::mt19937 rng(seed);
	std::vector<int8_t> base((size_t) L), seq(n * (size_t) L, (int8_t) -2);
	for(auto& b : base) b = (int8_t)(rng() & 3);
	for(size_t i = 0; i < n; ++i) if(!inner[i]) for(int32_t j = 0; j < L; ++j) {
		const unsigned x = rng() % 100;
		seq[i * (size_t) L + (size_t) j] = x < 12 ? (int8_t)(rng() & 3) : x < 17 ? (int8_t) -2 : base[(size_t) j];
	}
	if(gapRow >= 0) for(int32_t j = 0; j < L; ++j) seq[(size_t) gapRow * (size_t) L + (size_t) j] = -2;
	if(copyFrom >= 0) memcpy(&seq[(size_t) copyTo * (size_t) L], &seq[(size_t) copyFrom * (size_t) L], (size_t) L);
	return seq;
}

int main() {
	/* three leaves on a root; leaves 1..3 */
	const std::vector<int32_t> star3 = {-1, 0, 0, 0};
	/* a bifurcating root, a node with four children (node 2), a cherry (node 7 with the leaves 8 and 9) */
	const std::vector<int32_t> four = {-1, 0, 0, 2, 2, 2, 2, 1, 7, 7, 1};
	for(int32_t L : {1, 257}) {
		run(star3, L, rows_for(star3, L, 1u + (unsigned) L, -1, -1, -1), 0.1, 0.0, 10.0, 20);
		run(star3, L, rows_for(star3, L, 2u + (unsigned) L, 2, -1, -1), 0.1, 0.0, 10.0, 20);       /* a row without a symbol */
		run(star3, L, rows_for(star3, L, 3u + (unsigned) L, -1, 1, 3), 0.3, 0.0, 2.0, 20);        /* identical rows */
		run(four, L, rows_for(four, L, 4u + (unsigned) L, -1, -1, -1), 0.1, 0.0, 10.0, 20);
		run(four, L, rows_for(four, L, 5u + (unsigned) L, 3, 8, 9), 0.05, 1e-6, 1.0, 20);          /* both, and a positive min_len */
	}
	/* every row without a symbol: a flat objective, nothing to improve */
	{
		std::vector<int8_t> seq(star3.size() * 5, (int8_t) -2);
		run(star3, 5, seq, 0.1, 0.0, 10.0, 3);
	}
	/* a start far off on a star: the full step is rejected */
	{
		const std::vector<int32_t> star6 = {-1, 0, 0, 0, 0, 0, 0};
		run(star6, 64, rows_for(star6, 64, 9u, -1, -1, -1), 2.0, 0.0, 10.0, 30);
	}
	/* the refusals */
	{
		hu_blen_opts o;
		hu_blen_default_opts(&o);
		HuBlenTopo tp;
		std::vector<int8_t> seq(4 * 3, (int8_t) 0);
		std::vector<double> b(4, 0.1);
		const int32_t twoRoots[4] = {-1, -1, 0, 0}, loop[4] = {-1, 2, 1, 0}, range[4] = {-1, 0, 9, 0};
		REQUIRE(hu_blen_check("driver", &o, 4, 3, twoRoots, b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		REQUIRE(hu_blen_check("driver", &o, 4, 3, loop, b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		REQUIRE(hu_blen_check("driver", &o, 4, 3, range, b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		REQUIRE(hu_blen_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 4, &tp) == HU_ERR_ARG);
		REQUIRE(hu_blen_check("driver", &o, 4, 0, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		seq[5] = 4;
		REQUIRE(hu_blen_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		seq[5] = 0; b[2] = NAN;
		REQUIRE(hu_blen_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		b[2] = 0.1; o.mem_budget = 100;
		REQUIRE(hu_blen_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_NOMEM);
		o.mem_budget = 0; o.eps = 1e-9;
		REQUIRE(hu_blen_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		REQUIRE(hu_blen_need(4, 3) == 65 * 12 + 24 + (1 << 20));
	}
	printf("%d cases\n", g_cases);
	return 0;
}
