// The host half of the fit under the discrete Gamma of rates (hmmufotu_amd/csrc/hu_gamma_host.cpp: the rates, the checks, the host path
// and the passes; with hu_blen_host.cpp for the sweep of a category and the rounds of a fit) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_tree_gamma.py builds and runs it): three leaves, a node with four children, 1 and 257 columns,
// rows without a symbol and identical rows, 1 and 16 categories, the refusals.  Every case also holds the pulley principle: f_u at the
// branch's own length is the tree's log-likelihood for every u; and with one category the scores are the fixed-rate ones, bit for bit.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_gamma.h"

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

/* one tree through the checks, the log-likelihood, the scores, the step and the fit */
static void run(const std::vector<int32_t>& parent, int32_t L, const std::vector<int8_t>& seq, int32_t K, double alpha, double start, double lo, double hi) {
	const int32_t n = (int32_t) parent.size();
	const HuBlenModel m = jc69();
	hu_gamma_opts o;
	hu_gamma_default_opts(&o);
	o.blen.min_len = lo; o.blen.max_len = hi; o.blen.max_rounds = 5; o.blen.host = 1; o.k = K; o.alpha = alpha; o.max_outer = 2;
	std::vector<hu_gamma_pass> rec(2);
	o.passes = rec.data(); o.passes_cap = 2;
	std::vector<double> blen((size_t) n, start);
	HuBlenTopo tp;
	REQUIRE(hu_gamma_check("driver", &o, n, L, parent.data(), blen.data(), seq.data(), 0, &tp) == HU_OK);
	std::unique_ptr<HuGammaRun> r(hu_gamma_host_run(tp, m, K, L, parent.data(), seq.data(), lo, hi));
	double rate[HU_MAX_DGK], sum = 0;
	REQUIRE(hu_gamma_rates(K, alpha > 0 ? alpha : 1.0, rate) == HU_OK);
	for(int c = 0; c < K; ++c) { REQUIRE(rate[c] > 0 && (c == 0 || rate[c] > rate[c - 1])); sum += rate[c]; }
	REQUIRE(std::fabs(sum - K) <= 1e-13);
	REQUIRE(r->set_rates(rate) == HU_OK && r->sweep(blen.data(), true) == HU_OK);
	std::vector<double> perCol((size_t) L), perCat((size_t) K * (size_t) L), ts((size_t) n), f((size_t) n), d1((size_t) n), d2((size_t) n);
	std::vector<uint8_t> capped((size_t) n);
	double ll = 0;
	REQUIRE(r->loglik(perCol.data(), perCat.data(), &ll) == HU_OK && std::isfinite(ll));
	int64_t nCap = -1;
	REQUIRE(r->step(blen.data(), ts.data(), f.data(), d1.data(), d2.data(), capped.data(), &nCap) == HU_OK && nCap == 0);
	for(int32_t u = 0; u < n; ++u) if(u != tp.root) {
		REQUIRE(std::fabs(f[(size_t) u] - ll) <= 1e-10 * std::fabs(ll) + 1e-12);
		REQUIRE(ts[(size_t) u] >= lo && ts[(size_t) u] <= hi);
	}
	if(K == 1) {
		/* one category of rate 1: the fixed-rate entries, bit for bit */
		const size_t cells = (size_t) n * (size_t) L * 4;
		std::vector<double> up(cells), down(cells), ts1((size_t) n), f1((size_t) n), g1((size_t) n), h1((size_t) n);
		hu_blen_host_sweep(tp, m, parent.data(), L, blen.data(), seq.data(), up.data(), down.data());
		REQUIRE(hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4) == ll);
		REQUIRE(hu_blen_host_step(tp, m, L, blen.data(), up.data(), down.data(), lo, hi, ts1.data(), f1.data(), g1.data(), h1.data(), nullptr) == 0);
		for(int32_t u = 0; u < n; ++u) REQUIRE(ts1[(size_t) u] == ts[(size_t) u] && f1[(size_t) u] == f[(size_t) u] && g1[(size_t) u] == d1[(size_t) u] && h1[(size_t) u] == d2[(size_t) u]);
	}
	double sec[5];
	REQUIRE(hu_gamma_fit_run("driver", &o, n, tp.root, blen.data(), *r, sec) == HU_OK);
	REQUIRE(o.ll_final >= o.ll_start && o.n_outer >= 1 && o.n_outer <= 2 && o.stop >= 0 && o.stop <= 2);
	REQUIRE(o.alpha_fit >= HU_GAMMA_ALPHA_MIN && o.alpha_fit <= HU_GAMMA_ALPHA_MAX && (alpha == 0 || (o.alpha_fit == alpha && o.n_outer == 1 && o.stop == HU_GAMMA_FIXED_ALPHA)));
	for(int32_t p = 1; p < o.n_outer; ++p) REQUIRE(rec[(size_t) p].ll >= rec[(size_t) p - 1].ll);
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
		run(star3, L, rows_for(star3, L, 1u + (unsigned) L, -1, -1, -1), 1, 0.5, 0.1, 0.0, 10.0);
		run(star3, L, rows_for(star3, L, 2u + (unsigned) L, 2, -1, -1), 4, 0.0, 0.1, 0.0, 10.0);       /* a row without a symbol; alpha estimated */
		run(star3, L, rows_for(star3, L, 3u + (unsigned) L, -1, 1, 3), 16, 0.3, 0.3, 0.0, 2.0);        /* identical rows */
		run(four, L, rows_for(four, L, 4u + (unsigned) L, -1, -1, -1), 1, 0.0, 0.1, 0.0, 10.0);
		run(four, L, rows_for(four, L, 5u + (unsigned) L, 3, 8, 9), L == 1 ? 16 : 2, 0.0, 0.05, 1e-6, 1.0);   /* both, and a positive min_len */
	}
	run(four, 33, rows_for(four, 33, 7u, -1, -1, -1), 16, 0.05, 0.1, 0.0, 10.0);                  /* the smallest alpha: rates down to 1e-25 */
	/* every row without a symbol: a flat objective, nothing to improve */
	{
		std::vector<int8_t> seq(star3.size() * 5, (int8_t) -2);
		run(star3, 5, seq, 4, 0.0, 0.1, 0.0, 10.0);
	}
	/* the refusals */
	{
		hu_gamma_opts o;
		hu_gamma_default_opts(&o);
		HuBlenTopo tp;
		std::vector<int8_t> seq(4 * 3, (int8_t) 0);
		std::vector<double> b(4, 0.1);
		double rate[HU_MAX_DGK];
		const int32_t twoRoots[4] = {-1, -1, 0, 0};
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_OK);
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, twoRoots, b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 4, &tp) == HU_ERR_ARG);
		for(int32_t k : {0, 17, -1}) { o.k = k; REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG); REQUIRE(hu_gamma_rates(k, 1.0, rate) == HU_ERR_ARG); }
		o.k = 4;
		for(double a : {0.01, 200.0, -1.0, (double) NAN}) { o.alpha = a; REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG); REQUIRE(hu_gamma_rates(4, a, rate) == HU_ERR_ARG); }
		o.alpha = 0; o.eps_ll = 0;
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.eps_ll = 0.01; o.max_outer = 0;
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_ARG);
		o.max_outer = 10; o.blen.mem_budget = 100;
		REQUIRE(hu_gamma_check("driver", &o, 4, 3, star3.data(), b.data(), seq.data(), 0, &tp) == HU_ERR_NOMEM);
		REQUIRE(strstr(g_err, "need 1051780 bytes") && strstr(g_err, "budget is 100 bytes"));
		REQUIRE(hu_gamma_need(4, 3, 4) == 64 * 4 * 12 + 12 + 8 * 5 * 3 + (1 << 20));
		REQUIRE(hu_gamma_need(4, 270, 4) - hu_gamma_need(4, 269, 4) == 64 * 4 * 4 + 4 + 8 * 5 + 4 * 32 * 4 * 270);     /* beyond LDS: the scratch of 4 branches */
	}
	printf("%d cases\n", g_cases);
	return 0;
}
