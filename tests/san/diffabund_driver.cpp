// The host half of hu_diffabund (hu_diffabund_host.cpp: the checks, the totals, the ranking, L, the cells, the host path, maxT and BH)
// under AddressSanitizer + UBSan, as a stand-alone program.
//   diffabund_driver
// Shapes: n = 3, 4, 65 and 300, two to sixty-four groups, a group of one, one OTU and many, P = 1, both ways of ranking, a prevalence
// floor, group sizes whose L needs more than 32 bits, and what the plan refuses.  Checked on every result: the doubled ranks of a row
// add to N (N + 1), 0 <= count_ge <= P, p <= p_maxT <= 1 (H is monotone in T, so a permutation counted for p is counted for maxT),
// p <= q <= 1, T of a relabelling that is the observed one equals the observed T, and an untested OTU carries NaN.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_diffabund.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

static std::vector<double> table(std::mt19937_64& g, int M, int n) {
	std::vector<double> c((size_t) M * n, 0.0);
	for(auto& v : c) if(g() % 3 == 0) v = (double)(1 + g() % 4);
	for(int j = 0; j < n; ++j) c[(size_t)(M - 1) * n + j] += 1 + (double)(g() % 2);
	if(M >= 4) for(int j = 0; j < n; ++j) { c[j] = 0; c[(size_t) n + j] = 7; }          /* an all-zero row and an all-equal one */
	return c;
}

static int run(int M, int n, const std::vector<int32_t>& grp, int64_t perms, int rank_by, int64_t min_prev, std::mt19937_64& g) {
	const std::vector<double> c = table(g, M, n);
	hu_diffabund_opts o;
	hu_diffabund_default_opts(&o);
	o.perms = perms; o.host = 1; o.seed = 7; o.rank_by = rank_by; o.min_prevalence = min_prev;
	HuDaPlan pl;
	if(hu_da_plan("driver", M, n, c.data(), grp.data(), &o, pl) != HU_OK) FAIL("plan refused M %d n %d", M, n);
	const size_t m = pl.row.size();
	std::vector<uint64_t> tobs(2 * m); std::vector<double> hobs(m), mx((size_t) perms, -1.0); std::vector<int64_t> count(m, -1);
	hu_da_host_run(pl, tobs.data(), hobs.data(), count.data(), mx.data());
	std::vector<hu_diffabund_rec> rec((size_t) M);
	hu_da_result(pl, tobs.data(), hobs.data(), count.data(), mx.data(), rec.data());
	std::vector<int32_t> r2((size_t) M * n);
	if(hu_diffabund_ranks(M, n, c.data(), rank_by, r2.data()) != HU_OK) FAIL("ranks");
	for(int i = 0; i < M; ++i) {
		int64_t s = 0;
		for(int j = 0; j < n; ++j) s += r2[(size_t) i * n + j];
		if(s != (int64_t) n * (n + 1)) FAIL("the doubled ranks of OTU %d add to %lld", i, (long long) s);
		const hu_diffabund_rec& x = rec[(size_t) i];
		if(!x.tested) { if(x.H == x.H || x.p == x.p || x.best != -1) FAIL("untested OTU %d carries values", i); continue; }
		if(x.count_ge < 0 || x.count_ge > perms || !(x.p > 0 && x.p <= 1)) FAIL("OTU %d: count %lld p %g", i, (long long) x.count_ge, x.p);
		if(!(x.p_maxT >= x.p && x.p_maxT <= 1) || !(x.q >= x.p && x.q <= 1)) FAIL("OTU %d: p %g p_maxT %g q %g", i, x.p, x.p_maxT, x.q);
		if(!(x.H >= 0) || x.best < 0 || x.best >= pl.a) FAIL("OTU %d: H %g best %d", i, x.H, x.best);
	}
	std::vector<uint8_t> lab((size_t) n);
	for(int64_t p = 0; p < perms; ++p) {
		hu_da_host_shuffle(pl, (uint64_t) p, lab.data());
		std::vector<uint8_t> s(lab), want(pl.lab);
		std::sort(s.begin(), s.end()); std::sort(want.begin(), want.end());
		if(s != want) FAIL("permutation %lld is no rearrangement of the labels", (long long) p);
		if(lab == pl.lab) for(size_t r = 0; r < m; ++r) {
			uint64_t hi, lo;
			hu_da_host_T(pl, (int64_t) r, lab.data(), &hi, &lo, nullptr);
			if(hi != tobs[2 * r] || lo != tobs[2 * r + 1]) FAIL("the observed labelling as permutation %lld gives another T", (long long) p);
		}
	}
	return 0;
}

static std::vector<int32_t> labels(std::mt19937_64& g, int n, int a) {
	std::vector<int32_t> l((size_t) n);
	for(int i = 0; i < n; ++i) l[(size_t) i] = i < a ? i : (int32_t)(g() % (uint64_t) a);
	std::shuffle(l.begin(), l.end(), g);
	return l;
}

int main() {
	std::mt19937_64 g(11);
	int cases = 0;
	const int shape[][3] = {{3, 2, 5}, {4, 2, 5}, {4, 3, 5}, {7, 6, 9}, {65, 2, 9}, {65, 3, 70}, {65, 64, 9}, {300, 64, 2}};
	for(const auto& s : shape) for(int rank_by = 0; rank_by < 2; ++rank_by) {
		if(run(s[2], s[0], labels(g, s[0], s[1]), s[0] <= 7 ? 99 : 20, rank_by, 1, g)) return 1;
		++cases;
	}
	if(run(9, 9, {0, 1, 1, 1, 1, 1, 1, 1, 1}, 50, 0, 1, g)) return 1;                    /* a group of one */
	++cases;
	if(run(9, 17, labels(g, 17, 3), 1, 0, 3, g)) return 1;                               /* P = 1, a prevalence floor */
	++cases;
	{	/* groups of 2, 3, 5, .., 37: L = 7,420,738,134,810 */
		const int primes[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
		std::vector<int32_t> l;
		for(int k = 0; k < 12; ++k) for(int i = 0; i < primes[k]; ++i) l.push_back(k);
		if(run(5, (int) l.size(), l, 9, 0, 1, g)) return 1;
		++cases;
	}
	/* what the plan refuses */
	{
		const std::vector<double> c = table(g, 6, 5);
		hu_diffabund_opts o;
		hu_diffabund_default_opts(&o);
		HuDaPlan pl;
		auto refused = [&](const std::vector<double>& t, int M, int n, const std::vector<int32_t>& l) { g_err[0] = 0; return hu_da_plan("driver", M, n, t.data(), l.data(), &o, pl) == HU_ERR_ARG && g_err[0]; };
		if(!refused(c, 6, 2, {0, 1})) FAIL("two samples");
		if(!refused(c, 6, 5, {0, 0, 0, 0, 0})) FAIL("one group");
		if(!refused(c, 6, 5, {0, 2, 0, 2, 2})) FAIL("labels with a hole");
		if(!refused(c, 6, 5, {0, 1, 2, 3, 4})) FAIL("groups of one");
		std::vector<double> bad(c); bad[7] = -1;
		if(!refused(bad, 6, 5, {0, 1, 0, 1, 1})) FAIL("a negative cell");
		if(!refused(std::vector<double>(15, 1.0), 3, 5, {0, 1, 0, 1, 1})) FAIL("every OTU untested");
		o.perms = 0;
		if(!refused(c, 6, 5, {0, 1, 0, 1, 1})) FAIL("no permutation");
		o.perms = 9;
		/* sixteen groups of the first sixteen primes: L is 2^64 or more */
		const int primes[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53};
		std::vector<int32_t> l;
		for(int k = 0; k < 16; ++k) for(int i = 0; i < primes[k]; ++i) l.push_back(k);
		if(!refused(std::vector<double>(2 * l.size(), 1.0), 2, (int) l.size(), l) || !strstr(g_err, "2^64")) FAIL("L beyond 64 bits");
		cases += 5;
	}
	printf("%d cases\n", cases);
	return 0;
}
