// The host half of hu_alpha (hu_alpha_host.cpp: the checks, the plan, the host path, the metrics, the curve) with hu_unifrac_host.cpp
// (the tree walk) and hu_otu_table.cpp (the cell checks, the keys) under AddressSanitizer + UBSan, as a stand-alone program: random
// trees and tables of every degenerate shape.
//   alpha_driver <trials>
// Checked on every result: the whole sample's statistics against plain loops over the column; a draw's S, F1, F2, Q consistent with its
// depth (S <= m, F1 + 2 F2 <= m, m <= Q <= m^2); the kept sets nested in the depth, so S and PD never fall as the depth grows; the
// depth N_j equal to the whole sample bit for bit; draws beyond N_j absent; every metric finite and in its range.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_alpha.h"

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

static int run(const Case& c, bool tree, int keyBits, uint64_t seed, int64_t reps) {
	const size_t M = (size_t) c.M, S = (size_t) c.S;
	std::vector<uint64_t> tot(S, 0);
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) tot[j] += (uint64_t) c.counts[i * S + j];
	uint64_t lo = tot[0], hi = tot[0];
	for(uint64_t t : tot) { lo = std::min(lo, t); hi = std::max(hi, t); }
	std::vector<uint64_t> depths = {1};
	for(uint64_t m : {(uint64_t) 2, lo - 1, lo, lo + 1, hi}) if(m > depths.back()) depths.push_back(m);
	hu_alpha_opts o;
	hu_alpha_default_opts(&o);
	o.host = 1; o.key_bits = keyBits; o.chunk = 64;
	hu_unifrac_tree t; t.n_nodes = (int32_t) c.parent.size(); t.parent = c.parent.data(); t.blen = c.blen.data();
	HuAlPlan pl;
	if(hu_al_plan("driver", tree ? &t : nullptr, c.M, c.S, tree ? c.node.data() : nullptr, c.counts.data(), (int64_t) depths.size(), depths.data(), reps, seed, &o, pl) != HU_OK)
		FAIL("plan refused M %lld S %lld", (long long) c.M, (long long) c.S);
	std::vector<HuAlStat> stat;
	hu_al_host(pl, stat);
	const size_t nD = depths.size(), R = (size_t) reps;
	std::vector<hu_alpha_rec> whole(S), draws(S * nD * R);
	hu_al_fill(pl, stat, whole.data(), draws.data());
	int64_t need = hu_alpha_need(c.S, (int64_t) pl.prefix.size() - c.S, (int64_t) pl.br.size(), pl.maxNnz, pl.maxChunk, (int64_t) pl.unit.size());
	if(need < (1 << 20)) FAIL("need %lld", (long long) need);
	for(size_t j = 0; j < S; ++j) {
		uint64_t s = 0, f1 = 0, f2 = 0, q = 0;
		for(size_t i = 0; i < M; ++i) { const uint64_t v = (uint64_t) c.counts[i * S + j]; s += v > 0; f1 += v == 1; f2 += v == 2; q += v * v; }
		const hu_alpha_rec& w = whole[j];
		if(w.reads != tot[j] || w.S != s || w.F1 != f1 || w.F2 != f2 || w.Q != q) FAIL("whole sample %zu: S %llu F1 %llu F2 %llu Q %llu", j, (unsigned long long) w.S, (unsigned long long) w.F1, (unsigned long long) w.F2, (unsigned long long) w.Q);
		if(!(w.shannon >= 0 && w.shannon <= std::log((double) s) + 1e-12) || !(w.simpson >= 0 && w.simpson < 1) || !(w.goods_coverage >= 0 && w.goods_coverage <= 1) || !(w.chao1 >= (double) s))
			FAIL("whole sample %zu: shannon %g simpson %g coverage %g chao1 %g", j, w.shannon, w.simpson, w.goods_coverage, w.chao1);
		if(tree ? !(w.PD >= 0 && std::isfinite(w.PD)) : w.PD == w.PD) FAIL("whole sample %zu: PD %g", j, w.PD);
		for(size_t r = 0; r < R; ++r) {
			uint64_t lastS = 0; double lastPD = 0;
			for(size_t d = 0; d < nD; ++d) {
				const hu_alpha_rec& x = draws[(j * nD + d) * R + r];
				const uint64_t m = depths[d];
				if(m > tot[j]) { if(x.reads != 0 || x.shannon == x.shannon) FAIL("sample %zu depth %llu beyond its %llu reads exists", j, (unsigned long long) m, (unsigned long long) tot[j]); continue; }
				if(x.reads != m || x.S > m || x.S < 1 || x.F1 + 2 * x.F2 > m || x.Q < m || x.Q > m * m || x.S > w.S) FAIL("sample %zu depth %llu: S %llu F1 %llu F2 %llu Q %llu", j, (unsigned long long) m, (unsigned long long) x.S, (unsigned long long) x.F1, (unsigned long long) x.F2, (unsigned long long) x.Q);
				if(x.S < lastS || (tree && x.PD < lastPD)) FAIL("sample %zu repeat %zu: not nested at depth %llu", j, r, (unsigned long long) m);
				lastS = x.S; lastPD = tree ? x.PD : 0;
				if(!(x.shannon >= 0) || !(x.simpson >= 0 && x.simpson < 1) || !std::isfinite(x.chao1)) FAIL("sample %zu depth %llu: shannon %g simpson %g", j, (unsigned long long) m, x.shannon, x.simpson);
				if(m == tot[j] && (memcmp(&x.S, &w.S, 4 * sizeof(uint64_t)) != 0 || memcmp(&x.A, &w.A, sizeof(double)) != 0 || memcmp(&x.PD, &w.PD, sizeof(double)) != 0))
					FAIL("sample %zu: the depth N_j is not the whole sample", j);
			}
		}
	}
	/* the curve of the observed OTUs of sample 0 at depth 1: every draw has one OTU */
	std::vector<double> x(R);
	for(size_t r = 0; r < R; ++r) x[r] = draws[r].observed;
	double mean = 0, sd = 0;
	if(hu_alpha_curve((int64_t) R, x.data(), &mean, &sd) != HU_OK || mean != 1.0 || (R > 1 ? sd != 0.0 : sd == sd)) FAIL("curve: mean %g sd %g", mean, sd);
	return 0;
}

int main(int argc, char** argv) {
	const int trials = argc > 1 ? atoi(argv[1]) : 20;
	std::mt19937_64 g(20240830);
	int done = 0;
	/* chains that keep exactly B branches, S around one wave; keys that tie */
	static const int Bs[] = {1, 63, 64, 65}, Ss[] = {1, 2, 5};
	for(int B : Bs) for(int S : Ss) for(int kb : {64, 4}) {
		Case c;
		make_tree(g, B + 5, true, c);
		const int64_t M = std::min(B, 6);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back(i == 0 ? B : (int32_t)(g() % (uint64_t)(B + 1)));
		fill(g, c, M, S, 50);
		if(run(c, true, kb, 7 + (uint64_t) done, kb == 4 ? 3 : 1)) return 1;
		++done;
	}
	/* one OTU; only the root; two rows on one node; no tree; a seed whose repeats wrap at 2^64 */
	{
		Case c;
		make_tree(g, 9, false, c);
		c.node = {5}; fill(g, c, 1, 3, 50);
		if(run(c, true, 64, 1, 2)) return 1;
		c.node = {0}; fill(g, c, 1, 2, 50);
		if(run(c, true, 64, 1, 2)) return 1;
		c.node = {4, 4, 0}; fill(g, c, 3, 5, 50);
		if(run(c, true, 8, ~0ull, 3) || run(c, false, 64, 3, 1)) return 1;
		done += 4;
	}
	for(int tr = 0; tr < trials; ++tr) {
		Case c;
		const int n = 1 + (int)(g() % 300);
		make_tree(g, n, g() % 4 == 0, c);
		const int64_t M = 1 + (int64_t)(g() % 300), S = 1 + (int64_t)(g() % 8);
		c.node.clear();
		for(int64_t i = 0; i < M; ++i) c.node.push_back((int32_t)(g() % (uint64_t) n));
		fill(g, c, M, S, g() % 2 ? 4 : 40);
		if(run(c, g() % 4 != 0, g() % 3 == 0 ? 6 : 64, g(), 1 + (int64_t)(g() % 3))) return 1;
		++done;
	}
	/* a cell of 2^32 - 1 alone in its sample: Q near 2^64 */
	{
		Case c; make_tree(g, 3, true, c); c.node = {2}; c.M = 1; c.S = 1; c.counts = {4294967295.0};
		hu_unifrac_tree t; t.n_nodes = 3; t.parent = c.parent.data(); t.blen = c.blen.data();
		HuAlPlan pl;
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 0, nullptr, 0, 1, nullptr, pl) != HU_OK) FAIL("the largest cell was refused");
		std::vector<HuAlStat> stat; hu_al_host(pl, stat);
		hu_alpha_rec w; hu_al_fill(pl, stat, &w, nullptr);
		if(w.Q != 18446744065119617025ull || w.shannon != 0.0 || w.simpson != 0.0) FAIL("the largest cell: Q %llu shannon %g simpson %g", (unsigned long long) w.Q, w.shannon, w.simpson);
		++done;
	}
	/* what the plan refuses */
	{
		Case c; make_tree(g, 4, false, c); c.node = {2}; fill(g, c, 1, 1, 50);
		hu_unifrac_tree t; t.n_nodes = 4; t.parent = c.parent.data(); t.blen = c.blen.data();
		HuAlPlan pl;
		const uint64_t zero[] = {0}, down[] = {2, 2};
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 1, zero, 1, 1, nullptr, pl) != HU_ERR_ARG) FAIL("a depth of 0 was taken");
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 2, down, 1, 1, nullptr, pl) != HU_ERR_ARG) FAIL("depths that do not ascend were taken");
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 1, down, 0, 1, nullptr, pl) != HU_ERR_ARG) FAIL("depths without repeats were taken");
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 1, down, -1, 1, nullptr, pl) != HU_ERR_ARG) FAIL("negative repeats were taken");
		c.node = {9};
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 0, nullptr, 0, 1, nullptr, pl) != HU_ERR_ARG) FAIL("a node outside the tree was taken");
		c.node = {2}; c.counts = {0.0};
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 0, nullptr, 0, 1, nullptr, pl) != HU_ERR_ARG) FAIL("a sample without reads was taken");
		c.counts = {1.5};
		if(hu_al_plan("driver", &t, 1, 1, c.node.data(), c.counts.data(), 0, nullptr, 0, 1, nullptr, pl) != HU_ERR_ARG) FAIL("a fraction was taken");
	}
	printf("%d cases\n", done);
	return 0;
}
