// The host half of hmmufotu-amd-tree (hu_nj_host.cpp: the checks, the host path of the counts, the distances and the joins, the
// Newick writer) under AddressSanitizer + UBSan, as a stand-alone program.
//   nj_driver <trials>
// Cases: n = 3 and 4, all-zero and all-equal matrices (every Q ties), a matrix whose first join takes the last slot as j (no move),
// random symmetric matrices up to n = 70 (more than one block of the row sums would need 257: one of that size too), rows with gaps
// and an all-gap row through the counts and every distance type.  Checked on every tree: every node is used once, the lengths are
// finite, the Newick text has n leaves and balanced brackets, and a second run gives the same bits.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_tree_nj.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

static int g_cases = 0;

static int run_nj(int64_t n, const std::vector<double>& D, int wantJ = -1) {
	if(hu_nj_check("driver", n, D.data()) != HU_OK) FAIL("matrix of %lld refused", (long long) n);
	const size_t m = (size_t)(n - 3);
	std::vector<int32_t> join[2]; std::vector<double> len[2]; int32_t l3[2][3]; double ll3[2][3];
	for(int rep = 0; rep < 2; ++rep) {
		join[rep].assign(2 * m, -1); len[rep].assign(2 * m, NAN);
		std::vector<double> work(D);
		hu_nj_host_run(n, work.data(), join[rep].data(), len[rep].data(), l3[rep], ll3[rep]);
	}
	if(join[0] != join[1] || (m > 0 && memcmp(len[0].data(), len[1].data(), 2 * m * 8) != 0) || memcmp(l3[0], l3[1], 12) != 0 || memcmp(ll3[0], ll3[1], 24) != 0) FAIL("two runs differ at n %lld", (long long) n);
	if(wantJ >= 0 && m > 0 && join[0][1] != wantJ) FAIL("the first join takes %d, expected %d", join[0][1], wantJ);
	std::vector<int> used((size_t)(2 * n - 3), 0);
	for(size_t t = 0; t < m; ++t) for(int s = 0; s < 2; ++s) {
		const int32_t v = join[0][2 * t + s];
		if(v < 0 || v >= (int32_t)(n + t) || used[(size_t) v]++) FAIL("join %zu names node %d", t, v);
		if(!std::isfinite(len[0][2 * t + s])) FAIL("join %zu has a length that is not finite", t);
	}
	for(int s = 0; s < 3; ++s) { if(l3[0][s] < 0 || l3[0][s] >= 2 * n - 3 || used[(size_t) l3[0][s]]++) FAIL("the top names node %d", l3[0][s]); if(!std::isfinite(ll3[0][s])) FAIL("top length"); }
	for(int u : used) if(u != 1) FAIL("a node is not used once");
	std::vector<std::string> names((size_t) n); std::vector<const char*> nm((size_t) n);
	for(int64_t i = 0; i < n; ++i) { names[(size_t) i] = (i % 7 == 3 ? "odd name " : "s") + std::to_string(i); nm[(size_t) i] = names[(size_t) i].c_str(); }
	const int64_t L = hu_nj_newick(n, nm.data(), join[0].data(), len[0].data(), l3[0], ll3[0], nullptr, 0);
	if(L < 0) FAIL("the writer refused");
	std::string text((size_t) L + 1, '\0');
	if(hu_nj_newick(n, nm.data(), join[0].data(), len[0].data(), l3[0], ll3[0], &text[0], L + 1) != L) FAIL("the writer's two calls differ");
	text.resize((size_t) L);
	int64_t open = 0, close = 0, colon = 0;
	for(char c : text) { open += c == '('; close += c == ')'; colon += c == ':'; }
	if(open != n - 2 || close != n - 2 || colon != 2 * n - 3 || text.compare(text.size() - 2, 2, ";\n") != 0) FAIL("Newick of n %lld: %lld ( %lld ) %lld :", (long long) n, (long long) open, (long long) close, (long long) colon);
	char small[8];
	if(hu_nj_newick(n, nm.data(), join[0].data(), len[0].data(), l3[0], ll3[0], small, sizeof(small)) != L || strlen(small) != 7) FAIL("a short buffer");
	++g_cases;
	return 0;
}

static std::vector<double> constant(int64_t n, double v) {
	std::vector<double> D((size_t)(n * n), v);
	for(int64_t i = 0; i < n; ++i) D[(size_t)(i * n + i)] = 0.0;
	return D;
}

int main(int argc, char** argv) {
	const int trials = argc > 1 ? atoi(argv[1]) : 20;
	std::mt19937_64 g(20251);
	for(int64_t n : {3, 4, 5, 9}) { if(run_nj(n, constant(n, 0.0))) return 1; if(run_nj(n, constant(n, 1.5))) return 1; }
	{   /* the closest pair is (1, n - 1): j is the last slot, nothing moves */
		const int64_t n = 6;
		std::vector<double> D = constant(n, 10.0);
		D[1 * n + 5] = D[5 * n + 1] = 1.0;
		if(run_nj(n, D, 5)) return 1;
	}
	for(int tr = 0; tr < trials; ++tr) {
		const int64_t n = tr == 0 ? 257 : 3 + (int64_t)(g() % 68);
		std::vector<double> D((size_t)(n * n), 0.0);
		const bool ints = tr % 2 == 0;
		for(int64_t i = 0; i < n; ++i) for(int64_t j = i + 1; j < n; ++j) {
			const double v = ints ? (double)(1 + g() % 1000) : (double)(g() % 100000) / 99991.0;
			D[(size_t)(i * n + j)] = v; D[(size_t)(j * n + i)] = v;
		}
		if(run_nj(n, D)) return 1;
	}
	/* refusals of the checks */
	{
		std::vector<double> D = constant(4, 1.0);
		D[1] = 2.0;
		if(hu_nj_check("driver", 4, D.data()) == HU_OK) FAIL("an asymmetric matrix passed");
		D[1] = 1.0; D[5] = 1.0;
		if(hu_nj_check("driver", 4, D.data()) == HU_OK) FAIL("a diagonal of 1 passed");
		D[5] = 0.0; D[2] = D[8] = INFINITY;
		if(hu_nj_check("driver", 4, D.data()) == HU_OK) FAIL("an infinite distance passed");
		if(hu_nj_check("driver", 2, D.data()) == HU_OK) FAIL("n = 2 passed");
		g_cases += 4;
	}
	/* the counts and the distances: gaps, an all-gap row, identical rows, a saturated pair */
	for(int tr = 0; tr < 6; ++tr) {
		const int64_t n = 5 + tr, L = tr == 0 ? 1 : 37 + 31 * tr;
		std::vector<int8_t> rows((size_t)(n * L));
		for(auto& c : rows) { const int k = (int)(g() % 6); c = (int8_t)(k < 4 ? k : k == 4 ? -2 : -1); }
		for(int64_t k = 0; k < L; ++k) { rows[(size_t)(1 * L + k)] = -2; rows[(size_t)(2 * L + k)] = rows[(size_t) k]; rows[(size_t)(3 * L + k)] = 0; rows[(size_t)(4 * L + k)] = 1; }
		std::vector<int32_t> cnt((size_t)(n * n * 4));
		hu_dist_host_counts(n, L, rows.data(), cnt.data());
		for(int64_t i = 0; i < n; ++i) if(cnt[(size_t)((1 * n + i) * 4)] != 0) FAIL("the all-gap row compares a column");
		if(cnt[(size_t)((0 * n + 2) * 4 + 1)] + cnt[(size_t)((0 * n + 2) * 4 + 2)] + cnt[(size_t)((0 * n + 2) * 4 + 3)] != 0) FAIL("identical rows differ");
		if(cnt[(size_t)((3 * n + 4) * 4 + 3)] != L) FAIL("A against C is not all transversions");
		const double pi[4] = {0.1, 0.2, 0.3, 0.4};
		for(int type = HU_DIST_PDIST; type <= HU_DIST_TN93; ++type) for(double sat : {0.0, 3.0}) {
			if(hu_dist_check("driver", n, L, rows.data(), type, pi, sat) != HU_OK) FAIL("rows refused");
			std::vector<double> D((size_t)(n * n), NAN); int64_t ns = -1;
			if(hu_dist_host("driver", n, L, rows.data(), type, pi, sat, D.data(), &ns) != HU_OK) FAIL("distances of type %d refused", type);
			/* A against C in every column: beyond every logarithm but HKY85's, whose argument stays positive for this pi */
			const bool mustSat = type != HU_DIST_PDIST && type != HU_DIST_HKY85;
			if((type == HU_DIST_PDIST && ns != 0) || (mustSat && ns < 1)) FAIL("type %d: %lld saturated pairs", type, (long long) ns);
			for(int64_t i = 0; i < n; ++i) for(int64_t j = 0; j < n; ++j) {
				const double a = D[(size_t)(i * n + j)], b = D[(size_t)(j * n + i)];
				if(!std::isfinite(a) || a < 0 || memcmp(&a, &b, 8) != 0 || (i == j && a != 0)) FAIL("type %d: D[%lld][%lld] = %g", type, (long long) i, (long long) j, a);
			}
			if(D[2] != 0.0 || D[1] != 0.0) FAIL("identical rows, or a row without symbols, at a distance");
			if(mustSat && sat > 0 && D[(size_t)(3 * n + 4)] != sat) FAIL("the saturated pair has %g", D[(size_t)(3 * n + 4)]);
			if(n >= 3 && run_nj(n, D)) return 1;
		}
		rows[0] = 4;
		if(hu_dist_check("driver", n, L, rows.data(), HU_DIST_JC69, nullptr, 0.0) == HU_OK) FAIL("a code of 4 passed");
	}
	printf("%d cases\n", g_cases);
	return 0;
}
