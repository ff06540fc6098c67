// The host half of hu_permanova (hu_permanova_host.cpp: the checks, the plan, the shuffle, the host path and the reader of a distance
// matrix) under AddressSanitizer + UBSan, as a stand-alone program.
//   permanova_driver <scratch file>
// Shapes: n = 3, n = 65 (a ragged second tile), a group of one, P = 1, and what the plan and the reader refuse.  Checked on every
// result: 0 <= SS_W(p) <= SS_T (1 + 2^-40), a labelling is a rearrangement of the observed one, a permutation that keeps the partition
// gives the observed bits, and a matrix written to a file reads back bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_permanova.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

static std::vector<double> points(std::mt19937_64& g, int n) {
	std::vector<double> x((size_t) n * 3), d((size_t) n * n, 0.0);
	for(auto& v : x) v = (double)(g() % 100000) / 1000.0;
	for(int i = 0; i < n; ++i) for(int j = i + 1; j < n; ++j) {
		double s = 0;
		for(int k = 0; k < 3; ++k) { const double t = x[(size_t) i * 3 + k] - x[(size_t) j * 3 + k]; s += t * t; }
		d[(size_t) i * n + j] = d[(size_t) j * n + i] = std::sqrt(s) + 1e-3;
	}
	return d;
}

static int run(int n, const std::vector<int32_t>& grp, int64_t perms, const std::vector<double>& d) {
	hu_permanova_opts o;
	hu_permanova_default_opts(&o);
	o.perms = perms; o.host = 1; o.seed = 7;
	HuPmPlan pl;
	if(hu_pm_plan("driver", n, d.data(), grp.data(), &o, pl) != HU_OK) FAIL("plan refused n %d", n);
	std::vector<double> ssw((size_t) perms, -1.0);
	double obs = -1;
	hu_pm_host_run(pl, d.data(), &obs, ssw.data());
	const double ssT = hu_pm_ss_total(n, d.data());
	hu_permanova_result r;
	hu_pm_result(pl, ssT, obs, ssw.data(), &r);
	if(!(obs >= 0 && obs <= ssT * (1 + 0x1p-40))) FAIL("SS_W %g, SS_T %g", obs, ssT);
	if(r.count_le < 0 || r.count_le > perms || !(r.p > 0 && r.p <= 1)) FAIL("count %lld p %g", (long long) r.count_le, r.p);
	std::vector<int32_t> lab((size_t)(perms * n));
	if(hu_permanova_labels(n, grp.data(), 7, 0, perms, lab.data()) != HU_OK) FAIL("labels");
	std::vector<int32_t> want(grp); std::sort(want.begin(), want.end());
	for(int64_t p = 0; p < perms; ++p) {
		if(!(ssw[(size_t) p] >= 0 && ssw[(size_t) p] <= ssT * (1 + 0x1p-40))) FAIL("SS_W(%lld) %g, SS_T %g", (long long) p, ssw[(size_t) p], ssT);
		std::vector<int32_t> g(lab.begin() + p * n, lab.begin() + (p + 1) * n), s(g);
		std::sort(s.begin(), s.end());
		if(s != want) FAIL("permutation %lld is no rearrangement of the labels", (long long) p);
		if(g == grp && memcmp(&ssw[(size_t) p], &obs, 8) != 0) FAIL("the observed labelling as permutation %lld gives other bits", (long long) p);
	}
	return 0;
}

static int refused(const char* what, int n, const std::vector<double>& d, const std::vector<int32_t>& g, int64_t perms) {
	hu_permanova_opts o;
	hu_permanova_default_opts(&o);
	o.perms = perms;
	HuPmPlan pl;
	if(hu_pm_plan("driver", n, d.data(), g.data(), &o, pl) != HU_ERR_ARG) FAIL("%s was taken", what);
	return 0;
}

int main(int argc, char** argv) {
	if(argc < 2) { fprintf(stderr, "usage: permanova_driver <scratch file>\n"); return 2; }
	std::mt19937_64 g(20240927);
	int done = 0;
	for(int n : {3, 4, 7, 64, 65}) for(int64_t perms : {(int64_t) 1, (int64_t) 40}) {
		const std::vector<double> d = points(g, n);
		std::vector<int32_t> grp((size_t) n);
		for(int a : {2, 3, n - 1}) {
			if(a > n - 1 || a < 2) continue;
			for(int i = 0; i < n; ++i) grp[(size_t) i] = i < a ? i : (int32_t)(g() % (uint64_t) a);
			if(run(n, grp, perms, d)) return 1;
			++done;
		}
		std::fill(grp.begin(), grp.end(), 0); grp[(size_t)(n - 1)] = 1;          /* a group of one */
		if(run(n, grp, perms, d)) return 1;
		++done;
	}
	{	/* the refusals */
		const std::vector<double> d = points(g, 4);
		if(refused("n = 2", 2, d, {0, 1}, 9)) return 1;
		if(refused("a negative label", 4, d, {0, -1, 1, 0}, 9)) return 1;
		if(refused("labels with a hole", 4, d, {0, 2, 2, 0}, 9)) return 1;
		if(refused("a label beyond n", 4, d, {0, 9, 1, 0}, 9)) return 1;
		if(refused("one group", 4, d, {0, 0, 0, 0}, 9)) return 1;
		if(refused("n groups", 4, d, {0, 1, 2, 3}, 9)) return 1;
		if(refused("no permutation", 4, d, {0, 1, 1, 0}, 0)) return 1;
		if(refused("too many permutations", 4, d, {0, 1, 1, 0}, 10000001)) return 1;
		std::vector<double> x = d; x[1] = -1; x[4] = -1;
		if(refused("a negative cell", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x = d; x[1] = x[4] = NAN;
		if(refused("a NaN", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x = d; x[1] = x[4] = INFINITY;
		if(refused("an infinite cell", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x = d; x[1] = x[4] = 0x1p512;
		if(refused("a cell whose square is not finite", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x = d; x[7] += 1;
		if(refused("an asymmetric matrix", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x = d; x[5] = 1;
		if(refused("a diagonal that is not zero", 4, x, {0, 1, 1, 0}, 9)) return 1;
		x.assign(16, 0.0);
		if(refused("a matrix of zeros", 4, x, {0, 1, 1, 0}, 9)) return 1;
		if(hu_permanova_need(0, 2, 1) != -1 || hu_permanova_need(3, 2, 1) != 8 * 9 + 2 * 3 * 256 + 8 * 256 + 8 * 256 + 16 + 6 + (1 << 20)) FAIL("hu_permanova_need");
		++done;
	}
	{	/* the reader */
		const int n = 5;
		const std::vector<double> d = points(g, n);
		FILE* f = fopen(argv[1], "w");
		if(!f) FAIL("cannot write %s", argv[1]);
		for(int j = 0; j < n; ++j) fprintf(f, "\ts %d", j);
		fprintf(f, "\n");
		for(int i = 0; i < n; ++i) { fprintf(f, "s %d", i); for(int j = 0; j < n; ++j) fprintf(f, "\t%.17g", d[(size_t) i * n + j]); fprintf(f, "\n"); }
		fclose(f);
		hu_dist_matrix* m = nullptr;
		if(hu_dist_matrix_read(argv[1], &m) != HU_OK) FAIL("a good matrix was refused");
		int64_t nn = 0;
		hu_dist_matrix_dims(m, &nn);
		if(nn != n || strcmp(hu_dist_matrix_sample(m, 4), "s 4") != 0 || *hu_dist_matrix_sample(m, 5) || memcmp(hu_dist_matrix_values(m), d.data(), d.size() * 8) != 0) FAIL("the matrix read back differs");
		hu_dist_matrix_free(m);
		static const char* const bad[] = {"", "a\tb\n", "\ta\tb\na\t0\t1\n", "\ta\tb\na\t0\t1\nb\t1\n", "\ta\tb\na\t0\t1\nc\t1\t0\n", "\ta\tb\na\t0\tx\nb\t1\t0\n",
			"\ta\ta\na\t0\t1\na\t1\t0\n", "\ta\tb\na\t0\t1\nb\t1\t0\nc\t1\t1\n", "\ta\t\na\t0\t1\n"};
		for(const char* text : bad) {
			f = fopen(argv[1], "w");
			if(!f) FAIL("cannot write %s", argv[1]);
			fputs(text, f); fclose(f);
			m = nullptr;
			if(hu_dist_matrix_read(argv[1], &m) != HU_ERR_IO || m) FAIL("a bad matrix was taken: '%s'", text);
		}
		std::string gone = std::string(argv[1]) + ".none";
		if(hu_dist_matrix_read(gone.c_str(), &m) != HU_ERR_IO) FAIL("a missing file was read");
		remove(argv[1]);
		++done;
	}
	printf("%d cases\n", done);
	return 0;
}
