// The host half of hu_permanova_design (hu_permanova_design_host.cpp: the design builder, the checks, the plan, the index arrays and the
// host path; hu_design_file.h: the META reader) under AddressSanitizer + UBSan, as a stand-alone program.
//   permanova_design_driver <scratch file>
// Shapes: n = 4, 7 and 65, a factor, a covariate and their interaction, strata, a dropped column, P = 1, and what the builder, the plan
// and the reader refuse.  Checked on every result: the basis is orthonormal and centred to 1e-14, sum_t SS_t + SS_res = SS_T to 1e-9
// relatively, every index array is a permutation that keeps the strata, and the identity as a permutation gives the observed bits.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_permanova_design.h"
#include "../../hmmufotu_amd/csrc/hu_design_file.h"

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

static int run(std::mt19937_64& g, int n, int levels, bool interaction, bool strata, int64_t perms) {
	const std::vector<double> d = points(g, n);
	std::vector<double> cov((size_t) n); std::vector<int32_t> lab((size_t) n), st((size_t) n);
	for(int i = 0; i < n; ++i) { cov[(size_t) i] = (double)(g() % 1000) / 10.0; lab[(size_t) i] = i < levels ? i : (int32_t)(g() % (uint64_t) levels); st[(size_t) i] = i % 2; }
	hu_design_var var[2] = {{1, 0, nullptr, lab.data()}, {0, 0, cov.data(), nullptr}};
	hu_design_term term[3] = {{0, -1}, {1, -1}, {0, 1}};
	const int64_t T = interaction ? 3 : 2, raw = hu_design_raw_columns(n, 2, var, T, term);
	if(raw != (levels - 1) + 1 + (interaction ? levels - 1 : 0)) FAIL("raw columns %lld", (long long) raw);
	std::vector<double> Q((size_t)(n * raw));
	int64_t q = 0, ts[4], df[3], dropped[3];
	if(hu_design_build(n, 2, var, T, term, nullptr, Q.data(), &q, ts, df, dropped) != HU_OK) FAIL("build refused n %d", n);
	for(int64_t a = 0; a < q; ++a) for(int64_t b = 0; b <= a; ++b) {
		double dot = 0, sum = 0;
		for(int i = 0; i < n; ++i) { dot += Q[(size_t)(i * q + a)] * Q[(size_t)(i * q + b)]; sum += Q[(size_t)(i * q + a)]; }
		if(std::fabs(dot - (a == b ? 1 : 0)) > 1e-14 || std::fabs(sum) > 1e-14) FAIL("the basis: column %lld x %lld gives %g, its sum %g", (long long) a, (long long) b, dot, sum);
	}
	hu_permanova_design_opts o;
	hu_permanova_design_default_opts(&o);
	o.perms = perms; o.host = 1; o.seed = 7;
	HuPmdPlan pl;
	if(hu_pmd_plan("driver", n, d.data(), Q.data(), q, T, ts, strata ? st.data() : nullptr, &o, pl) != HU_OK) FAIL("plan refused n %d", n);
	std::vector<double> ss((size_t)((1 + perms) * T), -1.0);
	hu_pmd_host_run(pl, d.data(), Q.data(), ss.data());
	std::vector<hu_permanova_design_term> res((size_t) T);
	const double ssT = hu_pm_ss_total(n, d.data());
	hu_pmd_result(pl, ssT, ss.data(), res.data());
	double sum = res[0].ss_res;
	for(int64_t t = 0; t < T; ++t) { sum += res[(size_t) t].ss; if(res[(size_t) t].count_ge < 0 || res[(size_t) t].count_ge > perms || !(res[(size_t) t].p > 0 && res[(size_t) t].p <= 1)) FAIL("count or p of term %lld", (long long) t); }
	if(std::fabs(sum - ssT) > 1e-9 * ssT) FAIL("the sums of squares add to %g, SS_T %g", sum, ssT);
	std::vector<int64_t> idx((size_t)(perms * n));
	if(hu_permanova_perms(n, strata ? st.data() : nullptr, 7, 0, perms, idx.data()) != HU_OK) FAIL("perms");
	for(int64_t p = 0; p < perms; ++p) {
		std::vector<int64_t> row(idx.begin() + p * n, idx.begin() + (p + 1) * n), s(row);
		std::sort(s.begin(), s.end());
		bool identity = true;
		for(int i = 0; i < n; ++i) {
			if(s[(size_t) i] != i) FAIL("permutation %lld is no permutation", (long long) p);
			if(strata && st[(size_t) row[(size_t) i]] != st[(size_t) i]) FAIL("permutation %lld leaves its stratum", (long long) p);
			identity = identity && row[(size_t) i] == i;
		}
		if(identity && memcmp(&ss[(size_t)((1 + p) * T)], &ss[0], (size_t)(8 * T)) != 0) FAIL("the identity as permutation %lld gives other bits", (long long) p);
	}
	return 0;
}

static int plan_refused(const char* what, int n, const std::vector<double>& d, const std::vector<double>& Q, int64_t q, std::vector<int64_t> ts, const int32_t* strata, int64_t perms, int64_t chunk) {
	hu_permanova_design_opts o;
	hu_permanova_design_default_opts(&o);
	o.perms = perms; o.chunk = chunk;
	HuPmdPlan pl;
	if(hu_pmd_plan("driver", n, d.data(), Q.data(), q, (int64_t) ts.size() - 1, ts.data(), strata, &o, pl) != HU_ERR_ARG) FAIL("%s was taken", what);
	return 0;
}

static bool meta_of(const char* path, const char* text, const std::vector<std::string>& sample, HuMeta& m, std::string& err) {
	FILE* f = fopen(path, "w");
	if(!f) { err = "cannot write"; return false; }
	fputs(text, f); fclose(f);
	return hu_meta_read(path, sample, m, err);
}

int main(int argc, char** argv) {
	if(argc < 2) { fprintf(stderr, "usage: permanova_design_driver <scratch file>\n"); return 2; }
	std::mt19937_64 g(20250211);
	int done = 0;
	for(int n : {7, 65}) for(int64_t perms : {(int64_t) 1, (int64_t) 30}) for(int inter = 0; inter < 2; ++inter) for(int strata = 0; strata < 2; ++strata) {
		if(run(g, n, n == 7 ? 2 : 3, inter != 0, strata != 0, perms)) return 1;
		++done;
	}
	if(run(g, 4, 2, false, false, 30)) return 1;
	++done;
	{	/* the builder's refusals and a dropped column */
		const int n = 6;
		std::vector<double> c = {1, 2, 4, 8, 16, 32}, c2 = {3, 5, 9, 17, 33, 65}, bad = {1, 2, NAN, 4, 5, 6};
		std::vector<int32_t> lab = {0, 1, 2, 0, 1, 2}, hole = {0, 2, 2, 0, 2, 0}, neg = {0, -1, 1, 0, 1, 0}, same = {0, 1, 0, 0, 1, 0};
		std::vector<double> Q((size_t) n * 8);
		int64_t q, ts[4], df[3], dropped[3];
		hu_design_var v[3] = {{0, 0, c.data(), nullptr}, {0, 0, c2.data(), nullptr}, {1, 0, nullptr, lab.data()}};
		hu_design_term dup[2] = {{0, -1}, {1, -1}}, one[1] = {{2, -1}}, out[1] = {{5, -1}}, full[3] = {{2, -1}, {0, -1}, {2, 0}};
		const char* names[2] = {"c", "c2"};
		if(hu_design_build(n, 3, v, 2, dup, names, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG || !strstr(g_err, "'c2' adds nothing")) FAIL("a duplicated covariate was taken");
		if(hu_design_build(n, 3, v, 1, out, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG) FAIL("a term outside the variables was taken");
		if(hu_design_build(n, 3, v, 3, full, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG || !strstr(g_err, "residual")) FAIL("a saturated design was taken");
		if(hu_design_build(n, 3, v, 1, one, nullptr, Q.data(), &q, ts, df, dropped) != HU_OK || q != 2 || dropped[0] != 0) FAIL("a factor of three levels");
		/* the interaction of a factor with itself repeats its columns and adds zero columns: they are dropped, the term refused */
		hu_design_term self[2] = {{2, -1}, {2, 2}};
		if(hu_design_build(n, 3, v, 2, self, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG || !strstr(g_err, "adds nothing")) FAIL("g:g after g was taken");
		v[0].value = bad.data();
		if(hu_design_build(n, 3, v, 2, dup, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG) FAIL("a NaN was taken");
		v[0].value = c.data(); v[2].label = hole.data();
		if(hu_design_build(n, 3, v, 1, one, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG) FAIL("labels with a hole were taken");
		v[2].label = neg.data();
		if(hu_design_build(n, 3, v, 1, one, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG) FAIL("a negative label was taken");
		/* a covariate that a factor of two levels explains but for one column: kept 1, nothing dropped; then the same twice: one dropped */
		std::vector<double> ind = {0, 1, 0, 0, 1, 0};
		v[2].label = same.data(); v[1].value = ind.data();
		hu_design_term two[2] = {{2, -1}, {1, -1}};
		if(hu_design_build(n, 3, v, 2, two, nullptr, Q.data(), &q, ts, df, dropped) != HU_ERR_ARG || !strstr(g_err, "number 2")) FAIL("an indicator after its factor was taken");
		++done;
	}
	{	/* the plan's refusals */
		const int n = 6;
		const std::vector<double> d = points(g, n);
		std::vector<double> c = {1, 2, 4, 8, 16, 32}, Q((size_t) n);
		hu_design_var v[1] = {{0, 0, c.data(), nullptr}};
		hu_design_term t[1] = {{0, -1}};
		int64_t q, ts[2], df[1], dropped[1];
		if(hu_design_build(n, 1, v, 1, t, nullptr, Q.data(), &q, ts, df, dropped) != HU_OK) FAIL("a covariate was refused");
		const std::vector<int32_t> single = {0, 1, 2, 3, 4, 5}, hole = {0, 2, 0, 2, 0, 2}, neg = {0, -1, 0, 1, 0, 1};
		if(plan_refused("n = 2", 2, d, Q, 1, {0, 1}, nullptr, 9, 0)) return 1;
		if(plan_refused("q = 0", n, d, Q, 0, {0, 0}, nullptr, 9, 0)) return 1;
		if(plan_refused("term_start beyond q", n, d, Q, 1, {0, 2}, nullptr, 9, 0)) return 1;
		if(plan_refused("term_start from 1", n, d, Q, 1, {1, 1}, nullptr, 9, 0)) return 1;
		if(plan_refused("no permutation", n, d, Q, 1, {0, 1}, nullptr, 0, 0)) return 1;
		if(plan_refused("too many permutations", n, d, Q, 1, {0, 1}, nullptr, 10000001, 0)) return 1;
		if(plan_refused("a negative chunk", n, d, Q, 1, {0, 1}, nullptr, 9, -1)) return 1;
		if(plan_refused("single strata", n, d, Q, 1, {0, 1}, single.data(), 9, 0)) return 1;
		if(plan_refused("strata with a hole", n, d, Q, 1, {0, 1}, hole.data(), 9, 0)) return 1;
		if(plan_refused("a negative stratum", n, d, Q, 1, {0, 1}, neg.data(), 9, 0)) return 1;
		std::vector<double> bad = Q; bad[3] = INFINITY;
		if(plan_refused("an infinite basis", n, d, bad, 1, {0, 1}, nullptr, 9, 0)) return 1;
		std::vector<double> x = d; x[1] = x[6] = -1;
		if(plan_refused("a negative cell", n, x, Q, 1, {0, 1}, nullptr, 9, 0)) return 1;
		if(hu_permanova_design_need(0, 1, 1, 1, 0) != -1 || hu_permanova_design_need(6, 1, 1, 1, 1) - hu_permanova_design_need(6, 1, 1, 1, 0) != 2 * 6 * 64) FAIL("hu_permanova_design_need");
		++done;
	}
	{	/* the META reader */
		const std::vector<std::string> sample = {"a", "b", "c"};
		HuMeta m; HuMetaVar v; std::string err;
		if(!meta_of(argv[1], "\n#SampleID\tg\tx\tk\n# note\nb\tu\t2.5\t1\n\nzz\tu\t1\t1\na\tv\t-1e3\t2\nc\tu\t7\t1\r\n", sample, m, err)) FAIL("a good file was refused: %s", err.c_str());
		if(m.column.size() != 3 || m.ignored != 1 || m.value[0][1] != "-1e3") FAIL("the file read back differs");
		if(!hu_meta_variable(m, sample, "x", false, v, err) || !v.numeric || v.value[0] != -1000 || v.value[2] != 7) FAIL("a numeric column");
		if(!hu_meta_variable(m, sample, "k", true, v, err) || v.numeric || v.label != std::vector<int32_t>({0, 1, 1}) || v.level.size() != 2) FAIL("a forced factor");
		if(!hu_meta_variable(m, sample, "g", false, v, err) || v.numeric || v.label != std::vector<int32_t>({0, 1, 1})) FAIL("a categorical column");
		if(hu_meta_variable(m, sample, "none", false, v, err)) FAIL("a missing column was taken");
		static const char* const bad[] = {"", "onlyone\n", "s\tg\na\tu\nb\tu\n", "s\tg\na\tu\nb\tu\nc\tu\na\tv\n", "s\tg\na\tu\nb\tu\tmore\nc\tu\n", "s\tg\tg\na\tu\tu\nb\tu\tu\nc\tu\tu\n"};
		for(const char* text : bad) if(meta_of(argv[1], text, sample, m, err)) FAIL("a bad file was taken: '%s'", text);
		if(!meta_of(argv[1], "s\tg\na\tNA\nb\t\nc\tu\n", sample, m, err)) FAIL("NA is a matter of the used columns: %s", err.c_str());
		if(hu_meta_variable(m, sample, "g", false, v, err) || err.find("'a'") == std::string::npos) FAIL("NA was taken");
		if(hu_meta_read(std::string(argv[1]) + ".none", sample, m, err)) FAIL("a missing file was read");
		remove(argv[1]);
		++done;
	}
	printf("%d cases\n", done);
	return 0;
}
