// hu_permanova without a device: the checks, the plan of a call, the host path and the reader of a distance matrix.
// No HIP headers: a plain C++ compiler builds this file (tests/san/permanova_driver.cpp).  The host path restates the definition of
// include/hmmufotu_amd.h in plain loops with the summation order of the kernels (hu_kern_permanova.h): tiles of 64 x 64 in ascending
// row-major order, in a tile the matching squares of a row by plain adds, the rows by fma with 1 / n_g, the tiles by plain adds.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "hu_permanova.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_permanova_default_opts(hu_permanova_opts* o) {
	if(!o) return;
	o->perms = 999; o->seed = 1; o->host = 0; o->reserved = 0; o->chunk = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_permanova_need(int64_t n, int64_t a, int64_t chunk) {
	if(n < 1 || a < 1 || chunk < 1 || n > 0x7fffffffll || chunk > HU_PM_MAX_PERMS) return -1;
	const int64_t c = hu_pm_pad(chunk), t = hu_pm_tiles(n);
	return 8 * n * n + 2 * n * c + 8 * t * c + 8 * c + 8 * a + 2 * n + (1 << 20);
}

int hu_pm_check_matrix(const char* fn, int64_t n, const double* dist) {
	bool any = false;
	/* the cells with j >= i, in blocks of 64 x 64 so that the mirrored cell is in the cache; a mirrored cell is held to its twin alone */
	for(int64_t ib = 0; ib < n; ib += HU_PM_TILE) for(int64_t jb = ib; jb < n; jb += HU_PM_TILE)
	for(int64_t i = ib; i < std::min(n, ib + HU_PM_TILE); ++i) for(int64_t j = std::max(jb, i); j < std::min(n, jb + HU_PM_TILE); ++j) {
		const double v = dist[i * n + j], w = dist[j * n + i];
		if(!(v >= 0) || !std::isfinite(v)) { hu_set_error("%s: the distance of samples %lld and %lld is negative or not finite", fn, (long long) i, (long long) j); return HU_ERR_ARG; }
		if(v > 0x1p511) { hu_set_error("%s: the distance of samples %lld and %lld is %g: its square is not finite", fn, (long long) i, (long long) j, v); return HU_ERR_ARG; }
		if(i == j && v != 0) { hu_set_error("%s: sample %lld is at the distance %g from itself", fn, (long long) i, v); return HU_ERR_ARG; }
		if(!(w == v)) { hu_set_error("%s: the matrix is not symmetric: d(%lld, %lld) = %.17g, d(%lld, %lld) = %.17g", fn,
			(long long) i, (long long) j, v, (long long) j, (long long) i, w); return HU_ERR_ARG; }
		any = any || v > 0;
	}
	if(!any) { hu_set_error("%s: every distance is 0: nothing to partition", fn); return HU_ERR_ARG; }
	return HU_OK;
}

int hu_pm_plan(const char* fn, int64_t n, const double* dist, const int32_t* group, const hu_permanova_opts* opts, HuPmPlan& pl) {
	hu_permanova_opts o;
	if(opts) o = *opts; else hu_permanova_default_opts(&o);
	if(!dist || !group) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(n < 3) { hu_set_error("%s: %lld samples: a test needs 3 at the least", fn, (long long) n); return HU_ERR_ARG; }
	if(hu_pm_tiles(n) > 0x7fffffffll) { hu_set_error("%s: %lld samples: more tiles than a grid holds", fn, (long long) n); return HU_ERR_ARG; }
	if(o.perms < 1 || o.perms > HU_PM_MAX_PERMS) { hu_set_error("%s: %lld permutations: between 1 and %d", fn, (long long) o.perms, HU_PM_MAX_PERMS); return HU_ERR_ARG; }
	if(o.chunk < 0) { hu_set_error("%s: chunk %lld below 0", fn, (long long) o.chunk); return HU_ERR_ARG; }
	std::vector<int64_t> size;
	{ const int rc = hu_groups_check(fn, n, group, HU_PM_MAX_GROUPS, "nothing varies within", size); if(rc != HU_OK) return rc; }
	const int64_t a = (int64_t) size.size();
	{ const int rc = hu_pm_check_matrix(fn, n, dist); if(rc != HU_OK) return rc; }
	pl.n = n; pl.a = a; pl.perms = o.perms; pl.chunk = o.chunk; pl.budget = o.mem_budget > 0 ? o.mem_budget : 0; pl.seed = o.seed; pl.host = o.host != 0;
	pl.inv.resize((size_t) a); pl.lab.resize((size_t) n);
	for(int64_t g = 0; g < a; ++g) pl.inv[(size_t) g] = 1.0 / (double) size[(size_t) g];
	for(int64_t i = 0; i < n; ++i) pl.lab[(size_t) i] = (uint16_t) group[i];
	return HU_OK;
}

double hu_pm_ss_total(int64_t n, const double* dist) {
	const int64_t nt = (n + HU_PM_TILE - 1) / HU_PM_TILE;
	double tot = 0.0;
	for(int64_t I = 0; I < nt; ++I) for(int64_t J = I; J < nt; ++J) {
		double s = 0.0;
		const int64_t i1 = std::min<int64_t>(n, (I + 1) * HU_PM_TILE), j1 = std::min<int64_t>(n, (J + 1) * HU_PM_TILE);
		for(int64_t i = I * HU_PM_TILE; i < i1; ++i) {
			double r = 0.0;
			for(int64_t j = std::max<int64_t>(J * HU_PM_TILE, i + 1); j < j1; ++j) { const double d = dist[i * n + j]; r += d * d; }
			s += r;
		}
		tot += s;
	}
	return tot / (double) n;
}

double hu_pm_host_ssw(const HuPmPlan& pl, const double* D2, const uint16_t* g) {
	const int64_t n = pl.n, nt = (n + HU_PM_TILE - 1) / HU_PM_TILE;
	double tot = 0.0;
	for(int64_t I = 0; I < nt; ++I) for(int64_t J = I; J < nt; ++J) {
		double s = 0.0;
		const int64_t i1 = std::min<int64_t>(n, (I + 1) * HU_PM_TILE), j1 = std::min<int64_t>(n, (J + 1) * HU_PM_TILE);
		for(int64_t i = I * HU_PM_TILE; i < i1; ++i) {
			const uint16_t gi = g[i];
			const double* row = D2 + i * n;
			double r = 0.0;
			for(int64_t j = std::max<int64_t>(J * HU_PM_TILE, i + 1); j < j1; ++j) if(g[j] == gi) r += row[j];
			s = std::fma(pl.inv[gi], r, s);
		}
		tot += s;
	}
	return tot;
}

void hu_pm_host_shuffle(const HuPmPlan& pl, uint64_t p, uint16_t* g) {
	std::copy(pl.lab.begin(), pl.lab.end(), g);
	hu_pm_shuffle(pl.seed, p, pl.n, g);
}

void hu_pm_host_run(const HuPmPlan& pl, const double* dist, double* obs, double* ssw) {
	const size_t n = (size_t) pl.n;
	std::vector<double> D2(n * n, 0.0);
	for(size_t i = 0; i < n; ++i) for(size_t j = i + 1; j < n; ++j) { const double d = dist[i * n + j]; D2[i * n + j] = d * d; }
	*obs = hu_pm_host_ssw(pl, D2.data(), pl.lab.data());
	std::vector<uint16_t> g(n);
	for(int64_t p = 0; p < pl.perms; ++p) {
		hu_pm_host_shuffle(pl, (uint64_t) p, g.data());
		ssw[p] = hu_pm_host_ssw(pl, D2.data(), g.data());
	}
}

void hu_pm_result(const HuPmPlan& pl, double ssT, double obs, const double* ssw, hu_permanova_result* out) {
	int64_t le = 0;
	for(int64_t p = 0; p < pl.perms; ++p) le += ssw[p] <= obs ? 1 : 0;
	out->n = pl.n; out->a = pl.a; out->perms = pl.perms;
	out->ss_total = ssT; out->ss_within = obs; out->ss_among = ssT - obs;
	out->F = (out->ss_among / (double)(pl.a - 1)) / (obs / (double)(pl.n - pl.a));
	out->R2 = out->ss_among / ssT;
	out->count_le = le;
	out->p = (double)(1 + le) / (double)(pl.perms + 1);
}

extern "C" int hu_permanova_labels(int64_t n, const int32_t* group, uint64_t seed, int64_t first, int64_t count, int32_t* out) try {
	if(n < 1 || !group || first < 0 || count < 0 || (count > 0 && !out)) { hu_set_error("hu_permanova_labels: bad argument"); return HU_ERR_ARG; }
	for(int64_t k = 0; k < count; ++k) {
		int32_t* g = out + k * n;
		std::copy(group, group + n, g);
		hu_pm_shuffle(seed, (uint64_t)(first + k), n, g);
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_permanova_labels"); }

/* ---- the distance matrix of hmmufotu-amd-unifrac -o ---- */

struct hu_dist_matrix {
	std::vector<std::string> names;
	std::vector<double> d;
};

static void pm_split(const std::string& line, std::vector<std::string>& f) {
	f.clear();
	size_t b = 0;
	for(;;) {
		const size_t e = line.find('\t', b);
		f.push_back(line.substr(b, e == std::string::npos ? e : e - b));
		if(e == std::string::npos) break;
		b = e + 1;
	}
}

extern "C" int hu_dist_matrix_read(const char* path, hu_dist_matrix** out) try {
	if(!path || !out) { hu_set_error("hu_dist_matrix_read: null argument"); return HU_ERR_ARG; }
	*out = nullptr;
	std::ifstream in(path);
	if(!in) { hu_set_error("Unable to open distance matrix '%s'", path); return HU_ERR_IO; }
	std::string line;
	std::vector<std::string> f;
	if(!std::getline(in, line)) { hu_set_error("%s: empty file", path); return HU_ERR_IO; }
	if(!line.empty() && line.back() == '\r') line.pop_back();
	pm_split(line, f);
	if(f.size() < 2 || !f[0].empty()) { hu_set_error("%s: line 1: the names of the samples, each after a tab", path); return HU_ERR_IO; }
	hu_dist_matrix* m = new hu_dist_matrix;
	struct Guard { hu_dist_matrix* m; ~Guard() { delete m; } } guard{m};
	m->names.assign(f.begin() + 1, f.end());
	const size_t n = m->names.size();
	for(size_t j = 0; j < n; ++j) {
		if(m->names[j].empty()) { hu_set_error("%s: line 1: sample %zu has no name", path, j + 1); return HU_ERR_IO; }
		for(size_t k = 0; k < j; ++k) if(m->names[k] == m->names[j]) { hu_set_error("%s: line 1: sample '%s' is named twice", path, m->names[j].c_str()); return HU_ERR_IO; }
	}
	m->d.resize(n * n);
	size_t row = 0; long long ln = 1;
	while(std::getline(in, line)) {
		++ln;
		if(!line.empty() && line.back() == '\r') line.pop_back();
		if(line.empty()) continue;
		if(row >= n) { hu_set_error("%s: line %lld: more than %zu rows", path, ln, n); return HU_ERR_IO; }
		pm_split(line, f);
		if(f[0] != m->names[row]) { hu_set_error("%s: line %lld: row '%s' where the header has '%s'", path, ln, f[0].c_str(), m->names[row].c_str()); return HU_ERR_IO; }
		if(f.size() != n + 1) { hu_set_error("%s: line %lld: sample '%s' has %zu of %zu numbers", path, ln, f[0].c_str(), f.size() - 1, n); return HU_ERR_IO; }
		for(size_t j = 0; j < n; ++j) {
			const char* s = f[j + 1].c_str();
			char* end = nullptr;
			const double v = strtod(s, &end);
			if(end == s || *end) { hu_set_error("%s: line %lld: '%s' is not a number", path, ln, s); return HU_ERR_IO; }
			m->d[row * n + j] = v;
		}
		++row;
	}
	if(in.bad()) { hu_set_error("%s: read error", path); return HU_ERR_IO; }
	if(row != n) { hu_set_error("%s: %zu rows for %zu samples", path, row, n); return HU_ERR_IO; }
	guard.m = nullptr;
	*out = m;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dist_matrix_read"); }

extern "C" void hu_dist_matrix_free(hu_dist_matrix* m) { delete m; }
extern "C" int hu_dist_matrix_dims(const hu_dist_matrix* m, int64_t* n) {
	if(!m) return HU_ERR_ARG;
	if(n) *n = (int64_t) m->names.size();
	return HU_OK;
}
extern "C" const char* hu_dist_matrix_sample(const hu_dist_matrix* m, int64_t i) {
	return m && i >= 0 && (size_t) i < m->names.size() ? m->names[(size_t) i].c_str() : "";
}
extern "C" const double* hu_dist_matrix_values(const hu_dist_matrix* m) { return m ? m->d.data() : nullptr; }
