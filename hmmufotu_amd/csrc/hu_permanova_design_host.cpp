// hu_permanova_design without a device: the design builder, the checks and the plan of a call, the index arrays of the
// permutations and the host path.  No HIP headers: a plain C++ compiler builds this file (tests/san/permanova_design_driver.cpp).  The
// host path restates the definition of include/hmmufotu_amd.h in straight loops; it is held to the error bound of §33, not to the
// device's bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "hu_permanova_design.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

/* ---- compensated sums: the result is the exact sum rounded once, up to terms of the order 2^-106 (Ogita, Rump and Oishi 2005) ---- */

static inline void pmd_two_sum(double a, double b, double& s, double& e) { s = a + b; const double z = s - a; e = (a - (s - z)) + (b - z); }
static double pmd_sum2(const double* x, int64_t n) {
	double s = 0.0, c = 0.0;
	for(int64_t i = 0; i < n; ++i) { double e; pmd_two_sum(s, x[i], s, e); c += e; }
	return s + c;
}
static double pmd_dot2(const double* a, const double* b, int64_t n) {
	double s = 0.0, c = 0.0;
	for(int64_t i = 0; i < n; ++i) {
		const double p = a[i] * b[i], ep = std::fma(a[i], b[i], -p);
		double e;
		pmd_two_sum(s, p, s, e);
		c += e + ep;
	}
	return s + c;
}
static void pmd_centre(double* x, int64_t n) {
	const double mean = pmd_sum2(x, n) / (double) n;
	for(int64_t i = 0; i < n; ++i) x[i] -= mean;
}

/* ---- the design ---- */

struct PmdVar { bool numeric; int64_t cols; };

/* the variables and the terms of a design, checked; info [n_var] */
static int pmd_design_check(const char* fn, int64_t n, int64_t n_var, const hu_design_var* var, int64_t T, const hu_design_term* term, std::vector<PmdVar>& info) {
	if(n < 1 || n_var < 1 || !var || T < 1 || !term) { hu_set_error("%s: bad argument: a design needs samples, variables and one term at the least", fn); return HU_ERR_ARG; }
	info.resize((size_t) n_var);
	for(int64_t v = 0; v < n_var; ++v) {
		if(var[v].kind == 0) {
			if(!var[v].value) { hu_set_error("%s: variable %lld has no values", fn, (long long) v); return HU_ERR_ARG; }
			for(int64_t i = 0; i < n; ++i) if(!std::isfinite(var[v].value[i])) { hu_set_error("%s: variable %lld is not finite at sample %lld", fn, (long long) v, (long long) i); return HU_ERR_ARG; }
			info[(size_t) v] = {true, 1};
		} else if(var[v].kind == 1) {
			if(!var[v].label) { hu_set_error("%s: variable %lld has no labels", fn, (long long) v); return HU_ERR_ARG; }
			int64_t top = -1;
			for(int64_t i = 0; i < n; ++i) {
				if(var[v].label[i] < 0) { hu_set_error("%s: variable %lld has the negative label %d at sample %lld", fn, (long long) v, var[v].label[i], (long long) i); return HU_ERR_ARG; }
				top = std::max<int64_t>(top, var[v].label[i]);
			}
			if(top >= n) { hu_set_error("%s: the labels of variable %lld are not dense in 0 .. L-1: label %lld among %lld samples", fn, (long long) v, (long long) top, (long long) n); return HU_ERR_ARG; }
			std::vector<char> used((size_t)(top + 1), 0);
			for(int64_t i = 0; i < n; ++i) used[(size_t) var[v].label[i]] = 1;
			for(int64_t l = 0; l <= top; ++l) if(!used[(size_t) l]) {
				hu_set_error("%s: the labels of variable %lld are not dense in 0 .. L-1: label %lld is used, label %lld is not", fn, (long long) v, (long long) top, (long long) l); return HU_ERR_ARG; }
			info[(size_t) v] = {false, top};
		} else { hu_set_error("%s: variable %lld is of kind %d: 0 (numeric) or 1 (categorical)", fn, (long long) v, var[v].kind); return HU_ERR_ARG; }
	}
	for(int64_t t = 0; t < T; ++t) if(term[t].a < 0 || term[t].a >= n_var || term[t].b >= n_var) {
		hu_set_error("%s: term %lld names a variable outside 0 .. %lld", fn, (long long) t, (long long)(n_var - 1)); return HU_ERR_ARG; }
	return HU_OK;
}

static int64_t pmd_term_cols(const std::vector<PmdVar>& info, const hu_design_term& t) { return info[(size_t) t.a].cols * (t.b < 0 ? 1 : info[(size_t) t.b].cols); }
/* raw column k of a variable at sample i */
static inline double pmd_raw(const hu_design_var& v, int64_t k, int64_t i) { return v.kind == 0 ? v.value[i] : (v.label[i] == k + 1 ? 1.0 : 0.0); }

extern "C" int64_t hu_design_raw_columns(int64_t n, int64_t n_var, const hu_design_var* var, int64_t T, const hu_design_term* term) try {
	std::vector<PmdVar> info;
	if(pmd_design_check("hu_design_raw_columns", n, n_var, var, T, term, info) != HU_OK) return -1;
	int64_t cols = 0;
	for(int64_t t = 0; t < T; ++t) cols += pmd_term_cols(info, term[t]);
	return cols;
} catch(...) { hu_catch_all("hu_design_raw_columns"); return -1; }

extern "C" int hu_design_build(int64_t n, int64_t n_var, const hu_design_var* var, int64_t T, const hu_design_term* term, const char* const* term_name,
		double* Q, int64_t* q_out, int64_t* term_start, int64_t* df, int64_t* dropped) try {
	const char* fn = "hu_design_build";
	std::vector<PmdVar> info;
	{ const int rc = pmd_design_check(fn, n, n_var, var, T, term, info); if(rc != HU_OK) return rc; }
	if(!Q || !q_out || !term_start || !df || !dropped) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	if(n < 3) { hu_set_error("%s: %lld samples: a test needs 3 at the least", fn, (long long) n); return HU_ERR_ARG; }
	std::vector<std::vector<double>> kept;
	std::vector<double> x((size_t) n);
	auto name = [&](int64_t t) { return term_name && term_name[t] ? std::string("'") + term_name[t] + "'" : "number " + std::to_string(t + 1); };
	term_start[0] = 0;
	for(int64_t t = 0; t < T; ++t) {
		const hu_design_var &A = var[term[t].a];
		const hu_design_var* B = term[t].b < 0 ? nullptr : &var[term[t].b];
		const bool numeric = A.kind == 0 || (B && B->kind == 0);
		const int64_t ca = info[(size_t) term[t].a].cols, cb = B ? info[(size_t) term[t].b].cols : 1;
		df[t] = 0; dropped[t] = 0;
		for(int64_t ka = 0; ka < ca; ++ka) for(int64_t kb = 0; kb < cb; ++kb) {
			for(int64_t i = 0; i < n; ++i) x[(size_t) i] = B ? pmd_raw(A, ka, i) * pmd_raw(*B, kb, i) : pmd_raw(A, ka, i);
			pmd_centre(x.data(), n);
			double before = std::sqrt(pmd_dot2(x.data(), x.data(), n));
			if(!std::isfinite(before)) { hu_set_error("%s: term %s: a column's norm is not finite", fn, name(t).c_str()); return HU_ERR_ARG; }
			if(numeric && before > 0) {
				for(int64_t i = 0; i < n; ++i) x[(size_t) i] /= before;
				before = std::sqrt(pmd_dot2(x.data(), x.data(), n));
			}
			double after = 0.0;
			if(before > 0) {
				for(int pass = 0; pass < 2; ++pass) for(const auto& k : kept) {
					const double c = pmd_dot2(k.data(), x.data(), n);
					for(int64_t i = 0; i < n; ++i) x[(size_t) i] = std::fma(-c, k[(size_t) i], x[(size_t) i]);
				}
				pmd_centre(x.data(), n);
				after = std::sqrt(pmd_dot2(x.data(), x.data(), n));
			}
			if(!(after >= HU_PMD_DROP * before) || !(after > 0)) { ++dropped[t]; continue; }
			for(int64_t i = 0; i < n; ++i) x[(size_t) i] /= after;
			kept.push_back(x);
			++df[t];
		}
		if(df[t] == 0) { hu_set_error("%s: term %s adds nothing to the terms before it: every column of it lies in their span", fn, name(t).c_str()); return HU_ERR_ARG; }
		term_start[t + 1] = (int64_t) kept.size();
	}
	const int64_t q = (int64_t) kept.size();
	if(n - 1 - q < 1) { hu_set_error("%s: %lld samples and %lld design columns leave %lld residual degrees of freedom: 1 at the least", fn, (long long) n, (long long) q, (long long)(n - 1 - q)); return HU_ERR_ARG; }
	for(int64_t i = 0; i < n; ++i) for(int64_t c = 0; c < q; ++c) Q[i * q + c] = kept[(size_t) c][(size_t) i];
	*q_out = q;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_design_build"); }

/* ---- the call ---- */

extern "C" void hu_permanova_design_default_opts(hu_permanova_design_opts* o) {
	if(!o) return;
	o->perms = 999; o->seed = 1; o->host = 0; o->index32 = 0; o->chunk = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_permanova_design_need(int64_t n, int64_t q, int64_t T, int64_t chunk, int32_t index32) {
	if(n < 1 || q < 1 || T < 1 || T > q || chunk < 1 || n > 0x7fffffffll || q > n || chunk > HU_PM_MAX_PERMS) return -1;
	const int64_t c = hu_pmd_pad(chunk), w = hu_pmd_vcpad(chunk, q), e = (index32 || n > 65536) ? 4 : 2;
	return 8 * n * n + e * n * c + 8 * n * q + 8 * hu_pmd_row_blocks(n) * hu_pc_slabs(n) * w + 8 * w + 8 * c * T + 4 * (2 * n + 1) + (1 << 20);
}

/* member [n] sorted by (stratum, index) and start [S + 1] of the labels strata [n] (NULL: one stratum) */
static int pmd_strata(const char* fn, int64_t n, const int32_t* strata, std::vector<int32_t>& member, std::vector<int32_t>& start) {
	member.resize((size_t) n);
	if(!strata) {
		for(int64_t i = 0; i < n; ++i) member[(size_t) i] = (int32_t) i;
		start = {0, (int32_t) n};
		return HU_OK;
	}
	int64_t top = -1;
	for(int64_t i = 0; i < n; ++i) {
		if(strata[i] < 0) { hu_set_error("%s: sample %lld has the negative stratum label %d", fn, (long long) i, strata[i]); return HU_ERR_ARG; }
		top = std::max<int64_t>(top, strata[i]);
	}
	if(top >= n) { hu_set_error("%s: the stratum labels are not dense in 0 .. S-1: label %lld among %lld samples", fn, (long long) top, (long long) n); return HU_ERR_ARG; }
	start.assign((size_t)(top + 2), 0);
	for(int64_t i = 0; i < n; ++i) ++start[(size_t) strata[i] + 1];
	for(int64_t s = 0; s <= top; ++s) {
		if(start[(size_t) s + 1] == 0) { hu_set_error("%s: the stratum labels are not dense in 0 .. S-1: label %lld is used, label %lld is not", fn, (long long) top, (long long) s); return HU_ERR_ARG; }
		start[(size_t) s + 1] += start[(size_t) s];
	}
	std::vector<int32_t> at(start.begin(), start.end() - 1);
	for(int64_t i = 0; i < n; ++i) member[(size_t) at[(size_t) strata[i]]++] = (int32_t) i;
	return HU_OK;
}

int hu_pmd_plan(const char* fn, int64_t n, const double* dist, const double* Q, int64_t q, int64_t T, const int64_t* term_start, const int32_t* strata,
		const hu_permanova_design_opts* opts, HuPmdPlan& pl) {
	hu_permanova_design_opts o;
	if(opts) o = *opts; else hu_permanova_design_default_opts(&o);
	if(!dist || !Q || !term_start) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(n < 3) { hu_set_error("%s: %lld samples: a test needs 3 at the least", fn, (long long) n); return HU_ERR_ARG; }
	if(n > 65535ll * HU_PCOA_TILE) { hu_set_error("%s: %lld samples: more row blocks than a grid holds", fn, (long long) n); return HU_ERR_ARG; }
	if(q < 1) { hu_set_error("%s: %lld design columns: 1 at the least", fn, (long long) q); return HU_ERR_ARG; }
	if(n - 1 - q < 1) { hu_set_error("%s: %lld samples and %lld design columns leave %lld residual degrees of freedom: 1 at the least", fn, (long long) n, (long long) q, (long long)(n - 1 - q)); return HU_ERR_ARG; }
	if(T < 1 || T > q || term_start[0] != 0 || term_start[T] != q) { hu_set_error("%s: term_start does not ascend from 0 to q = %lld over %lld terms", fn, (long long) q, (long long) T); return HU_ERR_ARG; }
	for(int64_t t = 0; t < T; ++t) if(term_start[t + 1] <= term_start[t]) { hu_set_error("%s: term_start does not ascend at term %lld", fn, (long long) t); return HU_ERR_ARG; }
	if(o.perms < 1 || o.perms > HU_PM_MAX_PERMS) { hu_set_error("%s: %lld permutations: between 1 and %d", fn, (long long) o.perms, HU_PM_MAX_PERMS); return HU_ERR_ARG; }
	if(o.chunk < 0) { hu_set_error("%s: chunk %lld below 0", fn, (long long) o.chunk); return HU_ERR_ARG; }
	for(int64_t i = 0; i < n * q; ++i) if(!std::isfinite(Q[i])) { hu_set_error("%s: the design basis is not finite at sample %lld, column %lld", fn, (long long)(i / q), (long long)(i % q)); return HU_ERR_ARG; }
	{ const int rc = pmd_strata(fn, n, strata, pl.member, pl.start); if(rc != HU_OK) return rc; }
	pl.S = (int64_t) pl.start.size() - 1;
	if(pl.S == n) { hu_set_error("%s: every stratum is a single sample: no permutation exists", fn); return HU_ERR_ARG; }
	{ const int rc = hu_pm_check_matrix(fn, n, dist); if(rc != HU_OK) return rc; }
	pl.n = n; pl.q = q; pl.T = T; pl.perms = o.perms; pl.chunk = o.chunk; pl.budget = o.mem_budget > 0 ? o.mem_budget : 0; pl.seed = o.seed;
	pl.host = o.host != 0; pl.index32 = o.index32 != 0 || n > 65536;
	pl.term_start.assign(term_start, term_start + T + 1);
	return HU_OK;
}

extern "C" int hu_permanova_perms(int64_t n, const int32_t* strata, uint64_t seed, int64_t first, int64_t count, int64_t* out) try {
	const char* fn = "hu_permanova_perms";
	if(n < 1 || n > 0x7fffffffll || first < 0 || count < 0 || (count > 0 && !out)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	std::vector<int32_t> member, start;
	{ const int rc = pmd_strata(fn, n, strata, member, start); if(rc != HU_OK) return rc; }
	for(int64_t k = 0; k < count; ++k) {
		int64_t* idx = out + k * n;
		for(int64_t i = 0; i < n; ++i) idx[i] = i;
		hu_pmd_shuffle(seed, (uint64_t)(first + k), (int64_t) start.size() - 1, member.data(), start.data(), idx);
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_permanova_perms"); }

void hu_pmd_host_run(const HuPmdPlan& pl, const double* dist, const double* Q, double* ss) {
	const int64_t n = pl.n, q = pl.q;
	std::vector<double> D2((size_t)(n * n)), v((size_t) n);
	for(int64_t i = 0; i < n * n; ++i) D2[(size_t) i] = dist[i] * dist[i];
	std::vector<int64_t> idx((size_t) n);
	for(int64_t r = 0; r <= pl.perms; ++r) {                              /* row 0: the identity */
		for(int64_t i = 0; i < n; ++i) idx[(size_t) i] = i;
		if(r > 0) hu_pmd_shuffle(pl.seed, (uint64_t)(r - 1), pl.S, pl.member.data(), pl.start.data(), idx.data());
		for(int64_t t = 0; t < pl.T; ++t) {
			double sum = 0.0;
			for(int64_t c = pl.term_start[(size_t) t]; c < pl.term_start[(size_t) t + 1]; ++c) {
				for(int64_t i = 0; i < n; ++i) v[(size_t) i] = Q[idx[(size_t) i] * q + c];
				double s = 0.0;
				for(int64_t i = 0; i < n; ++i) {
					const double* row = D2.data() + i * n;
					double w = 0.0;
					for(int64_t j = 0; j < n; ++j) w = std::fma(row[j], v[(size_t) j], w);
					s = std::fma(v[(size_t) i], w, s);
				}
				sum += s;
			}
			ss[r * pl.T + t] = -0.5 * sum;
		}
	}
}

void hu_pmd_result(const HuPmdPlan& pl, double ssT, const double* ss, hu_permanova_design_term* out) {
	const int64_t T = pl.T, dfRes = pl.n - 1 - pl.q;
	std::vector<double> F((size_t) T), bar((size_t) T);
	auto stat = [&](const double* row, double* f) {
		double sum = 0.0;
		for(int64_t t = 0; t < T; ++t) sum += row[t];
		const double res = ssT - sum;
		for(int64_t t = 0; t < T; ++t) f[t] = (row[t] / (double)(pl.term_start[(size_t) t + 1] - pl.term_start[(size_t) t])) / (res / (double) dfRes);
		return res;
	};
	const double res = stat(ss, F.data());
	for(int64_t t = 0; t < T; ++t) {
		hu_permanova_design_term& o = out[t];
		o.df = pl.term_start[(size_t) t + 1] - pl.term_start[(size_t) t]; o.df_res = dfRes;
		o.ss = ss[t]; o.ss_res = res; o.ss_total = ssT; o.R2 = ss[t] / ssT; o.F = F[(size_t) t];
		o.count_ge = 0; o.count_nan = 0;
		bar[(size_t) t] = std::isinf(o.F) ? o.F : o.F - 0x1p-26 * std::fabs(o.F);
	}
	std::vector<double> f((size_t) T);
	for(int64_t p = 0; p < pl.perms; ++p) {
		stat(ss + (p + 1) * T, f.data());
		for(int64_t t = 0; t < T; ++t) {
			if(std::isnan(f[(size_t) t])) ++out[t].count_nan;
			else if(f[(size_t) t] >= bar[(size_t) t]) ++out[t].count_ge;
		}
	}
	for(int64_t t = 0; t < T; ++t) out[t].p = std::isnan(out[t].F) ? NAN : (double)(1 + out[t].count_ge) / (double)(pl.perms + 1);
}
