// hu_diffabund without a device: the checks, the column totals, the ranking, the tie sums, L, the cells of the tested
// OTUs, the whole host path on one thread, and maxT and BH from what either path computed.  No HIP headers: a plain C++ compiler builds
// this file (tests/san/diffabund_driver.cpp).  Ranks are made once, here, for both paths; T and H are the functions of hu_diffabund.h
// that the kernels compile too.
#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <utility>
#include <vector>
#include "hu_diffabund.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_diffabund_default_opts(hu_diffabund_opts* o) {
	if(!o) return;
	o->perms = 999; o->seed = 1; o->host = 0; o->rank_by = 0; o->min_prevalence = 1; o->chunk = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_diffabund_need(int64_t n, int64_t a, int64_t n_otu, int64_t n_cell, int64_t chunk) {
	if(n < 1 || n > HU_DA_MAX_SAMPLES || a < 1 || a > HU_DA_MAX_GROUPS || n_otu < 1 || n_cell < 0 || chunk < 1 || chunk > HU_DA_MAX_PERMS) return -1;
	if(n_otu > (int64_t) 1 << 40 || n_cell > (int64_t) 1 << 50) return -1;
	const int64_t c = hu_da_pad(chunk), b = hu_da_blocks(n_otu);
	return 4 * n_cell + n * c + 8 * b * c + 8 * c + n + 16 * a + 52 * n_otu + 8 + (1 << 20);
}

/* total_j: the column sums, added in ascending OTU order */
static void da_totals(int64_t M, int64_t N, const double* counts, std::vector<double>& tot) {
	tot.assign((size_t) N, 0.0);
	for(int64_t i = 0; i < M; ++i) { const double* row = counts + i * N; for(int64_t j = 0; j < N; ++j) tot[(size_t) j] += row[j]; }
}

/* the cells of a row above 0 as (x, sample), sorted by x; returns the number of nonzero counts (the prevalence) */
static int64_t da_row_values(int64_t N, const double* row, const double* tot, std::vector<std::pair<double, int32_t>>& v) {
	v.clear();
	int64_t prev = 0;
	for(int64_t j = 0; j < N; ++j) if(row[j] != 0) {
		++prev;
		const double x = tot ? row[j] / tot[j] : row[j];
		if(x > 0) v.emplace_back(x, (int32_t) j);
	}
	std::sort(v.begin(), v.end());
	return prev;
}

/* r2 of the sorted cells above 0 among N cells, the others being 0: into r2 [v.size()]; returns sum_ties (t^3 - t), the zeros included */
static int64_t da_rank_sorted(int64_t N, const std::vector<std::pair<double, int32_t>>& v, std::vector<int32_t>& r2) {
	const int64_t k = (int64_t) v.size(), z = N - k;
	r2.resize((size_t) k);
	int64_t ties = z * z * z - z;
	for(int64_t b = 0; b < k;) {
		int64_t e = b + 1;
		while(e < k && v[(size_t) e].first == v[(size_t) b].first) ++e;
		const int64_t t = e - b;
		for(int64_t i = b; i < e; ++i) r2[(size_t) i] = (int32_t)(2 * (z + b) + t + 1);
		ties += t * t * t - t;
		b = e;
	}
	return ties;
}

static int da_check_cells(const char* fn, int64_t M, int64_t N, const double* counts) {
	for(int64_t i = 0; i < M; ++i) for(int64_t j = 0; j < N; ++j) {
		const double v = counts[i * N + j];
		if(!(v >= 0) || !std::isfinite(v)) { hu_set_error("%s: the cell of OTU %lld and sample %lld is negative or not finite", fn, (long long) i, (long long) j); return HU_ERR_ARG; }
	}
	return HU_OK;
}

int hu_da_plan(const char* fn, int64_t M, int64_t N, const double* counts, const int32_t* group, const hu_diffabund_opts* opts, HuDaPlan& pl) {
	hu_diffabund_opts o;
	if(opts) o = *opts; else hu_diffabund_default_opts(&o);
	if(!counts || !group) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(M < 1) { hu_set_error("%s: %lld OTUs: a table needs 1 at the least", fn, (long long) M); return HU_ERR_ARG; }
	if(N < 3) { hu_set_error("%s: %lld samples: a test needs 3 at the least", fn, (long long) N); return HU_ERR_ARG; }
	if(N > HU_DA_MAX_SAMPLES) { hu_set_error("%s: %lld samples: %d at the most", fn, (long long) N, HU_DA_MAX_SAMPLES); return HU_ERR_ARG; }
	if(o.perms < 1 || o.perms > HU_DA_MAX_PERMS) { hu_set_error("%s: %lld permutations: between 1 and %d", fn, (long long) o.perms, HU_DA_MAX_PERMS); return HU_ERR_ARG; }
	if(o.chunk < 0) { hu_set_error("%s: chunk %lld below 0", fn, (long long) o.chunk); return HU_ERR_ARG; }
	if(o.min_prevalence < 0) { hu_set_error("%s: min_prevalence %lld below 0", fn, (long long) o.min_prevalence); return HU_ERR_ARG; }
	if(o.rank_by != 0 && o.rank_by != 1) { hu_set_error("%s: rank_by %d: 0 (fraction) or 1 (count)", fn, o.rank_by); return HU_ERR_ARG; }
	std::vector<int64_t> size;
	{ const int rc = hu_groups_check(fn, N, group, HU_DA_MAX_GROUPS, "no relabelling changes a sum", size); if(rc != HU_OK) return rc; }
	const int64_t a = (int64_t) size.size();
	unsigned __int128 L = 1;
	for(int64_t g = 0; g < a; ++g) {
		uint64_t x = (uint64_t) L, y = (uint64_t) size[(size_t) g];
		while(y) { const uint64_t t = x % y; x = y; y = t; }                     /* x = gcd(L, n_g) */
		L = L / x * (uint64_t) size[(size_t) g];
		if(L >> 64) {
			std::string s;
			for(int64_t h = 0; h < a; ++h) s += (h ? ", " : "") + std::to_string(size[(size_t) h]);
			hu_set_error("%s: the least common multiple of the group sizes (%s) is 2^64 or more: T does not fit 128 bits", fn, s.c_str());
			return HU_ERR_ARG;
		}
	}
	{ const int rc = da_check_cells(fn, M, N, counts); if(rc != HU_OK) return rc; }
	std::vector<double> tot;
	if(o.rank_by == 0) {
		da_totals(M, N, counts, tot);
		for(int64_t j = 0; j < N; ++j) {
			if(!(tot[(size_t) j] > 0)) { hu_set_error("%s: sample %lld has no reads: its fractions do not exist", fn, (long long) j); return HU_ERR_ARG; }
			if(!std::isfinite(tot[(size_t) j])) { hu_set_error("%s: the reads of sample %lld do not add to a finite number", fn, (long long) j); return HU_ERR_ARG; }
		}
	}
	pl.n = N; pl.a = a; pl.n_otu = M; pl.perms = o.perms; pl.chunk = o.chunk; pl.budget = o.mem_budget > 0 ? o.mem_budget : 0;
	pl.seed = o.seed; pl.host = o.host != 0;
	pl.L = (uint64_t) L; pl.dL = (double) pl.L; pl.c2 = 3.0 / ((double) N * (double)(N + 1));
	pl.size = size; pl.w.resize((size_t) a); pl.lab.resize((size_t) N);
	for(int64_t g = 0; g < a; ++g) pl.w[(size_t) g] = pl.L / (uint64_t) size[(size_t) g];
	for(int64_t i = 0; i < N; ++i) pl.lab[(size_t) i] = (uint8_t) group[i];
	pl.prevalence.assign((size_t) M, 0); pl.row.clear(); pl.ptr.assign(1, 0); pl.cell.clear(); pl.ez.clear(); pl.dsum.clear(); pl.tc.clear();
	const double den = (double)(N * N * N - N);
	std::vector<std::pair<double, int32_t>> v; std::vector<int32_t> r2;
	for(int64_t i = 0; i < M; ++i) {
		const int64_t prev = da_row_values(N, counts + i * N, o.rank_by == 0 ? tot.data() : nullptr, v);
		pl.prevalence[(size_t) i] = prev;
		const int64_t ties = da_rank_sorted(N, v, r2);
		const double tc = 1.0 - (double) ties / den;
		if(tc == 0 || prev < o.min_prevalence) continue;
		const int64_t k = (int64_t) v.size(), ez = -k;                            /* r2_z = z + 1, so e_z = z - N */
		int64_t dsum = 0;
		for(int64_t c = 0; c < k; ++c) {
			const int64_t d = (int64_t) r2[(size_t) c] - (N + 1) - ez;              /* z + t <= d <= 2 N */
			dsum += d;
			pl.cell.push_back((uint32_t) v[(size_t) c].second << 16 | (uint32_t) d);
		}
		pl.row.push_back(i); pl.ptr.push_back((int64_t) pl.cell.size()); pl.ez.push_back((int32_t) ez); pl.dsum.push_back((int32_t) dsum); pl.tc.push_back(tc);
	}
	if(pl.row.empty()) { hu_set_error("%s: no OTU is left to test: the cells of every OTU tie, or fewer than %lld are above 0", fn, (long long) o.min_prevalence); return HU_ERR_ARG; }
	return HU_OK;
}

void hu_da_host_shuffle(const HuDaPlan& pl, uint64_t p, uint8_t* g) {
	std::copy(pl.lab.begin(), pl.lab.end(), g);
	hu_pm_shuffle(pl.seed, p, pl.n, g);
}

void hu_da_host_T(const HuDaPlan& pl, int64_t r, const uint8_t* g, uint64_t* hi, uint64_t* lo, int64_t* C) {
	int64_t D[HU_DA_MAX_GROUPS];
	for(int64_t k = 0; k < pl.a; ++k) D[k] = 0;
	for(int64_t c = pl.ptr[(size_t) r]; c < pl.ptr[(size_t) r + 1]; ++c) { const uint32_t w = pl.cell[(size_t) c]; D[g[w >> 16]] += (int64_t)(w & 0xffff); }
	uint64_t h = 0, l = 0;
	for(int64_t k = 0; k < pl.a; ++k) {
		const int64_t c = pl.size[(size_t) k] * pl.ez[(size_t) r] + D[k];
		if(C) C[k] = c;
		hu_da_T_add(h, l, c, pl.w[(size_t) k]);
	}
	*hi = h; *lo = l;
}

void hu_da_host_run(const HuDaPlan& pl, uint64_t* tobs, double* hobs, int64_t* count, double* maxstat) {
	const int64_t m = (int64_t) pl.row.size();
	for(int64_t r = 0; r < m; ++r) {
		hu_da_host_T(pl, r, pl.lab.data(), &tobs[2 * r], &tobs[2 * r + 1], nullptr);
		hobs[r] = hu_da_H(tobs[2 * r], tobs[2 * r + 1], pl.dL, pl.c2, pl.tc[(size_t) r]);
		count[r] = 0;
	}
	std::vector<uint8_t> g((size_t) pl.n);
	for(int64_t p = 0; p < pl.perms; ++p) {
		hu_da_host_shuffle(pl, (uint64_t) p, g.data());
		double mx = 0.0;
		for(int64_t r = 0; r < m; ++r) {
			uint64_t hi, lo;
			hu_da_host_T(pl, r, g.data(), &hi, &lo, nullptr);
			if(hu_da_T_ge(hi, lo, tobs[2 * r], tobs[2 * r + 1])) ++count[r];
			const double H = hu_da_H(hi, lo, pl.dL, pl.c2, pl.tc[(size_t) r]);
			mx = H > mx ? H : mx;
		}
		maxstat[p] = mx;
	}
}

void hu_da_result(const HuDaPlan& pl, const uint64_t* tobs, const double* hobs, const int64_t* count, const double* maxstat, hu_diffabund_rec* rec) {
	const double nan = std::numeric_limits<double>::quiet_NaN();
	const int64_t m = (int64_t) pl.row.size();
	for(int64_t i = 0; i < pl.n_otu; ++i) {
		hu_diffabund_rec& x = rec[i];
		x.tested = 0; x.best = -1; x.prevalence = pl.prevalence[(size_t) i]; x.T_hi = x.T_lo = 0; x.count_ge = 0; x.H = x.p = x.p_maxT = x.q = nan;
	}
	std::vector<double> M(maxstat, maxstat + pl.perms);
	std::sort(M.begin(), M.end());
	std::vector<int64_t> order((size_t) m), C((size_t) pl.a);
	for(int64_t r = 0; r < m; ++r) {
		hu_diffabund_rec& x = rec[pl.row[(size_t) r]];
		x.tested = 1; x.T_hi = tobs[2 * r]; x.T_lo = tobs[2 * r + 1]; x.count_ge = count[r]; x.H = hobs[r];
		x.p = (double)(1 + count[r]) / (double)(pl.perms + 1);
		const int64_t ge = (int64_t)(M.end() - std::lower_bound(M.begin(), M.end(), hobs[r]));
		x.p_maxT = (double)(1 + ge) / (double)(pl.perms + 1);
		uint64_t hi, lo;
		hu_da_host_T(pl, r, pl.lab.data(), &hi, &lo, C.data());
		int64_t best = 0;
		for(int64_t g = 1; g < pl.a; ++g) if(C[(size_t) g] * pl.size[(size_t) best] > C[(size_t) best] * pl.size[(size_t) g]) best = g;
		x.best = (int32_t) best;
		order[(size_t) r] = r;
	}
	std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return rec[pl.row[(size_t) x]].p < rec[pl.row[(size_t) y]].p; });
	double run = 1.0;
	for(int64_t j = m; j >= 1; --j) {
		hu_diffabund_rec& x = rec[pl.row[(size_t) order[(size_t)(j - 1)]]];
		const double q = (x.p * (double) m) / (double) j;
		run = q < run ? q : run;
		x.q = run;
	}
}

extern "C" int hu_diffabund_ranks(int64_t M, int64_t N, const double* counts, int32_t rank_by, int32_t* r2_out) try {
	const char* fn = "hu_diffabund_ranks";
	if(!counts || !r2_out || M < 1 || N < 1 || N > HU_DA_MAX_SAMPLES || (rank_by != 0 && rank_by != 1)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	{ const int rc = da_check_cells(fn, M, N, counts); if(rc != HU_OK) return rc; }
	std::vector<double> tot;
	if(rank_by == 0) {
		da_totals(M, N, counts, tot);
		for(int64_t j = 0; j < N; ++j) if(!(tot[(size_t) j] > 0) || !std::isfinite(tot[(size_t) j])) {
			hu_set_error("%s: sample %lld has no reads: its fractions do not exist", fn, (long long) j); return HU_ERR_ARG; }
	}
	std::vector<std::pair<double, int32_t>> v; std::vector<int32_t> r2;
	for(int64_t i = 0; i < M; ++i) {
		da_row_values(N, counts + i * N, rank_by == 0 ? tot.data() : nullptr, v);
		da_rank_sorted(N, v, r2);
		int32_t* out = r2_out + i * N;
		const int32_t rz = (int32_t)(N - (int64_t) v.size()) + 1;
		for(int64_t j = 0; j < N; ++j) out[j] = rz;
		for(size_t c = 0; c < v.size(); ++c) out[v[c].second] = r2[c];
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_diffabund_ranks"); }
