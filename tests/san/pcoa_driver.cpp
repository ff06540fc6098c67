// The host half of hu_pcoa (hu_pcoa_host.cpp: the checks, the plan, the block iteration, the m x m work and the host's operations; with
// hu_permanova_host.cpp for the matrix checks and the trace) under AddressSanitizer + UBSan, as a stand-alone program.
//   pcoa_driver
// Shapes: n = 3, 4, 7, 17 and 65 (a block of 64 = n - 1 columns, and padded blocks of 16 and 32), k = 1, 2 and n - 1, blocks of one
// column, a block that is widened (to the ceiling of 64 columns too), and what the plan and the iteration refuse.  Checked on every result: the eigenvalues are positive and
// descend, every residual is within tol * lambda_1, a coordinate column has the squared length lambda_a and its largest entry is
// positive, and the coordinates give the distances back where the points have no more dimensions than axes were asked.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_pcoa.h"
#include "../../hmmufotu_amd/csrc/hu_permanova.h"

static char g_err[4096];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }
extern "C" const char* hu_last_error(void) { return g_err; }

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return 1; } while(0)

/* n points in q dimensions, the axes scaled 8, 4, 2, ... */
static std::vector<double> points(std::mt19937_64& g, int n, int q) {
	std::vector<double> x((size_t) n * q), d((size_t) n * n, 0.0);
	for(int i = 0; i < n; ++i) for(int c = 0; c < q; ++c) x[(size_t) i * q + c] = ((double)(g() % 200001) / 100000.0 - 1.0) * std::ldexp(8.0, -std::min(c, 6));
	for(int i = 0; i < n; ++i) for(int j = i + 1; j < n; ++j) {
		double s = 0;
		for(int c = 0; c < q; ++c) { const double t = x[(size_t) i * q + c] - x[(size_t) j * q + c]; s += t * t; }
		d[(size_t) i * n + j] = d[(size_t) j * n + i] = std::sqrt(s);
	}
	return d;
}

static int call(int n, const std::vector<double>& d, const hu_pcoa_opts& o, hu_pcoa_result* res, std::vector<double>& x, std::vector<double>& lam, std::vector<double>& rs) {
	HuPcPlan pl;
	int rc = hu_pc_plan("driver", n, d.data(), &o, pl);
	if(rc != HU_OK) return rc;
	x.assign((size_t)(n * o.k), 0.0); lam.assign((size_t) o.k, 0.0); rs.assign((size_t) o.k, 0.0);
	std::unique_ptr<HuPcOps> ops(hu_pc_host_ops(n, d.data()));
	memset(res, 0, sizeof(*res));
	return hu_pc_run("driver", *ops, pl, hu_pm_ss_total(n, d.data()), res, x.data(), lam.data(), rs.data());
}

static int run(int n, int q, int k, int over, const std::vector<double>& d) {
	hu_pcoa_opts o;
	hu_pcoa_default_opts(&o);
	o.k = k; o.oversample = over; o.host = 1; o.seed = 7;
	hu_pcoa_result res;
	std::vector<double> x, lam, rs;
	if(call(n, d, o, &res, x, lam, rs) != HU_OK) FAIL("n %d q %d k %d oversample %d refused", n, q, k, over);
	if(res.n != n || res.k != k || res.iterations < 1 || res.m_final < k || res.m_final > n - 1 || res.positive_in_block < k || !(res.trace > 0)) FAIL("n %d k %d: the result's header", n, k);
	for(int a = 0; a < k; ++a) {
		if(!(lam[(size_t) a] > 0) || (a && lam[(size_t) a] > lam[(size_t) a - 1]) || !(rs[(size_t) a] <= o.tol * lam[0])) FAIL("n %d k %d axis %d: lambda %g residual %g", n, k, a, lam[(size_t) a], rs[(size_t) a]);
		double ss = 0, big = 0, at = 0;
		for(int i = 0; i < n; ++i) { const double v = x[(size_t) i * k + a]; ss += v * v; if(std::fabs(v) > big) { big = std::fabs(v); at = v; } }
		if(std::fabs(ss - lam[(size_t) a]) > 1e-12 * lam[0] || !(at > 0)) FAIL("n %d k %d axis %d: squared length %g of lambda %g, largest entry %g", n, k, a, ss, lam[(size_t) a], at);
	}
	if(k >= q) for(int i = 0; i < n; ++i) for(int j = 0; j < n; ++j) {
		double s = 0;
		for(int a = 0; a < k; ++a) { const double t = x[(size_t) i * k + a] - x[(size_t) j * k + a]; s += t * t; }
		if(std::fabs(std::sqrt(s) - d[(size_t) i * n + j]) > 1e-7 * std::sqrt(lam[0])) FAIL("n %d k %d: the distance of %d and %d comes back as %g, not %g", n, k, i, j, std::sqrt(s), d[(size_t) i * n + j]);
	}
	return 0;
}

static int refused(const char* what, int want, int n, const std::vector<double>& d, const hu_pcoa_opts& o) {
	hu_pcoa_result res;
	std::vector<double> x, lam, rs;
	if(call(n, d, o, &res, x, lam, rs) != want) FAIL("%s: not refused as expected", what);
	return 0;
}

int main() {
	std::mt19937_64 g(20241020);
	int done = 0;
	for(int n : {3, 4, 7, 17, 65}) {
		const int q = std::min(3, n - 1);
		const std::vector<double> d = points(g, n, q);
		for(int k : {1, 2, q}) {
			if(k > q) continue;
			for(int over : {0, 8}) { if(run(n, q, k, over, d)) return 1; ++done; }             /* 3 x 2 per n, but n = 3: k = 1, 2, 2 */
		}
	}
	{	/* every axis of points in n - 1 dimensions: blocks of 6, 16 (no padding) and 64 = the ceiling */
		for(int n : {7, 17, 65}) { if(run(n, n - 1, n - 1, 8, points(g, n, n - 1))) return 1; ++done; }
	}
	{	/* the refusals */
		const std::vector<double> d = points(g, 5, 3);
		hu_pcoa_opts o, b;
		hu_pcoa_default_opts(&o); o.host = 1; o.k = 2;
		b = o; b.k = 0; if(refused("k = 0", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.k = 5; if(refused("k = n", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.oversample = -1; if(refused("oversample < 0", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.tol = 0; if(refused("tol = 0", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.tol = 1e-2; if(refused("tol = 1e-2", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.tol = NAN; if(refused("tol = NaN", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.max_it = 0; if(refused("max_it = 0", HU_ERR_ARG, 5, d, b)) return 1;
		b = o; b.k = 1; if(refused("n = 2", HU_ERR_ARG, 2, d, b)) return 1;
		std::vector<double> x = d; x[1] = -1; x[5] = -1;
		if(refused("a negative cell", HU_ERR_ARG, 5, x, o)) return 1;
		x = d; x[7] += 1;
		if(refused("an asymmetric matrix", HU_ERR_ARG, 5, x, o)) return 1;
		x = d; x[6] = 1;
		if(refused("a diagonal that is not zero", HU_ERR_ARG, 5, x, o)) return 1;
		x.assign(25, 0.0);
		if(refused("a matrix of zeros", HU_ERR_ARG, 5, x, o)) return 1;
		b = o; b.k = 4; if(refused("more axes than the points have dimensions", HU_ERR_NUMERIC, 5, d, b)) return 1;
		if(!strstr(g_err, "only 3 positive axes; 4 asked")) FAIL("the count of positive axes is not named");
		const std::vector<double> e = points(g, 65, 3);
		b = o; b.k = 1; b.oversample = 0; b.max_it = 1; if(refused("one iteration of the power method", HU_ERR_NUMERIC, 65, e, b)) return 1;
		if(!strstr(g_err, "no convergence in 1 iterations: axis 1")) FAIL("the worst axis is not named");
		const std::vector<double> f = points(g, 129, 3);                         /* widened to the ceiling of 64 columns, refused once the block has settled */
		b = o; b.k = 4; if(refused("four axes of points in three dimensions, n = 129", HU_ERR_NUMERIC, 129, f, b)) return 1;
		if(!strstr(g_err, "3 positive axes found in a settled block of 64 columns")) FAIL("the widest block's refusal");
		if(hu_pcoa_need(2, 1, 0) != -1 || hu_pcoa_need(65, 3, 8) != 8 * 65 * 65 + 8 * 5 * 65 * 16 + 8 * 4 * 256 + 8 * 16 + (1 << 20) || hu_pcoa_slabs(280) != 3) FAIL("hu_pcoa_need");
		++done;
	}
	{	/* the m x m work alone: L L' = G and Q Theta Q' = H */
		const int m = 9, ld = 16;
		std::vector<double> A((size_t) m * m), G((size_t) m * ld, 0.0), L, H, Q((size_t) m * ld), th((size_t) m);
		for(auto& v : A) v = (double)(g() % 2001) / 1000.0 - 1.0;
		for(int i = 0; i < m; ++i) for(int j = 0; j < m; ++j) { double s = i == j ? 1.0 : 0.0; for(int p = 0; p < m; ++p) s += A[(size_t) i * m + p] * A[(size_t) j * m + p]; G[(size_t) i * ld + j] = s; }
		L = G; H = G;
		int64_t fail = -1;
		if(!hu_pc_cholesky(m, ld, L.data(), &fail)) FAIL("a positive definite matrix has no factor at %lld", (long long) fail);
		hu_pc_jacobi(m, ld, H.data(), th.data(), Q.data());
		for(int i = 0; i < m; ++i) for(int j = 0; j < m; ++j) {
			double s = 0, t = 0;
			for(int p = 0; p < m; ++p) { s += L[(size_t) i * ld + p] * L[(size_t) j * ld + p]; t += Q[(size_t) i * ld + p] * th[(size_t) p] * Q[(size_t) j * ld + p]; }
			if(std::fabs(s - G[(size_t) i * ld + j]) > 1e-12 || std::fabs(t - G[(size_t) i * ld + j]) > 1e-12) FAIL("cell (%d, %d): L L' %g, Q Theta Q' %g, G %g", i, j, s, t, G[(size_t) i * ld + j]);
		}
		std::vector<double> Z((size_t) 2 * ld, 1.0);                              /* two equal columns: the second pivot is not positive */
		if(hu_pc_cholesky(2, ld, Z.data(), &fail) || fail != 1) FAIL("a singular matrix was factored");
		++done;
	}
	printf("%d cases\n", done);
	return 0;
}
