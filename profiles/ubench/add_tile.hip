// k_add_score (hu_kern_add.h) at tiles of 1, 4, 16 and 64 queries against the plain formulation of the same
// scores, one workgroup per (edge, query) that computes the junction of the edge again at every evaluation of f' (two carries with
// their exp per column and evaluation): 2,046 edges of random messages around one dominant base per column, 64 queries that share
// that base in 17 columns of 20, at 256, 1,450, 1,451 and 7,682 columns.  The best of three launches by events after a warm-up;
// the rate is (edge, query, column) triples per second of the whole launch.  Not part of the library's build.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o add_tile add_tile.hip
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <vector>
#include <random>
#include "../../hmmufotu_amd/csrc/hu_kern_add.h"

void hu_set_error(const char*, ...) {}
int hu_catch_all(const char*) noexcept { return -5; }

__global__ __launch_bounds__(HU_ADD_WG) void k_add_plain(HuAddArgs a) {
	__shared__ double red[3 * HU_ADD_WG];
	__shared__ double P[16], tab[HU_ADD_TAB];
	const int64_t w = blockIdx.x, q = blockIdx.y, L = a.csLen, n = a.n;
	if(w >= n || q >= a.nq || w == a.root) return;
	const int tid = threadIdx.x;
	const HuBlenModel& m = *a.m;
	if(tid < 16) P[tid] = hu_nni_pentry(m, 0.5 * a.blen[w], tid >> 2, tid & 3);
	else if(tid < 16 + HU_ADD_TAB) tab[tid - 16] = hu_add_tab_entry(m, tid - 16);
	__syncthreads();
	const double* mu = a.up + w * L * 4;
	const double* md = a.down + w * L * 4;
	const int8_t* row = a.q + q * L;
	HuBlenExp E;
	auto eval3 = [&](double x, double* f, double* g, double* h) {
		hu_blen_exp(m, x, &E);
		double v[3] = {0.0, 0.0, 0.0};
		for(int64_t j = tid; j < L; j += HU_ADD_WG) {
			double Mu[4], Md[4], rho[3], r[3], K, p, c;
			const double2 p0 = *reinterpret_cast<const double2*>(mu + j * 4), p1 = *reinterpret_cast<const double2*>(mu + j * 4 + 2);
			const double2 c0 = *reinterpret_cast<const double2*>(md + j * 4), c1 = *reinterpret_cast<const double2*>(md + j * 4 + 2);
			Mu[0] = p0.x; Mu[1] = p0.y; Mu[2] = p1.x; Mu[3] = p1.y; Md[0] = c0.x; Md[1] = c0.y; Md[2] = c1.x; Md[3] = c1.y;
			hu_add_edge_column(m, P, Mu, Md, rho, &K);
			const int s = hu_add_sym(row[j]);
			hu_add_ratio(tab, s, rho[0], rho[1], rho[2], r);
			hu_blen_terms(E, r, &p, &c);
			v[0] += (K + tab[15 + s]) + log(hu_blen_den(E, r)); v[1] += p; v[2] += c;
		}
		blen_reduce<3>(red, v);
		*f = v[0]; *g = v[1]; *h = v[2];
	};
	double f0, g0, h0, f1, g1, h1;
	eval3(a.t0, &f0, &g0, &h0);
	auto eval = [&](double x, double* g, double* h) { double f; eval3(x, &f, g, h); };
	int it = 0;
	const double x = hu_blen_solve(a.t0, g0, h0, a.lo, a.hi, eval, &it);
	eval3(x, &f1, &g1, &h1);
	if(tid == 0) { a.tStar[q * n + w] = x; a.f[q * n + w] = f1; }
}

#define CK(c) do { hipError_t e_ = (c); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while(0)

int main() {
	const double H[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
	double U1[16], lam[4] = {0, -4.0 / 3, -4.0 / 3, -4.0 / 3};
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) U1[k * 4 + i] = H[i * 4 + k] / 4;
	HuBlenModel m;
	hu_blen_model_set(&m, H, lam, U1);
	const int32_t n = 2047, nq = 64;
	const int64_t Ls[4] = {256, 1450, 1451, 7682};
	const int32_t tiles[4] = {1, 4, 16, 64};
	const int64_t Lmax = 7682;
	const size_t cells = (size_t) n * (size_t) Lmax;
	std::vector<double> hu(cells * 4), hd(cells * 4), hb((size_t) n, 0.1);
	std::vector<int8_t> hq((size_t) nq * (size_t) Lmax);
	std::mt19937_64 rng(7);
	std::uniform_real_distribution<double> un(0.0, 1.0);
	std::vector<int> col((size_t) Lmax);
	for(auto& b : col) b = (int)(rng() & 3);
	for(size_t c = 0; c < cells; ++c) {
		const int b0 = col[c % (size_t) Lmax], b = un(rng) < 0.9 ? b0 : (int)(rng() & 3), b2 = un(rng) < 0.9 ? b0 : (int)(rng() & 3);
		const bool leaf = un(rng) < 0.5;
		for(int i = 0; i < 4; ++i) {
			hu[c * 4 + i] = leaf ? (i == b ? 0.0 : -INFINITY) : std::log(i == b ? 0.9 : 0.02 + 0.03 * un(rng)) - 40.0 * un(rng);
			hd[c * 4 + i] = std::log(i == b2 ? 0.85 : 0.03 + 0.04 * un(rng)) - 300.0;
		}
	}
	for(size_t c = 0; c < hq.size(); ++c) { const double x = un(rng); hq[c] = x < 0.05 ? (int8_t) -2 : x < 0.85 ? (int8_t) col[c % (size_t) Lmax] : (int8_t)(rng() & 3); }
	for(auto& b : hb) b = 0.02 + 0.2 * un(rng);
	double *up, *down, *blen, *ratio, *vec; int8_t* q; HuBlenModel* dm;
	const size_t nOut = (size_t) nq * (size_t) n, ratioBytes = (size_t) nq * (size_t) n * 24 * (size_t) Lmax;      /* a tile of 1: one scratch per (edge, query) */
	CK(hipMalloc((void**) &up, cells * 32)); CK(hipMalloc((void**) &down, cells * 32)); CK(hipMalloc((void**) &blen, (size_t) n * 8));
	CK(hipMalloc((void**) &ratio, ratioBytes)); CK(hipMalloc((void**) &vec, nOut * 16)); CK(hipMalloc((void**) &q, hq.size())); CK(hipMalloc((void**) &dm, sizeof(m)));
	CK(hipMemcpy(up, hu.data(), cells * 32, hipMemcpyHostToDevice)); CK(hipMemcpy(down, hd.data(), cells * 32, hipMemcpyHostToDevice));
	CK(hipMemcpy(blen, hb.data(), (size_t) n * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(dm, &m, sizeof(m), hipMemcpyHostToDevice));
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	std::vector<double> ref(nOut), got(nOut);
	for(int64_t L : Ls) {
		/* the rows of the queries at this width */
		std::vector<int8_t> rows((size_t) nq * (size_t) L);
		for(int32_t k = 0; k < nq; ++k) memcpy(rows.data() + (size_t) k * L, hq.data() + (size_t) k * Lmax, (size_t) L);
		CK(hipMemcpy(q, rows.data(), rows.size(), hipMemcpyHostToDevice));
		HuAddArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.blen = blen; a.q = q; a.m = dm; a.csLen = L; a.n = n; a.root = 0; a.nq = nq; a.lo = 0.0; a.hi = 10.0; a.t0 = 0.1;
		a.ratio = ratio; a.tStar = vec; a.f = vec + nOut;
		float best[5] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
		double dmax = 0;
		for(int v = 4; v >= 0; --v) {
			a.tile = v < 4 ? tiles[v] : 1;
			const dim3 grid((unsigned) n, (unsigned)(v < 4 ? (nq + a.tile - 1) / a.tile : nq));
			for(int rep = 0; rep < 4; ++rep) {
				CK(hipEventRecord(e0));
				if(v == 4) k_add_plain<<<grid, HU_ADD_WG>>>(a);
				else if(L <= HU_BLEN_LDS_COLS) k_add_score<true><<<grid, HU_ADD_WG, ((size_t) 3 * HU_ADD_WG + (size_t) 3 * L) * 8>>>(a);
				else k_add_score<false><<<grid, HU_ADD_WG, (size_t) 3 * HU_ADD_WG * 8>>>(a);
				CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
				float ms; CK(hipEventElapsedTime(&ms, e0, e1));
				if(rep && ms < best[v]) best[v] = ms;
			}
			CK(hipMemcpy(v == 4 ? ref.data() : got.data(), vec, nOut * 8, hipMemcpyDeviceToHost));
			if(v < 4) for(size_t i = 0; i < nOut; ++i) if(i % (size_t) n != 0) dmax = fmax(dmax, fabs(got[i] - ref[i]));
		}
		int inner = 0;
		for(size_t i = 0; i < nOut; ++i) if(i % (size_t) n != 0 && ref[i] > 0 && ref[i] < 10) ++inner;
		const double triples = (double)(n - 1) * nq * (double) L;
		printf("L %lld: tile 1 %.3f ms, tile 4 %.3f ms, tile 16 %.3f ms, tile 64 %.3f ms, plain %.3f ms; triples %.3g: %.3g / %.3g / %.3g / %.3g / %.3g per s; inner optima %d of %zu, max |t* tiled - t* plain| %.3g\n",
			(long long) L, best[0], best[1], best[2], best[3], best[4], triples, triples / best[0] * 1e3, triples / best[1] * 1e3, triples / best[2] * 1e3, triples / best[3] * 1e3,
			triples / best[4] * 1e3, inner, nOut - (size_t) nq, dmax);
		fflush(stdout);
	}
	return 0;
}
