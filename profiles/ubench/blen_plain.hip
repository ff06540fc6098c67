// k_blen_step (hu_kern_blen.h) against the plain formulation of the same step, which reads the two messages of a
// column again at every evaluation of f' (eight exp, the products and the divisions per column and evaluation), and the ratios in LDS
// against the ratios in global memory: 8,190 branches of random messages of similar neighbours, the best of five launches by events
// after a warm-up, the message bytes of pass 1 over the kernel's time.  Not part of the library's build.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o blen_plain blen_plain.hip
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <vector>
#include <random>
#include "../../hmmufotu_amd/csrc/hu_kern_blen.h"

void hu_set_error(const char*, ...) {}
int hu_catch_all(const char*) noexcept { return -5; }

__global__ __launch_bounds__(HU_BLEN_WG) void k_blen_plain(HuBlenArgs a) {
	extern __shared__ __attribute__((aligned(16))) double blen_sm[];
	const int64_t u = blockIdx.x, L = a.csLen;
	if(u >= a.n || u == a.root) return;
	const int tid = threadIdx.x;
	double* red = blen_sm;
	const double* mu = a.up + u * L * 4;
	const double* md = a.down + u * L * 4;
	const double t0 = a.t[u];
	HuBlenExp E;
	auto eval3 = [&](double x, double* f, double* g, double* h) {
		hu_blen_exp(a.m, x, &E);
		double w[3] = {0.0, 0.0, 0.0};
		for(int64_t j = tid; j < L; j += HU_BLEN_WG) {
			double Mu[4], Md[4], r[3], K, p, q;
			const double2 p0 = *reinterpret_cast<const double2*>(mu + j * 4), p1 = *reinterpret_cast<const double2*>(mu + j * 4 + 2);
			const double2 q0 = *reinterpret_cast<const double2*>(md + j * 4), q1 = *reinterpret_cast<const double2*>(md + j * 4 + 2);
			Mu[0] = p0.x; Mu[1] = p0.y; Mu[2] = p1.x; Mu[3] = p1.y; Md[0] = q0.x; Md[1] = q0.y; Md[2] = q1.x; Md[3] = q1.y;
			hu_blen_column(a.m, Mu, Md, r, &K);
			hu_blen_terms(E, r, &p, &q);
			w[0] += K; w[1] += p; w[2] += q;
		}
		blen_reduce<3>(red, w);
		*f = w[0]; *g = w[1]; *h = w[2];
	};
	double f0, g0, h0;
	eval3(t0, &f0, &g0, &h0);
	auto eval = [&](double x, double* g, double* h) { double f; eval3(x, &f, g, h); };
	if(tid == 0) { a.f[u] = f0; a.d1[u] = g0; a.d2[u] = h0; }
	int it = 0;
	const double x = hu_blen_solve(t0, g0, h0, a.lo, a.hi, eval, &it);
	if(tid == 0) { a.tStar[u] = x; a.iters[u] = it; }
}

#define CK(c) do { hipError_t e_ = (c); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while(0)

int main() {
	const double H[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
	double U1[16], lam[4] = {0, -4.0 / 3, -4.0 / 3, -4.0 / 3};
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) U1[k * 4 + i] = H[i * 4 + k] / 4;
	HuBlenModel m;
	hu_blen_model_set(&m, H, lam, U1);
	const int32_t n = 8191;
	const int64_t Ls[9] = {256, 1000, 2000, 2474, 3157, 3158, 4500, 6570, 7682};
	const int64_t Lmax = 7682;
	const size_t cells = (size_t) n * (size_t) Lmax;
	/* messages of a branch between two similar sequences: the same dominant base on either side in 9 columns of 10 */
	std::vector<double> hu(cells * 4), hd(cells * 4);
	std::mt19937_64 rng(5);
	std::uniform_real_distribution<double> un(0.0, 1.0);
	for(size_t c = 0; c < cells; ++c) {
		const int b = (int)(rng() & 3), b2 = un(rng) < 0.9 ? b : (int)(rng() & 3);
		const bool leaf = un(rng) < 0.5;
		for(int i = 0; i < 4; ++i) {
			hu[c * 4 + i] = leaf ? (i == b ? 0.0 : -INFINITY) : std::log(i == b ? 0.9 : 0.02 + 0.03 * un(rng)) - 40.0 * un(rng);
			hd[c * 4 + i] = std::log(i == b2 ? 0.85 : 0.03 + 0.04 * un(rng)) - 300.0;
		}
	}
	double *up, *down, *ratio, *vec; int32_t* iters;
	CK(hipMalloc((void**) &up, cells * 32)); CK(hipMalloc((void**) &down, cells * 32)); CK(hipMalloc((void**) &ratio, cells * 24));
	CK(hipMalloc((void**) &vec, (size_t) n * 40)); CK(hipMalloc((void**) &iters, (size_t) n * 4));
	CK(hipMemcpy(up, hu.data(), cells * 32, hipMemcpyHostToDevice)); CK(hipMemcpy(down, hd.data(), cells * 32, hipMemcpyHostToDevice));
	std::vector<double> t((size_t) n, 0.3), a1((size_t) n), a2((size_t) n);
	std::vector<int32_t> its((size_t) n);
	CK(hipMemcpy(vec, t.data(), (size_t) n * 8, hipMemcpyHostToDevice));
	CK(hipFuncSetAttribute((const void*) k_blen_step<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	for(int64_t L : Ls) {
		HuBlenArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.t = vec; a.csLen = L; a.n = n; a.root = 0; a.doStep = 1; a.lo = 0.0; a.hi = 10.0;
		a.ratio = ratio; a.tStar = vec + n; a.f = vec + 2 * (size_t) n; a.d1 = vec + 3 * (size_t) n; a.d2 = vec + 4 * (size_t) n; a.iters = iters; a.m = m;
		const size_t lds = ((size_t) 3 * HU_BLEN_WG + (size_t) 3 * L) * 8;
		float best[3] = {1e30f, 1e30f, 1e30f};
		for(int v = 0; v < 3; ++v) {
			if(v == 0 && L > 6570) continue;                       /* what 160 KB hold */
			for(int rep = 0; rep < 6; ++rep) {
				CK(hipEventRecord(e0));
				if(v == 0) k_blen_step<true><<<n, HU_BLEN_WG, lds>>>(a);
				else if(v == 1) k_blen_step<false><<<n, HU_BLEN_WG, 3 * HU_BLEN_WG * 8>>>(a);
				else k_blen_plain<<<n, HU_BLEN_WG, 3 * HU_BLEN_WG * 8>>>(a);
				CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
				float ms; CK(hipEventElapsedTime(&ms, e0, e1));
				if(rep && ms < best[v]) best[v] = ms;
			}
			CK(hipMemcpy(v == 2 ? a2.data() : a1.data(), vec + n, (size_t) n * 8, hipMemcpyDeviceToHost));
			CK(hipMemcpy(its.data(), iters, (size_t) n * 4, hipMemcpyDeviceToHost));
		}
		double dmax = 0, itsum = 0; int inner = 0;
		for(int32_t u = 1; u < n; ++u) { dmax = fmax(dmax, fabs(a1[u] - a2[u])); itsum += its[u]; if(a2[u] > 0 && a2[u] < 10) ++inner; }
		const double msg = 64.0 * (n - 1) * L;
		printf("L %lld: ratios in LDS %.3f ms (1e30: not run), ratios in global %.3f ms, plain %.3f ms; message bytes %.3g: %.3g / %.3g / %.3g TB/s; mean Newton steps %.2f, inner optima %d of %d, max |t* ratio - t* plain| %.3g\n",
			(long long) L, best[0], best[1], best[2], msg, msg / best[0] * 1e-9, msg / best[1] * 1e-9, msg / best[2] * 1e-9, itsum / (n - 1), inner, n - 1, dmax);
	}
	return 0;
}
