// k_nni_score (hu_kern_nni.h) with the nine ratios of an edge in LDS against the same kernel with the ratios in
// a global scratch, over the column counts at which the number of workgroups a CU's 160 KB of LDS hold changes (4 up to 483 columns, 3 up
// to 672, 2 up to 1,052, 1 up to 2,190): 4,095 edges on random messages of similar neighbours drawn from 4,096 nodes, the best of five
// launches by events after a warm-up, the message bytes of pass 1 (128 per edge and column) over the kernel's time.  Not part of the
// library's build.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o nni_plain nni_plain.hip
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <vector>
#include <random>
#include "../../hmmufotu_amd/csrc/hu_kern_nni.h"

void hu_set_error(const char*, ...) {}
int hu_catch_all(const char*) noexcept { return -5; }

#define CK(c) do { hipError_t e_ = (c); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while(0)

int main() {
	const double H[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
	double U1[16], lam[4] = {0, -4.0 / 3, -4.0 / 3, -4.0 / 3};
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) U1[k * 4 + i] = H[i * 4 + k] / 4;
	HuBlenModel m;
	hu_blen_model_set(&m, H, lam, U1);
	const int32_t n = 4096, E = 4095;
	const int64_t Ls[12] = {128, 256, 483, 484, 672, 673, 1052, 1053, 2190, 2474, 4500, 7682};
	const int64_t Lmax = 7682, LdsMax = 2190;
	const size_t cells = (size_t) n * (size_t) Lmax;
	/* messages around an edge between similar sequences: the same dominant base in 9 cells of 10 */
	std::vector<double> hu(cells * 4), hd(cells * 4);
	std::mt19937_64 rng(5);
	std::uniform_real_distribution<double> un(0.0, 1.0);
	for(size_t c = 0; c < cells; ++c) {
		const int b0 = 0;                                          /* one dominant base: every layout [n][L] of these cells has similar neighbours */
		const int b = un(rng) < 0.9 ? b0 : (int)(rng() & 3), b2 = un(rng) < 0.9 ? b0 : (int)(rng() & 3);
		const bool leaf = un(rng) < 0.5;
		for(int i = 0; i < 4; ++i) {
			hu[c * 4 + i] = leaf ? (i == b ? 0.0 : -INFINITY) : std::log(i == b ? 0.9 : 0.02 + 0.03 * un(rng)) - 40.0 * un(rng);
			hd[c * 4 + i] = std::log(i == b2 ? 0.85 : 0.03 + 0.04 * un(rng)) - 300.0;
		}
	}
	std::vector<HuNniEdge> he((size_t) E);
	for(int32_t e = 0; e < E; ++e) {
		HuNniEdge& x = he[(size_t) e];
		memset(&x, 0, sizeof(x));
		x.u = e + 1; x.kind = HU_NNI_INNER; x.t0 = 0.1;
		for(int k = 0; k < 4; ++k) { x.msg[k] = (int32_t)(rng() % (uint64_t) n) + (k == 3 ? n : 0); x.len[k] = 0.02 + 0.2 * un(rng); }
	}
	double *up, *down, *ratio, *vec; int32_t* iters; HuNniEdge* edges; HuBlenModel* dm;
	CK(hipMalloc((void**) &up, cells * 32)); CK(hipMalloc((void**) &down, cells * 32)); CK(hipMalloc((void**) &ratio, (size_t) E * 72 * (size_t) Lmax));
	CK(hipMalloc((void**) &vec, (size_t) E * 56)); CK(hipMalloc((void**) &iters, (size_t) E * 12)); CK(hipMalloc((void**) &edges, (size_t) E * sizeof(HuNniEdge)));
	CK(hipMalloc((void**) &dm, sizeof(HuBlenModel)));
	CK(hipMemcpy(dm, &m, sizeof(m), hipMemcpyHostToDevice)); CK(hipMemcpy(edges, he.data(), (size_t) E * sizeof(HuNniEdge), hipMemcpyHostToDevice));
	std::vector<double> a1((size_t) E * 3), a2((size_t) E * 3);
	std::vector<int32_t> its((size_t) E * 3);
	CK(hipFuncSetAttribute((const void*) k_nni_score<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	for(int64_t L : Ls) {
		/* the messages of node x at [x][L][4]: another L only reads a prefix of another layout of the same random values */
		CK(hipMemcpy(up, hu.data(), (size_t) n * (size_t) L * 32, hipMemcpyHostToDevice)); CK(hipMemcpy(down, hd.data(), (size_t) n * (size_t) L * 32, hipMemcpyHostToDevice));
		HuNniArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.edges = edges; a.m = dm; a.csLen = L; a.n = n; a.nEdges = E; a.lo = 0.0; a.hi = 10.0;
		a.ratio = ratio; a.tStar = vec; a.f = vec + 3 * (size_t) E; a.f0 = vec + 6 * (size_t) E; a.iters = iters;
		const size_t lds = ((size_t) 3 * HU_NNI_WG + (size_t) 9 * L) * 8;
		float best[2] = {1e30f, 1e30f};
		for(int v = 0; v < 2; ++v) {
			if(v == 0 && L > LdsMax) continue;                     /* what 160 KB hold */
			for(int rep = 0; rep < 6; ++rep) {
				CK(hipEventRecord(e0));
				if(v == 0) k_nni_score<true><<<E, HU_NNI_WG, lds>>>(a);
				else k_nni_score<false><<<E, HU_NNI_WG, 3 * HU_NNI_WG * 8>>>(a);
				CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
				float ms; CK(hipEventElapsedTime(&ms, e0, e1));
				if(rep && ms < best[v]) best[v] = ms;
			}
			CK(hipMemcpy(v == 0 ? a1.data() : a2.data(), vec, (size_t) E * 24, hipMemcpyDeviceToHost));
			CK(hipMemcpy(its.data(), iters, (size_t) E * 12, hipMemcpyDeviceToHost));
		}
		double dmax = 0, itsum = 0;
		for(size_t i = 0; i < (size_t) E * 3; ++i) { if(L <= LdsMax) dmax = fmax(dmax, fabs(a1[i] - a2[i])); itsum += its[i]; }
		const double msg = 128.0 * E * L;
		if(L <= LdsMax) printf("L %lld: ratios in LDS %.3f ms, ratios in global %.3f ms; message bytes %.3g: %.3g / %.3g TB/s; mean Newton steps per arrangement %.2f, max |t* LDS - t* global| %.3g\n",
			(long long) L, best[0], best[1], msg, msg / best[0] * 1e-9, msg / best[1] * 1e-9, itsum / (3.0 * E), dmax);
		else printf("L %lld: ratios in LDS not run (beyond 160 KB), ratios in global %.3f ms; message bytes %.3g: %.3g TB/s; mean Newton steps per arrangement %.2f\n",
			(long long) L, best[1], msg, msg / best[1] * 1e-9, itsum / (3.0 * E));
	}
	return 0;
}
