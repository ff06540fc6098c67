// k_nni_support (hu_kern_support.h) with the pairs (d^1_j, d^2_j) of an edge in LDS against the same kernel with
// the pairs in a global scratch, and with 1, 2, 4 and 8 replicates per thread, at 256, 483, 1,000, 2,474 and 7,682 columns and at the
// column counts where the workgroups a CU's 160 KB of LDS hold change (16 bytes a column and 6 KB of reduction scratch: 4 up to 2,176
// columns, 3 up to 3,029, 2 up to 4,736, 1 up to 9,856): 4,095 edges on random messages of similar neighbours drawn from 4,096 nodes,
// 1,000 replicates whose table k_support_weights draws, the optima t* made up.  The best of three launches by events after a warm-up;
// the table bytes phase B reads (2 per edge, column and replicate) over the kernel's time.  Not part of the library's build.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o support_plain support_plain.hip
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cmath>
#include <cstring>
#include <vector>
#include <random>
#include "../../hmmufotu_amd/csrc/hu_kern_support.h"

void hu_set_error(const char*, ...) {}
int hu_catch_all(const char*) noexcept { return -5; }

#define CK(c) do { hipError_t e_ = (c); if(e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while(0)

template<bool LDS, int RPT> static int run(const HuSupportArgs& a, size_t lds, hipEvent_t e0, hipEvent_t e1, float* best) {
	*best = 1e30f;
	for(int rep = 0; rep < 4; ++rep) {
		CK(hipEventRecord(e0));
		k_nni_support<LDS, RPT><<<a.nEdges, HU_NNI_WG, lds>>>(a);
		CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
		float ms; CK(hipEventElapsedTime(&ms, e0, e1));
		if(rep && ms < *best) *best = ms;
	}
	return 0;
}

int main() {
	const double H[16] = {1, 1, 1, 1, 1, 1, -1, -1, 1, -1, 1, -1, 1, -1, -1, 1};
	double U1[16], lam[4] = {0, -4.0 / 3, -4.0 / 3, -4.0 / 3};
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) U1[k * 4 + i] = H[i * 4 + k] / 4;
	HuBlenModel m;
	hu_blen_model_set(&m, H, lam, U1);
	const int32_t n = 4096, E = 4095;
	const int64_t Ls[9] = {256, 483, 1000, 2176, 2474, 3029, 3712, 4736, 7682};
	const int64_t Lmax = 7682, B = 1000, Bpad = 1000;              /* a multiple of 8: every RPT below reads aligned */
	const size_t cells = (size_t) n * (size_t) Lmax;
	std::vector<double> hu(cells * 4), hd(cells * 4);
	std::mt19937_64 rng(5);
	std::uniform_real_distribution<double> un(0.0, 1.0);
	for(size_t c = 0; c < cells; ++c) {
		const int b = un(rng) < 0.9 ? 0 : (int)(rng() & 3), b2 = un(rng) < 0.9 ? 0 : (int)(rng() & 3);
		const bool leaf = un(rng) < 0.5;
		for(int i = 0; i < 4; ++i) {
			hu[c * 4 + i] = leaf ? (i == b ? 0.0 : -INFINITY) : std::log(i == b ? 0.9 : 0.02 + 0.03 * un(rng)) - 40.0 * un(rng);
			hd[c * 4 + i] = std::log(i == b2 ? 0.85 : 0.03 + 0.04 * un(rng)) - 300.0;
		}
	}
	std::vector<HuNniEdge> he((size_t) E);
	std::vector<double> hts((size_t) E * 3);
	for(int32_t e = 0; e < E; ++e) {
		HuNniEdge& x = he[(size_t) e];
		memset(&x, 0, sizeof(x));
		x.u = e + 1; x.kind = HU_NNI_INNER; x.t0 = 0.1;
		for(int k = 0; k < 4; ++k) { x.msg[k] = (int32_t)(rng() % (uint64_t) n) + (k == 3 ? n : 0); x.len[k] = 0.02 + 0.2 * un(rng); }
		for(int q = 0; q < 3; ++q) hts[(size_t) e * 3 + q] = 0.01 + 0.2 * un(rng);
	}
	double *up, *down, *scratch, *ts, *f2; int32_t* cnt; HuNniEdge* edges; HuBlenModel* dm; uint16_t* Wt;
	CK(hipMalloc((void**) &up, cells * 32)); CK(hipMalloc((void**) &down, cells * 32)); CK(hipMalloc((void**) &scratch, (size_t) E * 72 * (size_t) Lmax));
	CK(hipMalloc((void**) &ts, (size_t) E * 24)); CK(hipMalloc((void**) &f2, (size_t) E * 24)); CK(hipMalloc((void**) &cnt, (size_t) E * 8));
	CK(hipMalloc((void**) &edges, (size_t) E * sizeof(HuNniEdge))); CK(hipMalloc((void**) &dm, sizeof(HuBlenModel)));
	CK(hipMalloc((void**) &Wt, (size_t) Lmax * Bpad * 2));
	CK(hipMemcpy(dm, &m, sizeof(m), hipMemcpyHostToDevice)); CK(hipMemcpy(edges, he.data(), (size_t) E * sizeof(HuNniEdge), hipMemcpyHostToDevice));
	CK(hipMemcpy(ts, hts.data(), (size_t) E * 24, hipMemcpyHostToDevice));
	CK(hipFuncSetAttribute((const void*) k_nni_support<true, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	CK(hipFuncSetAttribute((const void*) k_nni_support<true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	CK(hipFuncSetAttribute((const void*) k_nni_support<true, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	CK(hipFuncSetAttribute((const void*) k_nni_support<true, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
	std::vector<int32_t> c1((size_t) E), c2((size_t) E);
	for(int64_t L : Ls) {
		CK(hipMemcpy(up, hu.data(), (size_t) n * (size_t) L * 32, hipMemcpyHostToDevice)); CK(hipMemcpy(down, hd.data(), (size_t) n * (size_t) L * 32, hipMemcpyHostToDevice));
		CK(hipMemset(Wt, 0, (size_t) L * Bpad * 2));
		float wms = 0;
		CK(hipEventRecord(e0));
		k_support_weights<<<(unsigned)((B + 255) / 256), 256>>>(Wt, L, B, Bpad, 1);
		CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipGetLastError()); CK(hipEventElapsedTime(&wms, e0, e1));
		HuSupportArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.edges = edges; a.m = dm; a.csLen = L; a.B = B; a.Bpad = Bpad; a.n = n; a.nEdges = E;
		a.tStar = ts; a.Wt = Wt; a.dScratch = scratch; a.f2 = f2; a.count = cnt; a.bad = cnt + E; a.sums = nullptr;
		const size_t lds = ((size_t) 3 * HU_NNI_WG + (size_t) 2 * L) * 8, red = (size_t) 3 * HU_NNI_WG * 8;
		float t[2][4];
		if(run<true, 1>(a, lds, e0, e1, &t[0][0]) || run<true, 2>(a, lds, e0, e1, &t[0][1]) || run<true, 4>(a, lds, e0, e1, &t[0][2])) return 1;
		CK(hipMemcpy(c1.data(), cnt, (size_t) E * 4, hipMemcpyDeviceToHost));
		if(run<true, 8>(a, lds, e0, e1, &t[0][3])) return 1;
		if(run<false, 1>(a, red, e0, e1, &t[1][0]) || run<false, 2>(a, red, e0, e1, &t[1][1]) || run<false, 4>(a, red, e0, e1, &t[1][2])) return 1;
		CK(hipMemcpy(c2.data(), cnt, (size_t) E * 4, hipMemcpyDeviceToHost));
		if(run<false, 8>(a, red, e0, e1, &t[1][3])) return 1;
		int64_t differ = 0, total = 0;
		for(int32_t e = 0; e < E; ++e) { differ += c1[(size_t) e] != c2[(size_t) e]; total += c1[(size_t) e]; }
		const double bytes = 2.0 * E * L * B;
		printf("L %lld: weights %.3f ms; pairs in LDS, 1/2/4/8 replicates a thread: %.3f %.3f %.3f %.3f ms; pairs in global: %.3f %.3f %.3f %.3f ms; "
			"table bytes %.3g: %.3g (LDS, 4) / %.3g (global, 4) TB/s; edges whose count differs between the two: %lld, mean count %.1f\n",
			(long long) L, wms, t[0][0], t[0][1], t[0][2], t[0][3], t[1][0], t[1][1], t[1][2], t[1][3], bytes, bytes / t[0][2] * 1e-9, bytes / t[1][2] * 1e-9,
			(long long) differ, (double) total / E);
	}
	return 0;
}
