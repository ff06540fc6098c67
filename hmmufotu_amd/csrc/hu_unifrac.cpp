// hu_unifrac and hu_unifrac_embed: the entries and the device path of hmmufotu-amd-unifrac.  The host makes the plan
// (hu_unifrac_host.cpp: the kept branches in depth-first order, the rows sorted by it, every branch's interval of rows); the kernels
// of hu_kern_unifrac.h fill P and add the pairs.  The number of launches does not depend on the table.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_unifrac.h"

static thread_local double g_ufTiming[4] = {0, 0, 0, 0};

#define UCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_unifrac_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_ufTiming, sizeof(g_ufTiming));
	return HU_OK;
}

/* the device path on a plan: P (compact [B][S], may be NULL), dist and pd (may be NULL) */
static int uf_device(const char* fn, int device, const HuUfPlan& pl, const double* counts, double* Pout, double* dist, double* pd) {
	g_ufTiming[0] = g_ufTiming[1] = g_ufTiming[2] = g_ufTiming[3] = 0;
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	const size_t M = (size_t) pl.M, S = (size_t) pl.S, B = (size_t) pl.B;
	const size_t Sp = (S + HU_UF_TILE - 1) / HU_UF_TILE * HU_UF_TILE;
	const size_t tiles = (size_t) hu_uf_tiles(pl.S), nSlab = (size_t) pl.nSlab;
	const size_t nBlk = (M + HU_UF_SCAN_ROWS - 1) / HU_UF_SCAN_ROWS;
	if(tiles > 0x7fffffffull) { hu_set_error("%s: %zu tiles: more than a grid holds", fn, tiles); return HU_ERR_ARG; }
	if(B == 0) {                                                       /* every read on the root: no branch, no device work */
		if(dist) std::fill(dist, dist + S * S, 0.0);
		if(pd) std::fill(pd, pd + S, 0.0);
		return HU_OK;
	}
	const size_t bC = (M + 1) * Sp * 8, bBlk = std::max<size_t>(nBlk, 1) * Sp * 8, bP = B * Sp * 8, bLen = B * 8, bIdx = B * 4,
		bPart = dist ? nSlab * tiles * 2 * HU_UF_TILE * HU_UF_TILE * 8 : 0, bDist = dist ? S * S * 8 : 0, bPd = pd ? (nSlab + 1) * Sp * 8 : 0;
	UCHK(hipSetDevice(device));
	{
		size_t freeB = 0, totB = 0;
		UCHK(hipMemGetInfo(&freeB, &totB));
		if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
		const size_t need = bC + bBlk + bP + bLen + 2 * bIdx + bPart + bDist + bPd + (1 << 20);
		if(need > freeB) {
			hu_set_error("%s: %zu branches x %zu samples need %zu bytes of device memory (P %zu, the scan %zu, the partial sums of %zu slabs %zu, the outputs %zu), %zu bytes are free",
				fn, B, S, need, bP, bC + bBlk, nSlab, bPart + bPd, bDist, freeB);
			return HU_ERR_NOMEM;
		}
	}
	double *dC = nullptr, *dBlk = nullptr, *dP = nullptr, *dLen = nullptr, *dPart = nullptr, *dDist = nullptr, *dPd = nullptr;
	int32_t *dLo = nullptr, *dHi = nullptr;
	HuScope guard([&] { (void) hipFree(dC); (void) hipFree(dBlk); (void) hipFree(dP); (void) hipFree(dLen); (void) hipFree(dPart); (void) hipFree(dDist); (void) hipFree(dPd);
		(void) hipFree(dLo); (void) hipFree(dHi); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	UCHK(hipMalloc((void**) &dC, bC)); UCHK(hipMalloc((void**) &dBlk, bBlk)); UCHK(hipMalloc((void**) &dP, bP)); UCHK(hipMalloc((void**) &dLen, bLen));
	UCHK(hipMalloc((void**) &dLo, bIdx)); UCHK(hipMalloc((void**) &dHi, bIdx));
	if(dist) { UCHK(hipMalloc((void**) &dPart, bPart)); UCHK(hipMalloc((void**) &dDist, bDist)); }
	if(pd) UCHK(hipMalloc((void**) &dPd, bPd));
	UCHK(hipMemset(dC, 0, bC));
	if(M > 0) {
		const double* src = counts;
		std::vector<double> sorted;
		if(!pl.permIsIdentity) {
			sorted.resize(M * S);
			for(size_t q = 0; q < M; ++q) memcpy(sorted.data() + q * S, counts + (size_t) pl.perm[q] * S, S * 8);
			src = sorted.data();
		}
		UCHK(hipMemcpy2D(dC + Sp, Sp * 8, src, S * 8, S * 8, M, hipMemcpyHostToDevice));
	}
	UCHK(hipMemcpy(dLen, pl.b.data(), bLen, hipMemcpyHostToDevice));
	UCHK(hipMemcpy(dLo, pl.lo.data(), bIdx, hipMemcpyHostToDevice)); UCHK(hipMemcpy(dHi, pl.hi.data(), bIdx, hipMemcpyHostToDevice));
	UCHK(hipDeviceSynchronize());
	g_ufTiming[0] = since();
	(void) hipGetLastError();
	const unsigned gx = (unsigned)(Sp / 256 + (Sp % 256 ? 1 : 0));
	if(nBlk > 0) {
		if(nBlk > 65535) { hu_set_error("%s: %zu rows: more than the scan's grid holds", fn, M); return HU_ERR_ARG; }
		k_unifrac_scan_sums<<<dim3(gx, (unsigned) nBlk), 256>>>(dC, dBlk, (int64_t) M, (int64_t) Sp);
		UCHK(hipGetLastError());
		k_unifrac_scan_offs<<<gx, 256>>>(dBlk, (int64_t) nBlk, (int64_t) Sp);
		UCHK(hipGetLastError());
		k_unifrac_scan_rows<<<dim3(gx, (unsigned) nBlk), 256>>>(dC, dBlk, (int64_t) M, (int64_t) Sp);
		UCHK(hipGetLastError());
	}
	for(size_t kb = 0; kb < B; kb += 65535) {                            /* grid.y holds 65535 */
		const size_t nb = std::min<size_t>(65535, B - kb);
		k_unifrac_gather<<<dim3(gx, (unsigned) nb), 256>>>(dC, dLo + kb, dHi + kb, dP + kb * Sp, (int64_t) M, (int64_t) S, (int64_t) Sp, (int64_t) nb);
		UCHK(hipGetLastError());
	}
	UCHK(hipDeviceSynchronize());
	g_ufTiming[1] = since() - g_ufTiming[0];
	if(dist) {
		const dim3 grid((unsigned) tiles, (unsigned) nSlab);
		switch(pl.method) {
		case HU_UF_UNWEIGHTED: k_unifrac_pairs<HU_UF_UNWEIGHTED><<<grid, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.L, pl.alpha); break;
		case HU_UF_WEIGHTED: k_unifrac_pairs<HU_UF_WEIGHTED><<<grid, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.L, pl.alpha); break;
		case HU_UF_WEIGHTED_RAW: k_unifrac_pairs<HU_UF_WEIGHTED_RAW><<<grid, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.L, pl.alpha); break;
		default: k_unifrac_pairs<HU_UF_GENERALIZED><<<grid, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.L, pl.alpha); break;
		}
		UCHK(hipGetLastError());
		k_unifrac_finish<<<dim3((unsigned) tiles, 16), 256>>>(dPart, dDist, (int64_t) S, (int64_t) Sp, (int64_t) nSlab, pl.method == HU_UF_WEIGHTED_RAW);
		UCHK(hipGetLastError());
	}
	if(pd) {
		k_unifrac_pd<<<dim3(gx, (unsigned) nSlab), 256>>>(dP, dLen, dPd + Sp, (int64_t) Sp, (int64_t) B, pl.L);
		UCHK(hipGetLastError());
		k_unifrac_pd_finish<<<gx, 256>>>(dPd + Sp, dPd, (int64_t) S, (int64_t) Sp, (int64_t) nSlab);
		UCHK(hipGetLastError());
	}
	UCHK(hipDeviceSynchronize());
	g_ufTiming[2] = since() - g_ufTiming[0] - g_ufTiming[1];
	if(dist) UCHK(hipMemcpy(dist, dDist, bDist, hipMemcpyDeviceToHost));
	if(pd) UCHK(hipMemcpy(pd, dPd, S * 8, hipMemcpyDeviceToHost));
	if(Pout) UCHK(hipMemcpy2D(Pout, S * 8, dP, Sp * 8, S * 8, B, hipMemcpyDeviceToHost));
	g_ufTiming[3] = since() - g_ufTiming[0] - g_ufTiming[1] - g_ufTiming[2];
	return HU_OK;
}

extern "C" int hu_unifrac(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, double* dist, double* pd) try {
	const char* fn = "hu_unifrac";
	if(!dist) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuUfPlan pl;
	const int rc = hu_uf_plan(fn, tree, n_otu, n_sample, otu_node, counts, opts, pl);
	if(rc != HU_OK) return rc;
	if(pl.host) {
		std::vector<double> P((size_t) pl.B * (size_t) pl.S);
		hu_uf_host_embed(pl, counts, P.data());
		hu_uf_host_pairs(pl, P.data(), dist, pd);
		return HU_OK;
	}
	return uf_device(fn, device, pl, counts, nullptr, dist, pd);
} catch(...) { return hu_catch_all("hu_unifrac"); }

extern "C" int hu_unifrac_embed(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, int64_t* n_branch, int64_t cap_branch, int32_t* branch_node, double* branch_len, double* P) try {
	const char* fn = "hu_unifrac_embed";
	if(!n_branch) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuUfPlan pl;
	const int rc = hu_uf_plan(fn, tree, n_otu, n_sample, otu_node, counts, opts, pl);
	if(rc != HU_OK) return rc;
	*n_branch = pl.B;
	if(!P) return HU_OK;
	if(cap_branch < pl.B) { hu_set_error("%s: room for %lld branches, %lld are kept", fn, (long long) cap_branch, (long long) pl.B); return HU_ERR_ARG; }
	if(branch_node) std::copy(pl.node.begin(), pl.node.end(), branch_node);
	if(branch_len) std::copy(pl.b.begin(), pl.b.end(), branch_len);
	if(pl.host) { hu_uf_host_embed(pl, counts, P); return HU_OK; }
	return uf_device(fn, device, pl, counts, P, nullptr, nullptr);
} catch(...) { return hu_catch_all("hu_unifrac_embed"); }
