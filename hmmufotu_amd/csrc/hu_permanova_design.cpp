// hu_permanova_design: the entry and the device path of hmmufotu-amd-permanova --design.  The host checks the call and
// computes SS_T (hu_permanova_design_host.cpp, hu_permanova_host.cpp); the kernels of hu_kern_permanova_design.h shuffle the index arrays
// of a chunk of permutations and form the quadratic forms of every design column.  The identity runs through the same kernels in a
// launch of its own, so that the observed statistic's bits are the kernels'.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_permanova_design.h"

static thread_local double g_pmdTiming[4] = {0, 0, 0, 0};

#define DCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_permanova_design_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_pmdTiming, sizeof(g_pmdTiming));
	return HU_OK;
}

static int64_t pmd_need(const HuPmdPlan& pl, int64_t chunk) { return hu_permanova_design_need(pl.n, pl.q, pl.T, chunk, pl.index32 ? 1 : 0); }

static int pmd_nomem(const char* fn, const HuPmdPlan& pl, int64_t chunk, size_t freeB) {
	hu_set_error("%s: %lld samples, %lld design columns and a chunk of %lld permutations need %lld bytes of device memory (the matrix %lld, the partial sums %lld), %zu bytes are free",
		fn, (long long) pl.n, (long long) pl.q, (long long) chunk, (long long) pmd_need(pl, chunk), (long long)(8 * pl.n * pl.n),
		(long long)(8 * hu_pmd_row_blocks(pl.n) * hu_pc_slabs(pl.n) * hu_pmd_vcpad(chunk, pl.q)), freeB);
	return HU_ERR_NOMEM;
}

/* the chunk of a call under `freeB` bytes: the one asked for, or the largest multiple of 64 that fits (16,384 at the most); 0: none fits */
static int64_t pmd_chunk(const HuPmdPlan& pl, size_t freeB) {
	if(pl.chunk > 0) { const int64_t c = std::min(pl.chunk, pl.perms); return (size_t) pmd_need(pl, c) <= freeB ? c : 0; }
	int64_t c = std::min<int64_t>(hu_pmd_pad(pl.perms), HU_PMD_MAX_CHUNK);
	while(c > 0 && (size_t) pmd_need(pl, c) > freeB) c -= HU_PMD_SLOT;
	return std::min(c, pl.perms);
}

template<class I> static int pmd_device(const char* fn, int device, const HuPmdPlan& pl, const double* dist, const double* Q, double* ss) {
	g_pmdTiming[0] = g_pmdTiming[1] = g_pmdTiming[2] = g_pmdTiming[3] = 0;
	const int64_t n = pl.n, q = pl.q, T = pl.T, rowBlocks = hu_pmd_row_blocks(n), slabs = hu_pc_slabs(n), slabLen = hu_pc_slab_len(n);
	if(pl.budget > 0 && pmd_chunk(pl, (size_t) pl.budget) == 0)          /* the caller's budget needs no device to refuse */
		return pmd_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, (size_t) pl.budget);
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	DCHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	DCHK(hipMemGetInfo(&freeB, &totB));
	if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
	const int64_t chunk = pmd_chunk(pl, freeB);
	if(chunk == 0) return pmd_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, freeB);
	const int64_t cp = hu_pmd_pad(chunk), vcPad = hu_pmd_vcpad(chunk, q);
	if(vcPad / 16 > 0x7fffffffll) { hu_set_error("%s: a chunk of %lld permutations of %lld columns: more column blocks than a grid holds", fn, (long long) chunk, (long long) q); return HU_ERR_ARG; }
	double *dD2 = nullptr, *dQ = nullptr, *dPart = nullptr, *dS = nullptr, *dSs = nullptr;
	I* dIdx = nullptr; int32_t *dMember = nullptr, *dStart = nullptr; int64_t* dTerm = nullptr;
	HuScope guard([&] { (void) hipFree(dD2); (void) hipFree(dQ); (void) hipFree(dPart); (void) hipFree(dS); (void) hipFree(dSs); (void) hipFree(dIdx);
		(void) hipFree(dMember); (void) hipFree(dStart); (void) hipFree(dTerm); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	DCHK(hipMalloc((void**) &dD2, (size_t)(8 * n * n))); DCHK(hipMalloc((void**) &dQ, (size_t)(8 * n * q)));
	DCHK(hipMalloc((void**) &dIdx, sizeof(I) * (size_t)(n * cp))); DCHK(hipMalloc((void**) &dPart, (size_t)(8 * rowBlocks * slabs * vcPad)));
	DCHK(hipMalloc((void**) &dS, (size_t)(8 * vcPad))); DCHK(hipMalloc((void**) &dSs, (size_t)(8 * cp * T)));
	DCHK(hipMalloc((void**) &dMember, (size_t)(4 * n))); DCHK(hipMalloc((void**) &dStart, (size_t)(4 * (pl.S + 1)))); DCHK(hipMalloc((void**) &dTerm, (size_t)(8 * (T + 1))));
	DCHK(hipMemcpy(dD2, dist, (size_t)(8 * n * n), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dQ, Q, (size_t)(8 * n * q), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dMember, pl.member.data(), (size_t)(4 * n), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dStart, pl.start.data(), (size_t)(4 * (pl.S + 1)), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dTerm, pl.term_start.data(), (size_t)(8 * (T + 1)), hipMemcpyHostToDevice));
	k_pmd_square<<<(unsigned) std::min<int64_t>((n * n + 255) / 256, 65536), 256>>>(dD2, n * n);
	DCHK(hipGetLastError());
	DCHK(hipDeviceSynchronize());
	g_pmdTiming[0] = since();
	std::vector<double> hs((size_t)(cp * T));
	/* one launch: its slots [0, cnt) are permutations first .. first + cnt - 1, or (observed) slot 0 is the identity */
	auto run = [&](int64_t first, int64_t cnt, bool observed) -> int {
		const int64_t c = hu_pmd_pad(cnt), nvc = cnt * q;
		double ta = since();
		k_index_shuffle<I><<<(unsigned)(c / HU_PMD_SLOT), HU_PMD_SLOT>>>(dIdx, dMember, dStart, pl.S, n, cp, (uint64_t) first, pl.seed, observed ? 1 : 0);
		DCHK(hipGetLastError());
		DCHK(hipDeviceSynchronize());
		double tb = since();
		g_pmdTiming[1] += tb - ta;
		const int nt = nvc <= 16 ? 1 : nvc <= 32 ? 2 : 4;                   /* accumulator tiles per wave: a cell's bits do not depend on it */
		const int64_t mp = 16 * nt, colBlocks = (nvc + mp - 1) / mp;
		const dim3 grid((unsigned) colBlocks, (unsigned) rowBlocks, (unsigned) slabs);
		if(nt == 1) k_pmd_quad<1, I><<<grid, 256>>>(dD2, dQ, dIdx, dPart, n, q, cp, nvc, vcPad, slabLen);
		else if(nt == 2) k_pmd_quad<2, I><<<grid, 256>>>(dD2, dQ, dIdx, dPart, n, q, cp, nvc, vcPad, slabLen);
		else k_pmd_quad<4, I><<<grid, 256>>>(dD2, dQ, dIdx, dPart, n, q, cp, nvc, vcPad, slabLen);
		DCHK(hipGetLastError());
		DCHK(hipDeviceSynchronize());
		ta = since();
		g_pmdTiming[2] += ta - tb;
		k_pmd_finish<<<(unsigned)((colBlocks * mp + 255) / 256), 256>>>(dPart, dS, rowBlocks, slabs, vcPad, colBlocks * mp);
		DCHK(hipGetLastError());
		k_pmd_terms<<<(unsigned)((cnt * T + 255) / 256), 256>>>(dS, dTerm, dSs, cnt, T, q);
		DCHK(hipGetLastError());
		DCHK(hipMemcpy(hs.data(), dSs, (size_t)(8 * cnt * T), hipMemcpyDeviceToHost));
		g_pmdTiming[3] += since() - ta;
		return HU_OK;
	};
	int rc = run(0, 1, true);
	if(rc != HU_OK) return rc;
	std::copy(hs.begin(), hs.begin() + T, ss);
	for(int64_t first = 0; first < pl.perms; first += chunk) {
		const int64_t cnt = std::min(chunk, pl.perms - first);
		rc = run(first, cnt, false);
		if(rc != HU_OK) return rc;
		std::copy(hs.begin(), hs.begin() + cnt * T, ss + (1 + first) * T);
	}
	return HU_OK;
}

extern "C" int hu_permanova_design(int device, int64_t n, const double* dist, const double* Q, int64_t q, int64_t T, const int64_t* term_start, const int32_t* strata,
		const hu_permanova_design_opts* opts, hu_permanova_design_term* result, double* ss_perm) try {
	const char* fn = "hu_permanova_design";
	if(!result) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuPmdPlan pl;
	int rc = hu_pmd_plan(fn, n, dist, Q, q, T, term_start, strata, opts, pl);
	if(rc != HU_OK) return rc;
	std::vector<double> ss((size_t)((1 + pl.perms) * T));
	if(pl.host || device < 0) hu_pmd_host_run(pl, dist, Q, ss.data());
	else if((rc = pl.index32 ? pmd_device<uint32_t>(fn, device, pl, dist, Q, ss.data()) : pmd_device<uint16_t>(fn, device, pl, dist, Q, ss.data())) != HU_OK) return rc;
	hu_pmd_result(pl, hu_pm_ss_total(n, dist), ss.data(), result);
	if(ss_perm) std::copy(ss.begin() + T, ss.end(), ss_perm);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_permanova_design"); }
