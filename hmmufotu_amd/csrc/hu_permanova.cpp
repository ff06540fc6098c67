// hu_permanova: the entry and the device path of hmmufotu-amd-permanova.  The host checks the call and computes SS_T
// (hu_permanova_host.cpp); the kernels of hu_kern_permanova.h shuffle the labels of a chunk of permutations and add the within-group
// squares.  The observed labelling runs through the same kernels in a launch of its own, so that its bits are the kernel's.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_permanova.h"

static thread_local double g_pmTiming[4] = {0, 0, 0, 0};

#define PCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_permanova_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_pmTiming, sizeof(g_pmTiming));
	return HU_OK;
}

static int pm_nomem(const char* fn, const HuPmPlan& pl, int64_t chunk, size_t freeB) {
	const int64_t c = hu_pm_pad(chunk);
	hu_set_error("%s: %lld samples and a chunk of %lld permutations need %lld bytes of device memory (the matrix %lld, the labels %lld, the partial sums of %lld tiles %lld), %zu bytes are free",
		fn, (long long) pl.n, (long long) chunk, (long long) hu_permanova_need(pl.n, pl.a, chunk), (long long)(8 * pl.n * pl.n), (long long)(2 * pl.n * c),
		(long long) hu_pm_tiles(pl.n), (long long)(8 * hu_pm_tiles(pl.n) * c), freeB);
	return HU_ERR_NOMEM;
}

/* the chunk of a call under `freeB` bytes: the one asked for, or the largest multiple of 256 that fits (16,384 at the most); 0: none fits */
static int64_t pm_chunk(const HuPmPlan& pl, size_t freeB) {
	if(pl.chunk > 0) { const int64_t c = std::min(pl.chunk, pl.perms); return (size_t) hu_permanova_need(pl.n, pl.a, c) <= freeB ? c : 0; }
	int64_t c = std::min<int64_t>(hu_pm_pad(pl.perms), HU_PM_MAX_CHUNK);
	while(c > 0 && (size_t) hu_permanova_need(pl.n, pl.a, c) > freeB) c -= HU_PM_WG;
	return std::min(c, pl.perms);
}

static int pm_device(const char* fn, int device, const HuPmPlan& pl, const double* dist, double* obs, double* ssw) {
	g_pmTiming[0] = g_pmTiming[1] = g_pmTiming[2] = g_pmTiming[3] = 0;
	const int64_t n = pl.n, tiles = hu_pm_tiles(n);
	if(pl.budget > 0) {                                                  /* the caller's budget needs no device to refuse */
		const int64_t c = pm_chunk(pl, (size_t) pl.budget);
		if(c == 0) return pm_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, (size_t) pl.budget);
	}
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	PCHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	PCHK(hipMemGetInfo(&freeB, &totB));
	if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
	const int64_t chunk = pm_chunk(pl, freeB);
	if(chunk == 0) return pm_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, freeB);
	const int64_t cp = hu_pm_pad(chunk);
	if(cp / HU_PM_WG > 65535) { hu_set_error("%s: a chunk of %lld permutations: more than a grid holds", fn, (long long) chunk); return HU_ERR_ARG; }
	double *dDist = nullptr, *dInv = nullptr, *dPart = nullptr, *dSsw = nullptr;
	uint16_t *dObs = nullptr, *dLab = nullptr;
	HuScope guard([&] { (void) hipFree(dDist); (void) hipFree(dInv); (void) hipFree(dPart); (void) hipFree(dSsw); (void) hipFree(dObs); (void) hipFree(dLab); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	PCHK(hipMalloc((void**) &dDist, (size_t)(8 * n * n))); PCHK(hipMalloc((void**) &dInv, (size_t)(8 * pl.a))); PCHK(hipMalloc((void**) &dObs, (size_t)(2 * n)));
	PCHK(hipMalloc((void**) &dLab, (size_t)(2 * n * cp))); PCHK(hipMalloc((void**) &dPart, (size_t)(8 * tiles * cp)));
	PCHK(hipMalloc((void**) &dSsw, (size_t)(8 * cp)));
	PCHK(hipMemcpy(dDist, dist, (size_t)(8 * n * n), hipMemcpyHostToDevice));
	PCHK(hipMemcpy(dInv, pl.inv.data(), (size_t)(8 * pl.a), hipMemcpyHostToDevice));
	PCHK(hipMemcpy(dObs, pl.lab.data(), (size_t)(2 * n), hipMemcpyHostToDevice));
	const bool bytes = pl.a <= 256;                                      /* labels as bytes in LDS: two workgroups on a CU */
	if(!bytes) PCHK(hipFuncSetAttribute((const void*) k_permanova_pairs<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) HU_PM_LDS(16)));
	PCHK(hipDeviceSynchronize());
	g_pmTiming[0] = since();
	(void) hipGetLastError();
	std::vector<double> hs((size_t) cp);
	/* one chunk: slots [0, cnt) of it are permutations first .. first + cnt - 1, or (observed) the observed labelling in every slot */
	auto run = [&](int64_t first, int64_t cnt, bool observed) -> int {
		const int64_t c = observed ? HU_PM_WG : hu_pm_pad(cnt);             /* whole workgroups of this launch, <= cp */
		double ta = since();
		k_label_shuffle<uint16_t><<<(unsigned)(c / 64), 64>>>(dObs, dLab, n, c, (uint64_t) first, pl.seed, observed ? 1 : 0);
		PCHK(hipGetLastError());
		PCHK(hipDeviceSynchronize());
		double tb = since();
		g_pmTiming[1] += tb - ta;
		const dim3 grid((unsigned) tiles, (unsigned)(c / HU_PM_WG));
		if(bytes) k_permanova_pairs<8><<<grid, HU_PM_WG, HU_PM_LDS(8)>>>(dDist, dLab, dInv, dPart, n, c);
		else k_permanova_pairs<16><<<grid, HU_PM_WG, HU_PM_LDS(16)>>>(dDist, dLab, dInv, dPart, n, c);
		PCHK(hipGetLastError());
		PCHK(hipDeviceSynchronize());
		ta = since();
		g_pmTiming[2] += ta - tb;
		k_permanova_finish<<<(unsigned)(c / 256), 256>>>(dPart, dSsw, tiles, c);
		PCHK(hipGetLastError());
		PCHK(hipMemcpy(hs.data(), dSsw, (size_t)(8 * cnt), hipMemcpyDeviceToHost));
		g_pmTiming[3] += since() - ta;
		return HU_OK;
	};
	int rc = run(0, 1, true);
	if(rc != HU_OK) return rc;
	*obs = hs[0];
	for(int64_t first = 0; first < pl.perms; first += chunk) {
		const int64_t cnt = std::min(chunk, pl.perms - first);
		rc = run(first, cnt, false);
		if(rc != HU_OK) return rc;
		std::copy(hs.begin(), hs.begin() + cnt, ssw + first);
	}
	return HU_OK;
}

extern "C" int hu_permanova(int device, int64_t n, const double* dist, const int32_t* group, const hu_permanova_opts* opts, hu_permanova_result* out,
		double* ssw_perm) try {
	const char* fn = "hu_permanova";
	if(!out) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuPmPlan pl;
	int rc = hu_pm_plan(fn, n, dist, group, opts, pl);
	if(rc != HU_OK) return rc;
	std::vector<double> own;
	double* ssw = ssw_perm;
	if(!ssw) { own.resize((size_t) pl.perms); ssw = own.data(); }
	double obs = 0.0;
	if(pl.host || device < 0) hu_pm_host_run(pl, dist, &obs, ssw);
	else if((rc = pm_device(fn, device, pl, dist, &obs, ssw)) != HU_OK) return rc;
	hu_pm_result(pl, hu_pm_ss_total(n, dist), obs, ssw, out);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_permanova"); }
