// hu_diffabund: the entry and the device path of hmmufotu-amd-diffabund.  The host checks the call, ranks the rows and
// builds the cells (hu_diffabund_host.cpp); the kernels of hu_kern_diffabund.h shuffle the labels of a chunk of permutations, add the
// group sums of every tested OTU, count T >= the observed T and keep the maximum H of every permutation.  The observed labelling runs
// through the same kernels in a launch of its own, so that the observed T and H are the kernel's.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_diffabund.h"

static thread_local double g_daTiming[4] = {0, 0, 0, 0};

#define DCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_diffabund_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_daTiming, sizeof(g_daTiming));
	return HU_OK;
}

static int64_t da_need(const HuDaPlan& pl, int64_t chunk) { return hu_diffabund_need(pl.n, pl.a, (int64_t) pl.row.size(), (int64_t) pl.cell.size(), chunk); }

static int da_nomem(const char* fn, const HuDaPlan& pl, int64_t chunk, size_t freeB) {
	const int64_t c = hu_da_pad(chunk), m = (int64_t) pl.row.size();
	hu_set_error("%s: %lld tested OTUs with %lld cells above 0 and a chunk of %lld permutations need %lld bytes (the cells %lld, the labels %lld, the partial maxima of %lld blocks %lld), %zu bytes are free",
		fn, (long long) m, (long long) pl.cell.size(), (long long) chunk, (long long) da_need(pl, chunk), (long long)(4 * pl.cell.size()), (long long)(pl.n * c),
		(long long) hu_da_blocks(m), (long long)(8 * hu_da_blocks(m) * c), freeB);
	return HU_ERR_NOMEM;
}

/* the chunk of a call under `freeB` bytes: the one asked for, or the largest multiple of 256 that fits (16,384 at the most); 0: none fits */
static int64_t da_chunk(const HuDaPlan& pl, size_t freeB) {
	if(pl.chunk > 0) { const int64_t c = std::min(pl.chunk, pl.perms); return (size_t) da_need(pl, c) <= freeB ? c : 0; }
	int64_t c = std::min<int64_t>(hu_da_pad(pl.perms), HU_DA_MAX_CHUNK);
	while(c > 0 && (size_t) da_need(pl, c) > freeB) c -= HU_DA_WG;
	return std::min(c, pl.perms);
}

static int da_device(const char* fn, int device, const HuDaPlan& pl, uint64_t* tobs, double* hobs, int64_t* count, double* maxstat) {
	g_daTiming[0] = g_daTiming[1] = g_daTiming[2] = g_daTiming[3] = 0;
	const int64_t n = pl.n, m = (int64_t) pl.row.size(), blocks = hu_da_blocks(m), nc = (int64_t) pl.cell.size();
	if(pl.budget > 0) {                                                  /* the caller's budget needs no device to refuse */
		const int64_t c = da_chunk(pl, (size_t) pl.budget);
		if(c == 0) return da_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, (size_t) pl.budget);
	}
	if(blocks > 0x7fffffffll) { hu_set_error("%s: %lld tested OTUs: more blocks than a grid holds", fn, (long long) m); return HU_ERR_ARG; }
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	DCHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	DCHK(hipMemGetInfo(&freeB, &totB));
	if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
	const int64_t chunk = da_chunk(pl, freeB);
	if(chunk == 0) return da_nomem(fn, pl, pl.chunk > 0 ? std::min(pl.chunk, pl.perms) : 1, freeB);
	const int64_t cp = hu_da_pad(chunk);
	if(cp / HU_DA_WG > 65535) { hu_set_error("%s: a chunk of %lld permutations: more than a grid holds", fn, (long long) chunk); return HU_ERR_ARG; }
	uint32_t *dCell = nullptr, *dCount = nullptr; int64_t *dPtr = nullptr, *dSize = nullptr; int32_t *dEz = nullptr, *dDsum = nullptr;
	double *dTc = nullptr, *dHobs = nullptr, *dPart = nullptr, *dMax = nullptr; uint64_t *dW = nullptr, *dTobs = nullptr; uint8_t *dObs = nullptr, *dLab = nullptr;
	HuScope guard([&] { (void) hipFree(dCell); (void) hipFree(dCount); (void) hipFree(dPtr); (void) hipFree(dSize); (void) hipFree(dEz); (void) hipFree(dDsum); (void) hipFree(dTc);
		(void) hipFree(dHobs); (void) hipFree(dPart); (void) hipFree(dMax); (void) hipFree(dW); (void) hipFree(dTobs); (void) hipFree(dObs); (void) hipFree(dLab); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	DCHK(hipMalloc((void**) &dCell, (size_t)(4 * nc))); DCHK(hipMalloc((void**) &dPtr, (size_t)(8 * (m + 1)))); DCHK(hipMalloc((void**) &dEz, (size_t)(4 * m)));
	DCHK(hipMalloc((void**) &dDsum, (size_t)(4 * m))); DCHK(hipMalloc((void**) &dTc, (size_t)(8 * m))); DCHK(hipMalloc((void**) &dTobs, (size_t)(16 * m)));
	DCHK(hipMalloc((void**) &dHobs, (size_t)(8 * m))); DCHK(hipMalloc((void**) &dCount, (size_t)(4 * m))); DCHK(hipMalloc((void**) &dSize, (size_t)(8 * pl.a)));
	DCHK(hipMalloc((void**) &dW, (size_t)(8 * pl.a))); DCHK(hipMalloc((void**) &dObs, (size_t) n)); DCHK(hipMalloc((void**) &dLab, (size_t)(n * cp)));
	DCHK(hipMalloc((void**) &dPart, (size_t)(8 * blocks * cp))); DCHK(hipMalloc((void**) &dMax, (size_t)(8 * cp)));
	DCHK(hipMemcpy(dCell, pl.cell.data(), (size_t)(4 * nc), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dPtr, pl.ptr.data(), (size_t)(8 * (m + 1)), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dEz, pl.ez.data(), (size_t)(4 * m), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dDsum, pl.dsum.data(), (size_t)(4 * m), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dTc, pl.tc.data(), (size_t)(8 * m), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dSize, pl.size.data(), (size_t)(8 * pl.a), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dW, pl.w.data(), (size_t)(8 * pl.a), hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dObs, pl.lab.data(), (size_t) n, hipMemcpyHostToDevice));
	DCHK(hipMemset(dCount, 0, (size_t)(4 * m)));
	const bool two = pl.a == 2;
	const size_t lds = two ? 0 : (size_t) pl.a * HU_DA_WG * 4;                  /* 64 KB at a = 64, and 4 KB of staging: two workgroups on a CU */
	if(!two) DCHK(hipFuncSetAttribute((const void*) k_da_sums<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
	DCHK(hipDeviceSynchronize());
	g_daTiming[0] = since();
	(void) hipGetLastError();
	HuDaDev d;
	d.cell = dCell; d.ptr = dPtr; d.ez = dEz; d.dsum = dDsum; d.tc = dTc; d.size = dSize; d.w = dW; d.lab = dLab; d.tobs = dTobs; d.hobs = dHobs; d.count = dCount;
	d.partmax = dPart; d.m = m; d.cp = cp; d.cnt = 0; d.dL = pl.dL; d.c2 = pl.c2; d.a = (int) pl.a; d.observed = 0;
	std::vector<double> hm((size_t) cp);
	/* one chunk: slots [0, cnt) of it are permutations first .. first + cnt - 1, or (observed) the observed labelling in every slot */
	auto run = [&](int64_t first, int64_t cnt, bool observed) -> int {
		const int64_t c = observed ? HU_DA_WG : hu_da_pad(cnt);             /* whole workgroups of this launch, <= cp */
		double ta = since();
		k_label_shuffle<uint8_t><<<(unsigned)(c / 64), 64>>>(dObs, dLab, n, cp, (uint64_t) first, pl.seed, observed ? 1 : 0);
		DCHK(hipGetLastError());
		DCHK(hipDeviceSynchronize());
		double tb = since();
		g_daTiming[1] += tb - ta;
		d.cnt = cnt; d.observed = observed ? 1 : 0;
		const dim3 grid((unsigned) blocks, (unsigned)(c / HU_DA_WG));
		if(two) k_da_sums<true><<<grid, HU_DA_WG, 0>>>(d);
		else k_da_sums<false><<<grid, HU_DA_WG, lds>>>(d);
		DCHK(hipGetLastError());
		DCHK(hipDeviceSynchronize());
		ta = since();
		g_daTiming[2] += ta - tb;
		if(!observed) {
			k_da_finish<<<(unsigned)(c / 256), 256>>>(dPart, dMax, blocks, cp);
			DCHK(hipGetLastError());
			DCHK(hipMemcpy(hm.data(), dMax, (size_t)(8 * cnt), hipMemcpyDeviceToHost));
		}
		g_daTiming[3] += since() - ta;
		return HU_OK;
	};
	int rc = run(0, 1, true);
	if(rc != HU_OK) return rc;
	for(int64_t first = 0; first < pl.perms; first += chunk) {
		const int64_t cnt = std::min(chunk, pl.perms - first);
		rc = run(first, cnt, false);
		if(rc != HU_OK) return rc;
		std::copy(hm.begin(), hm.begin() + cnt, maxstat + first);
	}
	const double ta = since();
	std::vector<uint32_t> hc((size_t) m);
	DCHK(hipMemcpy(tobs, dTobs, (size_t)(16 * m), hipMemcpyDeviceToHost));
	DCHK(hipMemcpy(hobs, dHobs, (size_t)(8 * m), hipMemcpyDeviceToHost));
	DCHK(hipMemcpy(hc.data(), dCount, (size_t)(4 * m), hipMemcpyDeviceToHost));
	for(int64_t r = 0; r < m; ++r) count[r] = hc[(size_t) r];
	g_daTiming[3] += since() - ta;
	return HU_OK;
}

extern "C" int hu_diffabund(int device, int64_t n_otu, int64_t n_sample, const double* counts, const int32_t* group, const hu_diffabund_opts* opts,
		hu_diffabund_rec* rec_out, double* maxstat_perm_out) try {
	const char* fn = "hu_diffabund";
	if(!rec_out) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuDaPlan pl;
	int rc = hu_da_plan(fn, n_otu, n_sample, counts, group, opts, pl);
	if(rc != HU_OK) return rc;
	const size_t m = pl.row.size();
	std::vector<double> own, hobs(m);
	std::vector<uint64_t> tobs(2 * m);
	std::vector<int64_t> count(m);
	double* mx = maxstat_perm_out;
	if(!mx) { own.resize((size_t) pl.perms); mx = own.data(); }
	if(pl.host || device < 0) hu_da_host_run(pl, tobs.data(), hobs.data(), count.data(), mx);
	else if((rc = da_device(fn, device, pl, tobs.data(), hobs.data(), count.data(), mx)) != HU_OK) return rc;
	hu_da_result(pl, tobs.data(), hobs.data(), count.data(), mx, rec_out);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_diffabund"); }
