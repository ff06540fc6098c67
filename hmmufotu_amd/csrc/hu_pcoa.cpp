// hu_pcoa: the entry and the device's operations of hmmufotu-amd-pcoa.  The host checks the call and runs the block
// iteration (hu_pcoa_host.cpp); here its six operations are launches of the kernels of hu_kern_pcoa.h.  The matrix goes up once and is
// squared in place; after that only m x m matrices cross the bus until the final block comes back.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>
#include "hu_common.h"
#include "hu_permanova.h"
#include "hu_kern_pcoa.h"

#define PCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)
/* one instantiation per padded width */
#define PC_NT(nt, stmt) do { switch(nt) { case 1: { constexpr int NT = 1; stmt; } break; case 2: { constexpr int NT = 2; stmt; } break; \
	case 3: { constexpr int NT = 3; stmt; } break; default: { constexpr int NT = 4; stmt; } break; } } while(0)

namespace {
struct DevOps : HuPcOps {
	const char* fn; const HuPcPlan& pl; const double* dist;
	int64_t n, S, L, chunks, m = 0, mp = 0;
	size_t freeB = 0;
	double *dD2 = nullptr, *dPart = nullptr, *dBlk[4] = {nullptr, nullptr, nullptr, nullptr}, *dGpart = nullptr, *dG = nullptr, *dM1 = nullptr, *dM2 = nullptr, *dCol = nullptr;
	double* tm = hu_pc_timing_slots();
	std::chrono::steady_clock::time_point t0;

	DevOps(const char* fn_, const HuPcPlan& pl_, const double* dist_) : fn(fn_), pl(pl_), dist(dist_), n(pl_.n), S(hu_pc_slabs(pl_.n)), L(hu_pc_slab_len(pl_.n)), chunks(hu_pc_chunks(pl_.n)) {}
	void small_free() {
		(void) hipFree(dPart); (void) hipFree(dGpart); (void) hipFree(dG); (void) hipFree(dM1); (void) hipFree(dM2); (void) hipFree(dCol);
		for(auto& b : dBlk) { (void) hipFree(b); b = nullptr; }
		dPart = dGpart = dG = dM1 = dM2 = dCol = nullptr;
	}
	~DevOps() override { small_free(); (void) hipFree(dD2); }
	void tick() { t0 = std::chrono::steady_clock::now(); }
	/* waits for the device and adds the time since tick() to slot `slot` */
	int tock(int slot) {
		PCHK(hipGetLastError());
		PCHK(hipDeviceSynchronize());
		tm[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		return HU_OK;
	}
	int nomem(int64_t m_, size_t have) {
		hu_set_error("%s: %lld samples and a block of %lld columns need %lld bytes of device memory (the squares %lld), %zu bytes are free", fn, (long long) n, (long long) m_,
			(long long) hu_pc_need_m(n, m_), (long long)(8 * n * n), have);
		return HU_ERR_NOMEM;
	}
	int open(int device) {
		PCHK(hipSetDevice(device));
		size_t totB = 0;
		PCHK(hipMemGetInfo(&freeB, &totB));
		if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
		return HU_OK;
	}
	int setup(int64_t m_, const double* start, int dst) override {
		if((size_t) hu_pc_need_m(n, m_) > freeB) return nomem(m_, freeB);
		int rc;
		if(!dD2) {
			tick();
			PCHK(hipMalloc((void**) &dD2, (size_t)(8 * n * n)));
			PCHK(hipMemcpy(dD2, dist, (size_t)(8 * n * n), hipMemcpyHostToDevice));
			if((rc = tock(0)) != HU_OK) return rc;
			tick();
			k_pcoa_square<<<(unsigned) std::min<int64_t>((n * n + 255) / 256, 1 << 20), 256>>>(dD2, n * n);
			if((rc = tock(1)) != HU_OK) return rc;
		}
		tick();
		small_free();
		m = m_; mp = hu_pc_pad(m);
		const size_t blk = (size_t)(8 * n * mp), sq = (size_t)(8 * mp * mp);
		PCHK(hipMalloc((void**) &dPart, (size_t) S * blk));
		for(auto& b : dBlk) PCHK(hipMalloc((void**) &b, blk));
		PCHK(hipMalloc((void**) &dGpart, (size_t) chunks * sq)); PCHK(hipMalloc((void**) &dG, sq)); PCHK(hipMalloc((void**) &dM1, sq)); PCHK(hipMalloc((void**) &dM2, sq));
		PCHK(hipMalloc((void**) &dCol, (size_t)(8 * chunks * mp)));
		PCHK(hipMemcpy(dBlk[dst], start, blk, hipMemcpyHostToDevice));
		return tock(0);
	}
	/* dst = scale * J (sum of the S slabs of part) */
	int finish(const double* part, int64_t slabs, double scale, int dst) {
		k_pcoa_colsum<<<(unsigned) chunks, 256>>>(part, slabs, n, (int) mp, dCol);
		k_pcoa_finish<<<(unsigned)((n * mp + 255) / 256), 256>>>(part, slabs, n, (int) mp, dCol, chunks, scale, dBlk[dst]);
		return tock(3);
	}
	int bv(int src, int dst) override {
		tick();
		const dim3 grid((unsigned)((n + HU_PCOA_TILE - 1) / HU_PCOA_TILE), (unsigned) S);
		PC_NT(mp / 16, (k_pcoa_d2v<NT><<<grid, 256>>>(dD2, dBlk[src], dPart, n, L)));
		const int rc = tock(2);
		if(rc != HU_OK) return rc;
		tick();
		return finish(dPart, S, -0.5, dst);
	}
	int centre(int src, int dst) override { tick(); return finish(dBlk[src], 1, 1.0, dst); }
	int gram(int x, int y, double* G) override {
		tick();
		PC_NT(mp / 16, (k_pcoa_gram<NT><<<(unsigned) chunks, 256>>>(dBlk[x], dBlk[y], n, dGpart)));
		k_pcoa_gram_sum<<<(unsigned)((mp * mp + 255) / 256), 256>>>(dGpart, chunks, (int)(mp * mp), dG);
		PCHK(hipGetLastError());
		PCHK(hipMemcpy(G, dG, (size_t)(8 * mp * mp), hipMemcpyDeviceToHost));
		return tock(3);
	}
	int apply(int x, const double* M1, int y, const double* M2, int dst) override {
		tick();
		PCHK(hipMemcpy(dM1, M1, (size_t)(8 * mp * mp), hipMemcpyHostToDevice));
		if(y >= 0) PCHK(hipMemcpy(dM2, M2, (size_t)(8 * mp * mp), hipMemcpyHostToDevice));
		const unsigned grid = (unsigned)((n * mp + 255) / 256);
		if(y >= 0) PC_NT(mp / 16, (k_pcoa_apply<NT, true><<<grid, 256>>>(dBlk[x], dM1, dBlk[y], dM2, dBlk[dst], n)));
		else PC_NT(mp / 16, (k_pcoa_apply<NT, false><<<grid, 256>>>(dBlk[x], dM1, nullptr, nullptr, dBlk[dst], n)));
		return tock(3);
	}
	int fetch(int src, double* out) override {
		tick();
		PCHK(hipMemcpy(out, dBlk[src], (size_t)(8 * n * mp), hipMemcpyDeviceToHost));
		return tock(5);
	}
};
}

extern "C" int hu_pcoa(int device, int64_t n, const double* dist, const hu_pcoa_opts* opts, hu_pcoa_result* out, double* coords, double* eigval, double* resid) try {
	const char* fn = "hu_pcoa";
	if(!out || !coords || !eigval || !resid) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuPcPlan pl;
	int rc = hu_pc_plan(fn, n, dist, opts, pl);
	if(rc != HU_OK) return rc;
	memset(out, 0, sizeof(*out));
	std::fill(hu_pc_timing_slots(), hu_pc_timing_slots() + 6, 0.0);
	const double trace = hu_pm_ss_total(n, dist);
	if(pl.host || device < 0) {
		std::unique_ptr<HuPcOps> ops(hu_pc_host_ops(n, dist));
		return hu_pc_run(fn, *ops, pl, trace, out, coords, eigval, resid);
	}
	DevOps ops(fn, pl, dist);
	const int64_t m0 = std::min(pl.k + pl.oversample, n - 1);
	if(pl.budget > 0 && hu_pc_need_m(n, m0) > pl.budget) return ops.nomem(m0, (size_t) pl.budget);       /* the caller's budget needs no device to refuse */
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	if((rc = ops.open(device)) != HU_OK) return rc;
	return hu_pc_run(fn, ops, pl, trace, out, coords, eigval, resid);
} catch(...) { return hu_catch_all("hu_pcoa"); }
