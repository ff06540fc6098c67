// hu_alpha: the entry, and the device path of hmmufotu-amd-alpha.  The host makes the plan (hu_alpha_host.cpp: every
// sample's nonzero cells, their prefixes in table order and their places in the depth-first row order of hu_unifrac's embedding, the
// branch entries, the list of draws); the prefixes, the places and the entries go up once and stay; the draws are taken `cap` at a time through the kernels of hu_kern_draw.h and hu_kern_alpha.h, and 40
// bytes per draw come back.  The number of launches per chunk of draws does not depend on the table.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_alpha.h"

static thread_local double g_alTiming[6] = {0, 0, 0, 0, 0, 0};

#define ACHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_alpha_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_alTiming, sizeof(g_alTiming));
	return HU_OK;
}

static int al_device(const char* fn, int device, const HuAlPlan& pl, std::vector<HuAlStat>& stat) {
	const size_t U = pl.unit.size(), S = (size_t) pl.S;
	const int64_t want = pl.drawChunk > 0 ? std::min<int64_t>(pl.drawChunk, (int64_t) U) : 1;
	const int64_t need0 = hu_al_need_of(pl, want);
	if(pl.budget > 0 && need0 > pl.budget) {
		hu_set_error("%s: %lld resident draw(s) of %lld samples need %lld bytes of device memory, the budget is %lld bytes", fn, (long long) want, (long long) S, (long long) need0, (long long) pl.budget);
		return HU_ERR_NOMEM;
	}
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	ACHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	ACHK(hipMemGetInfo(&freeB, &totB));
	if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
	if((size_t) need0 > freeB) {
		hu_set_error("%s: %lld resident draw(s) of %lld samples need %lld bytes of device memory, %zu bytes are free", fn, (long long) want, (long long) S, (long long) need0, freeB);
		return HU_ERR_NOMEM;
	}
	/* the draws resident at once: what was asked for, or what the memory holds; a grid holds 2^31 - 1 chunks */
	const int64_t perDraw = 1136 + 4 * pl.maxNnz + 24 * pl.maxChunk;
	int64_t cap = want;
	if(pl.drawChunk == 0) cap = std::min<int64_t>((int64_t) U, ((int64_t) freeB - hu_al_need_of(pl, 0)) / perDraw);
	cap = std::max<int64_t>(1, std::min<int64_t>(cap, 0x7fffffffll / std::max<int64_t>(1, pl.maxChunk)));
	const size_t D = (size_t) cap, mc = (size_t) pl.maxChunk, mn = (size_t) pl.maxNnz;

	HuAlSample* dSmp = nullptr; HuAlBranch* dBr = nullptr; HuAlDraw* dDraw = nullptr; HuAlGroup* dGrp = nullptr; HuAlChunk* dChunk = nullptr; HuAlSel* dSel = nullptr;
	HuAlStat* dStat = nullptr; uint32_t *dPrefix = nullptr, *dSlot = nullptr, *dOut = nullptr, *dHist = nullptr, *dTie = nullptr;
	HuScope guard([&] { (void) hipFree(dSmp); (void) hipFree(dBr); (void) hipFree(dDraw); (void) hipFree(dGrp); (void) hipFree(dChunk); (void) hipFree(dSel); (void) hipFree(dStat);
		(void) hipFree(dPrefix); (void) hipFree(dSlot); (void) hipFree(dOut); (void) hipFree(dHist); (void) hipFree(dTie); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	double mark = 0;
	auto phase = [&](int p) { const double now = since(); g_alTiming[p] += now - mark; mark = now; };
	ACHK(hipMalloc((void**) &dSmp, S * sizeof(HuAlSample))); ACHK(hipMalloc((void**) &dPrefix, pl.prefix.size() * 4)); ACHK(hipMalloc((void**) &dSlot, pl.slot.size() * 4));
	ACHK(hipMalloc((void**) &dBr, std::max<size_t>(pl.br.size(), 1) * sizeof(HuAlBranch)));
	ACHK(hipMalloc((void**) &dDraw, D * sizeof(HuAlDraw))); ACHK(hipMalloc((void**) &dGrp, D * sizeof(HuAlGroup))); ACHK(hipMalloc((void**) &dSel, D * sizeof(HuAlSel)));
	ACHK(hipMalloc((void**) &dStat, D * sizeof(HuAlStat))); ACHK(hipMalloc((void**) &dHist, D * 256 * 4)); ACHK(hipMalloc((void**) &dOut, D * mn * 4));
	ACHK(hipMalloc((void**) &dTie, D * mc * HU_AL_WAVES * 4)); ACHK(hipMalloc((void**) &dChunk, D * mc * sizeof(HuAlChunk)));
	ACHK(hipMemcpy(dSmp, pl.smp.data(), S * sizeof(HuAlSample), hipMemcpyHostToDevice));
	ACHK(hipMemcpy(dPrefix, pl.prefix.data(), pl.prefix.size() * 4, hipMemcpyHostToDevice));
	ACHK(hipMemcpy(dSlot, pl.slot.data(), pl.slot.size() * 4, hipMemcpyHostToDevice));
	if(!pl.br.empty()) ACHK(hipMemcpy(dBr, pl.br.data(), pl.br.size() * sizeof(HuAlBranch), hipMemcpyHostToDevice));
	ACHK(hipMemset(dHist, 0, D * 256 * 4));
	(void) hipGetLastError();

	stat.resize(U);
	std::vector<HuAlDraw> draw; std::vector<HuAlGroup> grp; std::vector<HuAlChunk> chunk; std::vector<HuAlSel> sel;
	const uint64_t perChunk = (uint64_t) pl.chunk;
	for(size_t u0 = 0; u0 < U; u0 += D) {
		const size_t n = std::min(D, U - u0);
		draw.assign(n, HuAlDraw{0, 0, 0, 0}); sel.assign(n, HuAlSel{0, 0, 0}); grp.clear(); chunk.clear();
		uint64_t cells = 0, ties = 0;
		uint32_t maxNd = 0;
		for(size_t a = 0; a < n; ++a) {
			const HuAlUnit& un = pl.unit[u0 + a];
			const HuAlSample& s = pl.smp[(size_t) un.smp];
			draw[a] = HuAlDraw{cells, ties, (uint32_t) un.smp, un.depth < 0 ? 0u : (uint32_t) pl.depth[(size_t) un.depth]};
			cells += s.nnz;
			if(un.depth < 0) continue;
			ties += (s.T + perChunk - 1) / perChunk * HU_DRAW_WAVES;
			sel[a] = HuAlSel{0, draw[a].m, s.T};
			const bool cont = a > 0 && pl.unit[u0 + a - 1].depth >= 0 && pl.unit[u0 + a - 1].smp == un.smp && pl.unit[u0 + a - 1].rep == un.rep;
			if(cont) ++grp.back().nd;
			else hu_draw_add_group(grp, chunk, (uint32_t) un.smp, pl.seed + (uint64_t) un.rep, (uint32_t) a, 1u, s.T, perChunk);
			maxNd = std::max(maxNd, grp.back().nd);
		}
		ACHK(hipMemcpy(dDraw, draw.data(), n * sizeof(HuAlDraw), hipMemcpyHostToDevice));
		ACHK(hipMemcpy(dSel, sel.data(), n * sizeof(HuAlSel), hipMemcpyHostToDevice));
		if(!grp.empty()) {
			ACHK(hipMemcpy(dGrp, grp.data(), grp.size() * sizeof(HuAlGroup), hipMemcpyHostToDevice));
			ACHK(hipMemcpy(dChunk, chunk.data(), chunk.size() * sizeof(HuAlChunk), hipMemcpyHostToDevice));
		}
		ACHK(hipMemset(dOut, 0, (size_t) cells * 4));
		ACHK(hipDeviceSynchronize());
		phase(0);
		const HuDrawDev dv = {dSmp, dDraw, dGrp, dChunk, dSel, dHist, dTie, dPrefix, dSlot, dOut, pl.keyBits, pl.chunk};
		ACHK(hu_draw_select<HU_AL_DT>(dv, (unsigned) n, (unsigned) chunk.size(), maxNd));
		ACHK(hipDeviceSynchronize());
		phase(1);
		k_al_whole<<<(unsigned) n, HU_AL_WG>>>(dSmp, dDraw, dPrefix, dSlot, dOut);
		ACHK(hipGetLastError());
		ACHK(hu_draw_take<HU_AL_DT>(dv, (unsigned) chunk.size(), maxNd));
		ACHK(hipDeviceSynchronize());
		phase(2);
		k_al_stats<<<(unsigned) n, HU_AL_WG>>>(dSmp, dDraw, dOut, dStat);
		ACHK(hipGetLastError());
		ACHK(hipDeviceSynchronize());
		phase(3);
		if(pl.hasTree) {
			k_al_pd<<<(unsigned) n, HU_AL_WG>>>(dSmp, dBr, dDraw, dOut, dStat);
			ACHK(hipGetLastError());
			ACHK(hipDeviceSynchronize());
			phase(4);
		}
		ACHK(hipMemcpy(stat.data() + u0, dStat, n * sizeof(HuAlStat), hipMemcpyDeviceToHost));
		phase(5);
	}
	return HU_OK;
}

extern "C" int hu_alpha(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, uint64_t seed, const hu_alpha_opts* opts, hu_alpha_rec* whole_out, hu_alpha_rec* draws_out) try {
	const char* fn = "hu_alpha";
	if(!whole_out || (!draws_out && n_depth > 0 && reps > 0)) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuAlPlan pl;
	const int rc = hu_al_plan(fn, tree, n_otu, n_sample, otu_node, counts, n_depth, depths, reps, seed, opts, pl);
	if(rc != HU_OK) return rc;
	std::vector<HuAlStat> stat;
	if(pl.host || device < 0) hu_al_host(pl, stat);
	else {
		for(double& s : g_alTiming) s = 0;
		const int rd = al_device(fn, device, pl, stat);
		if(rd != HU_OK) return rd;
	}
	hu_al_fill(pl, stat, whole_out, draws_out);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_alpha"); }
