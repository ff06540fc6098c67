// hu_unifrac_rarefied: the entry, and the device path of hmmufotu-amd-unifrac --rarefy.  The host makes the plan
// (hu_unifrac_rarefied_host.cpp) and the lists of one chunk of resident draws; the table goes up once and stays; per chunk the kernels of
// hu_kern_draw.h draw, those of hu_kern_unifrac_rarefied.h embed, add the pairs and take the recurrence's steps.  The lists of a chunk
// are the same for every chunk but for the keys, which a kernel sets: the host only launches.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_unifrac_rarefied.h"

static thread_local double g_urTiming[6] = {0, 0, 0, 0, 0, 0};
static thread_local int64_t g_urResident = 0;

#define RCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_unifrac_rarefied_timing(double* seconds, int64_t* resident_draws) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_urTiming, sizeof(g_urTiming));
	if(resident_draws) *resident_draws = g_urResident;
	return HU_OK;
}

static int ur_device(const char* fn, int device, const HuUrPlan& pl, double* mean, double* m2, double* draws) {
	const HuAlPlan& al = pl.al;
	const size_t S = (size_t) pl.nSample, Sk = (size_t) pl.Sk, B = (size_t) pl.uf.B, R = (size_t) pl.reps;
	const size_t Sp = (Sk + HU_UF_TILE - 1) / HU_UF_TILE * HU_UF_TILE, tiles = (size_t) hu_uf_tiles(pl.Sk), nSlab = (size_t) pl.uf.nSlab;
	const bool wantDraws = draws != nullptr;
	if(tiles > 0x7fffffffull) { hu_set_error("%s: %zu tiles: more than a grid holds", fn, tiles); return HU_ERR_ARG; }
	const int64_t want = pl.drawChunk > 0 ? std::min<int64_t>(pl.drawChunk, pl.reps) : 1;
	const int64_t need0 = hu_ur_need_of(pl, want, wantDraws);
	if(pl.budget > 0 && need0 > pl.budget) {
		hu_set_error("%s: %lld resident draw(s) of %zu kept samples and %zu branches need %lld bytes of device memory, the budget is %lld bytes", fn, (long long) want, Sk, B,
			(long long) need0, (long long) pl.budget);
		return HU_ERR_NOMEM;
	}
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	RCHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	RCHK(hipMemGetInfo(&freeB, &totB));
	if(pl.budget > 0 && (size_t) pl.budget < freeB) freeB = (size_t) pl.budget;
	if((size_t) need0 > freeB) {
		hu_set_error("%s: %lld resident draw(s) of %zu kept samples and %zu branches need %lld bytes of device memory, %zu bytes are free", fn, (long long) want, Sk, B,
			(long long) need0, freeB);
		return HU_ERR_NOMEM;
	}
	/* the lists of one resident draw: its units (kept samples), groups (the samples that are drawn, not taken whole) and chunks of reads */
	const uint64_t perChunk = (uint64_t) al.chunk;
	uint64_t cells1 = 0, ties1 = 0, chunks1 = 0, grp1 = 0;
	for(size_t a = 0; a < Sk; ++a) {
		const HuAlSample& s = al.smp[(size_t) pl.keptCol[a]];
		cells1 += s.nnz;
		if((uint64_t) s.T != pl.depth) { const uint64_t nc = (s.T + perChunk - 1) / perChunk; ties1 += nc * HU_AL_WAVES; chunks1 += nc; ++grp1; }
	}
	/* the draws resident at once: what was asked for, or what the memory holds; the grids hold 2^31 - 1 chunks and units and 65535 draws */
	int64_t cap = want;
	if(pl.drawChunk == 0) {
		const int64_t fixed = hu_ur_need_of(pl, 0, wantDraws), per = hu_ur_need_of(pl, 1, wantDraws) - fixed;
		cap = std::min<int64_t>(pl.reps, ((int64_t) freeB - fixed) / per);
	}
	cap = std::min<int64_t>(cap, 65535);
	cap = std::min<int64_t>(cap, 0x7fffffffll / (int64_t) std::max<uint64_t>(1, std::max<uint64_t>(chunks1, Sk)));
	cap = std::max<int64_t>(1, cap);
	const size_t D = (size_t) cap, U = D * Sk;
	g_urResident = cap;

	std::vector<HuAlDraw> draw(U); std::vector<HuAlGroup> grp; std::vector<HuAlChunk> chunk;
	grp.reserve(D * grp1); chunk.reserve(D * chunks1);
	{
		uint64_t cells = 0, ties = 0;
		for(size_t z = 0; z < D; ++z) for(size_t a = 0; a < Sk; ++a) {
			const uint32_t col = (uint32_t) pl.keptCol[a];
			const HuAlSample& s = al.smp[col];
			const bool whole = (uint64_t) s.T == pl.depth;
			draw[z * Sk + a] = HuAlDraw{cells, ties, col, whole ? 0u : (uint32_t) pl.depth};
			cells += s.nnz;
			if(whole) continue;
			ties += (s.T + perChunk - 1) / perChunk * HU_DRAW_WAVES;
			hu_draw_add_group(grp, chunk, col, 0, (uint32_t)(z * Sk + a), 1u, s.T, perChunk);   /* the key: k_ur_reset's */
		}
	}

	HuAlSample* dSmp = nullptr; HuAlBranch* dBr = nullptr; HuAlDraw* dDraw = nullptr; HuAlGroup* dGrp = nullptr; HuAlChunk* dChunk = nullptr; HuAlSel* dSel = nullptr;
	uint32_t *dPrefix = nullptr, *dSlot = nullptr, *dBrK = nullptr, *dOut = nullptr, *dHist = nullptr, *dTie = nullptr;
	double *dLen = nullptr, *dP = nullptr, *dPart = nullptr, *dMean = nullptr, *dM2 = nullptr, *dD = nullptr;
	HuScope guard([&] { (void) hipFree(dSmp); (void) hipFree(dBr); (void) hipFree(dDraw); (void) hipFree(dGrp); (void) hipFree(dChunk); (void) hipFree(dSel);
		(void) hipFree(dPrefix); (void) hipFree(dSlot); (void) hipFree(dBrK); (void) hipFree(dOut); (void) hipFree(dHist); (void) hipFree(dTie);
		(void) hipFree(dLen); (void) hipFree(dP); (void) hipFree(dPart); (void) hipFree(dMean); (void) hipFree(dM2); (void) hipFree(dD); });
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	double mark = 0;
	auto phase = [&](int p) { const double now = since(); g_urTiming[p] += now - mark; mark = now; };
	const size_t one = 1, bP1 = B * Sp * 8, bPart1 = nSlab * tiles * 2 * HU_UF_TILE * HU_UF_TILE * 8, bD1 = Sk * Sk * 8;
	RCHK(hipMalloc((void**) &dSmp, S * sizeof(HuAlSample))); RCHK(hipMalloc((void**) &dPrefix, al.prefix.size() * 4)); RCHK(hipMalloc((void**) &dSlot, std::max(al.slot.size(), one) * 4));
	RCHK(hipMalloc((void**) &dBr, std::max(al.br.size(), one) * sizeof(HuAlBranch))); RCHK(hipMalloc((void**) &dBrK, std::max(al.brK.size(), one) * 4));
	RCHK(hipMalloc((void**) &dLen, B * 8));
	RCHK(hipMalloc((void**) &dDraw, U * sizeof(HuAlDraw))); RCHK(hipMalloc((void**) &dGrp, U * sizeof(HuAlGroup))); RCHK(hipMalloc((void**) &dSel, U * sizeof(HuAlSel)));
	RCHK(hipMalloc((void**) &dHist, U * 256 * 4)); RCHK(hipMalloc((void**) &dOut, std::max<size_t>(D * cells1, one) * 4));
	RCHK(hipMalloc((void**) &dTie, std::max<size_t>(D * ties1, one) * 4)); RCHK(hipMalloc((void**) &dChunk, std::max<size_t>(D * chunks1, one) * sizeof(HuAlChunk)));
	RCHK(hipMalloc((void**) &dP, D * bP1)); RCHK(hipMalloc((void**) &dPart, D * bPart1));
	RCHK(hipMalloc((void**) &dMean, bD1)); RCHK(hipMalloc((void**) &dM2, bD1));
	if(wantDraws) RCHK(hipMalloc((void**) &dD, D * bD1));
	RCHK(hipMemcpy(dSmp, al.smp.data(), S * sizeof(HuAlSample), hipMemcpyHostToDevice));
	RCHK(hipMemcpy(dPrefix, al.prefix.data(), al.prefix.size() * 4, hipMemcpyHostToDevice));
	if(!al.slot.empty()) RCHK(hipMemcpy(dSlot, al.slot.data(), al.slot.size() * 4, hipMemcpyHostToDevice));
	if(!al.br.empty()) {
		RCHK(hipMemcpy(dBr, al.br.data(), al.br.size() * sizeof(HuAlBranch), hipMemcpyHostToDevice));
		RCHK(hipMemcpy(dBrK, al.brK.data(), al.brK.size() * 4, hipMemcpyHostToDevice));
	}
	RCHK(hipMemcpy(dLen, pl.uf.b.data(), B * 8, hipMemcpyHostToDevice));
	RCHK(hipMemcpy(dDraw, draw.data(), U * sizeof(HuAlDraw), hipMemcpyHostToDevice));
	if(!grp.empty()) {
		RCHK(hipMemcpy(dGrp, grp.data(), grp.size() * sizeof(HuAlGroup), hipMemcpyHostToDevice));
		RCHK(hipMemcpy(dChunk, chunk.data(), chunk.size() * sizeof(HuAlChunk), hipMemcpyHostToDevice));
	}
	RCHK(hipMemset(dHist, 0, U * 256 * 4));
	RCHK(hipMemset(dSel, 0, U * sizeof(HuAlSel)));
	RCHK(hipDeviceSynchronize());
	phase(0);
	(void) hipGetLastError();

	const HuDrawDev dv = {dSmp, dDraw, dGrp, dChunk, dSel, dHist, dTie, dPrefix, dSlot, dOut, al.keyBits, al.chunk};
	const int raw = pl.uf.method == HU_UF_WEIGHTED_RAW;
	for(size_t r0 = 0; r0 < R; r0 += D) {
		const size_t n = std::min(D, R - r0), nu = n * Sk, ng = n * (size_t) grp1, nc = n * (size_t) chunks1;
		RCHK(hipMemset(dOut, 0, std::max<size_t>(n * cells1, one) * 4));
		k_ur_reset<<<(unsigned)((nu + HU_AL_WG - 1) / HU_AL_WG), HU_AL_WG>>>(dSmp, dDraw, dSel, dGrp, (uint32_t) nu, (uint32_t) ng, (uint32_t) std::max<uint64_t>(grp1, 1), pl.seed + (uint64_t) r0);
		RCHK(hipGetLastError());
		/* every group is one draw: the kernels that hold one depth */
		RCHK(hu_draw_select<1>(dv, (unsigned) nu, (unsigned) nc, 1));
		k_al_whole<<<(unsigned) nu, HU_AL_WG>>>(dSmp, dDraw, dPrefix, dSlot, dOut);
		RCHK(hipGetLastError());
		RCHK(hu_draw_take<1>(dv, (unsigned) nc, 1));
		RCHK(hipDeviceSynchronize());
		phase(1);
		RCHK(hipMemset(dP, 0, n * bP1));
		k_ur_embed<<<(unsigned) nu, HU_AL_WG>>>(dSmp, dBr, dBrK, dDraw, dOut, dP, (uint32_t) Sk, (int64_t) Sp, (int64_t) B, (double) pl.depth);
		RCHK(hipGetLastError());
		RCHK(hipDeviceSynchronize());
		phase(2);
		const dim3 pg((unsigned) tiles, (unsigned) nSlab, (unsigned) n);
		switch(pl.uf.method) {
		case HU_UF_UNWEIGHTED: k_ur_pairs<HU_UF_UNWEIGHTED><<<pg, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.uf.L, pl.uf.alpha); break;
		case HU_UF_WEIGHTED: k_ur_pairs<HU_UF_WEIGHTED><<<pg, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.uf.L, pl.uf.alpha); break;
		case HU_UF_WEIGHTED_RAW: k_ur_pairs<HU_UF_WEIGHTED_RAW><<<pg, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.uf.L, pl.uf.alpha); break;
		default: k_ur_pairs<HU_UF_GENERALIZED><<<pg, HU_UF_WG>>>(dP, dLen, dPart, (int64_t) Sp, (int64_t) B, pl.uf.L, pl.uf.alpha); break;
		}
		RCHK(hipGetLastError());
		RCHK(hipDeviceSynchronize());
		phase(3);
		k_ur_finish<<<dim3((unsigned) tiles, 16), 256>>>(dPart, dMean, dM2, dD, (int64_t) Sk, (int64_t) Sp, (int64_t) nSlab, raw, (int64_t) n, (int64_t) r0);
		RCHK(hipGetLastError());
		RCHK(hipDeviceSynchronize());
		phase(4);
		if(wantDraws) { RCHK(hipMemcpy(draws + r0 * Sk * Sk, dD, n * bD1, hipMemcpyDeviceToHost)); phase(5); }
	}
	RCHK(hipMemcpy(mean, dMean, bD1, hipMemcpyDeviceToHost));
	RCHK(hipMemcpy(m2, dM2, bD1, hipMemcpyDeviceToHost));
	phase(5);
	return HU_OK;
}

extern "C" int hu_unifrac_rarefied(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, uint64_t seed, const hu_unifrac_rarefied_opts* opts, uint8_t* kept_out, double* mean_out, double* sd_out, double* draws_out) try {
	const char* fn = "hu_unifrac_rarefied";
	if(!mean_out || !sd_out) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuUrPlan pl;
	const int rc = hu_ur_plan(fn, tree, n_otu, n_sample, otu_node, counts, depth, reps, seed, opts, pl);
	if(rc != HU_OK) return rc;
	const size_t n2 = (size_t) pl.Sk * (size_t) pl.Sk;
	std::vector<double> m2(n2);
	if(pl.host || device < 0 || pl.uf.B == 0) hu_ur_host(pl, counts, mean_out, m2.data(), draws_out);   /* B == 0: every read on the root, every distance 0 */
	else {
		for(double& s : g_urTiming) s = 0;
		const int rd = ur_device(fn, device, pl, mean_out, m2.data(), draws_out);
		if(rd != HU_OK) return rd;
	}
	hu_ur_sd((int64_t) n2, pl.reps, m2.data(), sd_out);
	if(kept_out) { std::fill(kept_out, kept_out + n_sample, (uint8_t) 0); for(int32_t j : pl.keptCol) kept_out[j] = 1; }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_unifrac_rarefied"); }
