// hu_otu_subset: the entry, and the device path of hmmufotu-subset (src/OTUTable.cpp:166-209).  The host builds, for the
// samples that hold more than `size` reads, the prefixes of their nonzero cells and the list of (sample, chunk) pairs the workgroups
// take (the records of hu_draw.h); the kernels of hu_kern_draw.h (uniform) or hu_kern_otu.h (multinomial) do the selection; the host
// puts the cells back into the table.  The number of launches does not depend on the number of samples.  The checks and the host path
// (device < 0) are hu_otu_table.cpp's.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_otu.h"

static thread_local double g_otuTiming[3] = {0, 0, 0};

#define OCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_otu_subset_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_otuTiming, sizeof(g_otuTiming));
	return HU_OK;
}

extern "C" int hu_otu_subset(int device, int64_t n_otu, int64_t n_sample, const double* counts, uint64_t size, int method, uint64_t seed, const hu_otu_opts* opts,
		double* out) try {
	const char* fn = "hu_otu_subset";
	hu_otu_opts o;
	std::vector<uint64_t> total;
	const int rc = hu_otu_subset_check(fn, n_otu, n_sample, counts, size, method, opts, out, &o, total);
	if(rc != HU_OK) return rc;
	if(device < 0) { hu_otu_subset_host(n_otu, n_sample, counts, total, size, method, seed, o.key_bits, out); return HU_OK; }
	g_otuTiming[0] = g_otuTiming[1] = g_otuTiming[2] = 0;
	if(hu_device_count() <= 0) { hu_set_error("no gfx950 device visible: pass device < 0 for the host path"); return HU_ERR_DEVICE; }
	const size_t M = (size_t) n_otu, S = (size_t) n_sample;
	std::copy(counts, counts + M * S, out);
	/* the samples with more than `size` reads; the others are returned untouched */
	std::vector<int32_t> slot(S, -1);
	std::vector<HuAlSample> smp;
	for(size_t j = 0; j < S; ++j) if(total[j] > size) {
		slot[j] = (int32_t) smp.size();
		smp.push_back(HuAlSample{0, 0, 0, (uint32_t) total[j], (uint32_t) j, 0});
	}
	const size_t nA = smp.size();
	if(nA == 0) return HU_OK;
	const bool uniform = method == HU_OTU_UNIFORM;
	const uint32_t size32 = (uint32_t) size;                          /* size < T < 2^32 */
	/* the nonzero cells of those samples, column by column: row, and the reads before the cell */
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) if(slot[j] >= 0 && counts[i * S + j] > 0) ++smp[(size_t) slot[j]].nnz;
	/* a sample is one draw and one group, all under the key of the seed: reads to decide, or draws to make, by the chunk */
	const uint64_t perChunk = (uint64_t) o.chunk;
	uint64_t nCells = 0, nChunks = 0;
	for(const HuAlSample& s : smp) nChunks += ((uniform ? s.T : size32) + perChunk - 1) / perChunk;
	if(nChunks > 0x7fffffffull) { hu_set_error("%s: %llu chunks of %d: more than a grid holds, raise the chunk", fn, (unsigned long long) nChunks, o.chunk); return HU_ERR_ARG; }
	std::vector<HuAlDraw> draw(nA); std::vector<HuAlGroup> grp; std::vector<HuAlChunk> chunk; std::vector<HuAlSel> sel(nA);
	chunk.reserve((size_t) nChunks);
	for(size_t a = 0; a < nA; ++a) {
		HuAlSample& s = smp[a];
		s.pfx0 = nCells + a;
		draw[a] = HuAlDraw{nCells, (uint64_t) chunk.size() * HU_DRAW_WAVES, (uint32_t) a, size32};
		sel[a] = HuAlSel{0, size32, s.T};
		hu_draw_add_group(grp, chunk, (uint32_t) a, seed, (uint32_t) a, 1u, uniform ? s.T : size32, perChunk);
		nCells += s.nnz;
	}
	std::vector<uint32_t> prefix((size_t) nCells + nA), fill(nA, 0), run(nA, 0);
	std::vector<int32_t> rowOf((size_t) nCells);
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) {
		const double v = counts[i * S + j];
		if(slot[j] < 0 || !(v > 0)) continue;
		const size_t a = (size_t) slot[j];
		prefix[(size_t) smp[a].pfx0 + fill[a]] = run[a]; rowOf[(size_t) draw[a].cell0 + fill[a]] = (int32_t) i;
		++fill[a]; run[a] += (uint32_t) v;
	}
	for(size_t a = 0; a < nA; ++a) prefix[(size_t) smp[a].pfx0 + smp[a].nnz] = smp[a].T;

	OCHK(hipSetDevice(device));
	HuAlSample* dSmp = nullptr; HuAlDraw* dDraw = nullptr; HuAlGroup* dGrp = nullptr; HuAlChunk* dChunk = nullptr; HuAlSel* dSel = nullptr;
	uint32_t *dPrefix = nullptr, *dOut = nullptr, *dHist = nullptr, *dTie = nullptr;
	HuScope guard([&] { (void) hipFree(dSmp); (void) hipFree(dDraw); (void) hipFree(dGrp); (void) hipFree(dChunk); (void) hipFree(dSel); (void) hipFree(dPrefix); (void) hipFree(dOut);
		(void) hipFree(dHist); (void) hipFree(dTie); });
	const size_t bSmp = nA * sizeof(HuAlSample), bDraw = nA * sizeof(HuAlDraw), bGrp = nA * sizeof(HuAlGroup), bChunk = (size_t) nChunks * sizeof(HuAlChunk), bSel = nA * sizeof(HuAlSel),
		bPrefix = prefix.size() * 4, bOut = std::max<size_t>((size_t) nCells, 1) * 4, bHist = nA * 256 * 4, bTie = (size_t) nChunks * HU_DRAW_WAVES * 4;
	{
		size_t freeB = 0, totB = 0;
		OCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = bSmp + bDraw + bGrp + bChunk + bPrefix + bOut + (uniform ? bSel + bHist + bTie : 0) + (1 << 20);
		if(need > freeB) { hu_set_error("%s: %zu samples, %llu nonzero cells and %llu chunks need %.3f GB of device memory, %.3f GB are free", fn, nA, (unsigned long long) nCells, (unsigned long long) nChunks, need / 1e9, freeB / 1e9); return HU_ERR_NOMEM; }
	}
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	OCHK(hipMalloc((void**) &dSmp, bSmp)); OCHK(hipMalloc((void**) &dDraw, bDraw)); OCHK(hipMalloc((void**) &dGrp, bGrp)); OCHK(hipMalloc((void**) &dChunk, bChunk));
	OCHK(hipMalloc((void**) &dPrefix, bPrefix)); OCHK(hipMalloc((void**) &dOut, bOut));
	OCHK(hipMemcpy(dSmp, smp.data(), bSmp, hipMemcpyHostToDevice)); OCHK(hipMemcpy(dDraw, draw.data(), bDraw, hipMemcpyHostToDevice));
	OCHK(hipMemcpy(dGrp, grp.data(), bGrp, hipMemcpyHostToDevice)); OCHK(hipMemcpy(dChunk, chunk.data(), bChunk, hipMemcpyHostToDevice));
	OCHK(hipMemcpy(dPrefix, prefix.data(), bPrefix, hipMemcpyHostToDevice));
	OCHK(hipMemset(dOut, 0, bOut));
	if(uniform) {
		OCHK(hipMalloc((void**) &dSel, bSel)); OCHK(hipMalloc((void**) &dHist, bHist)); OCHK(hipMalloc((void**) &dTie, bTie));
		OCHK(hipMemcpy(dSel, sel.data(), bSel, hipMemcpyHostToDevice));
		OCHK(hipMemset(dHist, 0, bHist));
	}
	OCHK(hipDeviceSynchronize());
	g_otuTiming[0] = since();
	(void) hipGetLastError();
	if(uniform) {
		/* no slot map: a draw's cells stay in table order */
		const HuDrawDev dv = {dSmp, dDraw, dGrp, dChunk, dSel, dHist, dTie, dPrefix, nullptr, dOut, o.key_bits, o.chunk};
		OCHK(hu_draw_select<1>(dv, (unsigned) nA, (unsigned) nChunks, 1));
		OCHK(hu_draw_take<1>(dv, (unsigned) nChunks, 1));
	}
	else {
		k_otu_multinom<<<(unsigned) nChunks, HU_DRAW_WG>>>(dSmp, dDraw, dGrp, dChunk, dPrefix, dOut, o.chunk, size32);
		OCHK(hipGetLastError());
	}
	OCHK(hipDeviceSynchronize());
	g_otuTiming[1] = since() - g_otuTiming[0];
	std::vector<uint32_t> cells((size_t) nCells);
	if(nCells) OCHK(hipMemcpy(cells.data(), dOut, (size_t) nCells * 4, hipMemcpyDeviceToHost));
	for(size_t a = 0; a < nA; ++a) for(uint32_t c = 0; c < smp[a].nnz; ++c)
		out[(size_t) rowOf[(size_t) draw[a].cell0 + c] * S + smp[a].col] = (double) cells[(size_t) draw[a].cell0 + c];
	g_otuTiming[2] = since() - g_otuTiming[0] - g_otuTiming[1];
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_subset"); }
