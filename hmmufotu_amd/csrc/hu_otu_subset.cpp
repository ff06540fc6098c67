// hu_otu_subset: the entry, and the device path of hmmufotu-subset (src/OTUTable.cpp:166-209).  The host builds, for the
// samples that hold more than `size` reads, the prefixes of their nonzero cells and the list of (sample, chunk) pairs the workgroups
// take; the kernels of hu_kern_otu.h do the selection; the host puts the cells back into the table.  The number of launches does not
// depend on the number of samples.  The checks and the host path (device < 0) are hu_otu_table.cpp's.
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
	std::vector<HuOtuSample> smp;
	for(size_t j = 0; j < S; ++j) if(total[j] > size) {
		slot[j] = (int32_t) smp.size();
		HuOtuSample s; memset(&s, 0, sizeof(s));
		s.T = (uint32_t) total[j]; s.col = (uint32_t) j;
		smp.push_back(s);
	}
	const size_t nA = smp.size();
	if(nA == 0) return HU_OK;
	const uint32_t size32 = (uint32_t) size;                          /* size < T < 2^32 */
	/* the nonzero cells of those samples, column by column: row, and the reads before the cell */
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) if(slot[j] >= 0 && counts[i * S + j] > 0) ++smp[(size_t) slot[j]].nnz;
	uint64_t nCells = 0, nChunks = 0;
	const uint64_t perChunk = (uint64_t) o.chunk;
	for(size_t a = 0; a < nA; ++a) {
		HuOtuSample& s = smp[a];
		s.cell0 = nCells; s.pfx0 = nCells + a; s.chunk0 = nChunks;
		const uint64_t work = method == HU_OTU_UNIFORM ? s.T : size32;   /* reads to decide, or draws to make */
		s.nChunk = (uint32_t)((work + perChunk - 1) / perChunk);
		nCells += s.nnz; nChunks += s.nChunk;
	}
	if(nChunks > 0x7fffffffull) { hu_set_error("%s: %llu chunks of %d: more than a grid holds, raise the chunk", fn, (unsigned long long) nChunks, o.chunk); return HU_ERR_ARG; }
	std::vector<uint32_t> prefix((size_t) nCells + nA), fill(nA, 0), run(nA, 0);
	std::vector<int32_t> rowOf((size_t) nCells);
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) {
		const double v = counts[i * S + j];
		if(slot[j] < 0 || !(v > 0)) continue;
		const size_t a = (size_t) slot[j];
		prefix[(size_t) smp[a].pfx0 + fill[a]] = run[a]; rowOf[(size_t) smp[a].cell0 + fill[a]] = (int32_t) i;
		++fill[a]; run[a] += (uint32_t) v;
	}
	for(size_t a = 0; a < nA; ++a) prefix[(size_t) smp[a].pfx0 + smp[a].nnz] = smp[a].T;
	std::vector<HuOtuChunk> chunk((size_t) nChunks);
	for(size_t a = 0; a < nA; ++a) for(uint32_t c = 0; c < smp[a].nChunk; ++c) chunk[(size_t) smp[a].chunk0 + c] = HuOtuChunk{(uint32_t) a, (uint32_t)(c * perChunk)};
	std::vector<HuOtuSel> sel(nA);
	for(size_t a = 0; a < nA; ++a) sel[a] = HuOtuSel{0, size32, smp[a].T};

	OCHK(hipSetDevice(device));
	HuOtuSample* dSmp = nullptr; HuOtuChunk* dChunk = nullptr; HuOtuSel* dSel = nullptr; uint32_t *dPrefix = nullptr, *dOut = nullptr, *dHist = nullptr, *dTie = nullptr;
	HuScope guard([&] { (void) hipFree(dSmp); (void) hipFree(dChunk); (void) hipFree(dSel); (void) hipFree(dPrefix); (void) hipFree(dOut); (void) hipFree(dHist); (void) hipFree(dTie); });
	const bool uniform = method == HU_OTU_UNIFORM;
	const size_t bSmp = nA * sizeof(HuOtuSample), bChunk = (size_t) nChunks * sizeof(HuOtuChunk), bSel = nA * sizeof(HuOtuSel), bPrefix = prefix.size() * 4,
		bOut = std::max<size_t>((size_t) nCells, 1) * 4, bHist = nA * 256 * 4, bTie = (size_t) nChunks * HU_OTU_WAVES * 4;
	{
		size_t freeB = 0, totB = 0;
		OCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = bSmp + bChunk + bPrefix + bOut + (uniform ? bSel + bHist + bTie : 0) + (1 << 20);
		if(need > freeB) { hu_set_error("%s: %zu samples, %llu nonzero cells and %llu chunks need %.3f GB of device memory, %.3f GB are free", fn, nA, (unsigned long long) nCells, (unsigned long long) nChunks, need / 1e9, freeB / 1e9); return HU_ERR_NOMEM; }
	}
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	OCHK(hipMalloc((void**) &dSmp, bSmp)); OCHK(hipMalloc((void**) &dChunk, bChunk)); OCHK(hipMalloc((void**) &dPrefix, bPrefix)); OCHK(hipMalloc((void**) &dOut, bOut));
	OCHK(hipMemcpy(dSmp, smp.data(), bSmp, hipMemcpyHostToDevice)); OCHK(hipMemcpy(dChunk, chunk.data(), bChunk, hipMemcpyHostToDevice));
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
	const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
	const unsigned grid = (unsigned) nChunks;
	if(uniform) {
		const int passes = (o.key_bits + 7) / 8;                        /* the key is below 2^key_bits: its top digit may be a short one */
		for(int p = 0; p < passes; ++p) {
			k_otu_hist<<<grid, HU_OTU_WG>>>(dSmp, dChunk, dSel, dHist, k0, k1, o.key_bits, o.chunk, 8 * (passes - 1 - p), p == 0);
			OCHK(hipGetLastError());
			k_otu_pick<<<(unsigned) nA, 64>>>(dSel, dHist);
			OCHK(hipGetLastError());
		}
		k_otu_ties<<<grid, HU_OTU_WG>>>(dSmp, dChunk, dSel, dTie, k0, k1, o.key_bits, o.chunk);
		OCHK(hipGetLastError());
		k_otu_tie_scan<<<(unsigned) nA, 64>>>(dSmp, dSel, dTie);
		OCHK(hipGetLastError());
		k_otu_take<<<grid, HU_OTU_WG>>>(dSmp, dChunk, dSel, dTie, dPrefix, dOut, k0, k1, o.key_bits, o.chunk);
		OCHK(hipGetLastError());
	}
	else {
		k_otu_multinom<<<grid, HU_OTU_WG>>>(dSmp, dChunk, dPrefix, dOut, k0, k1, o.chunk, size32);
		OCHK(hipGetLastError());
	}
	OCHK(hipDeviceSynchronize());
	g_otuTiming[1] = since() - g_otuTiming[0];
	std::vector<uint32_t> cells((size_t) nCells);
	if(nCells) OCHK(hipMemcpy(cells.data(), dOut, (size_t) nCells * 4, hipMemcpyDeviceToHost));
	for(size_t a = 0; a < nA; ++a) for(uint32_t c = 0; c < smp[a].nnz; ++c)
		out[(size_t) rowOf[(size_t) smp[a].cell0 + c] * S + smp[a].col] = (double) cells[(size_t) smp[a].cell0 + c];
	g_otuTiming[2] = since() - g_otuTiming[0] - g_otuTiming[1];
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_subset"); }
