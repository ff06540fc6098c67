// hu_tree_nni_support: the entry and the device path of hmmufotu-amd-tree --ml-lengths --support.  The checks, the
// weights' host form and the host path are hu_support_host.cpp's; the kernels are hu_kern_support.h's; the buffers of the
// scoring and k_nni_score's launch are hu_nni_dev.h's, shared with the NNI search, the messages hu_tree_dev.h's.  The need is held against the budget and the free
// memory before anything is allocated.  The sums of the replicates, which only tests ask for, leave the device launch by launch.
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_nni_dev.h"
#include "hu_kern_support.h"

static thread_local double g_supTiming[4] = {0, 0, 0, 0};

extern "C" int hu_support_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_supTiming, sizeof(g_supTiming));
	return HU_OK;
}

namespace {
template<class T> struct DevBuf {
	T* p = nullptr;
	~DevBuf() { (void) hipFree(p); }
};

/* the table Wt [L][Bpad] on the current device */
int weights_dev(const char* fn, int64_t L, int64_t B, uint64_t seed, DevBuf<uint16_t>& Wt) {
	const int64_t Bpad = hu_support_bpad(B);
	TCHK(hipMalloc((void**) &Wt.p, (size_t)(L * Bpad) * 2));
	TCHK(hipMemset(Wt.p, 0, (size_t)(L * Bpad) * 2));
	(void) hipGetLastError();
	k_support_weights<<<(unsigned)((B + 255) / 256), 256>>>(Wt.p, L, B, Bpad, seed);
	TCHK(hipGetLastError());
	TCHK(hipDeviceSynchronize());
	return HU_OK;
}
}

extern "C" int hu_support_weights_device(int32_t device, int32_t cs_len, int32_t replicates, uint64_t seed, uint16_t* w) try {
	const char* fn = "hu_support_weights_device";
	if(!w) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(cs_len < 1 || cs_len > 65535 || replicates < 1 || replicates > HU_SUPPORT_MAX_REPLICATES) {
		hu_set_error("%s: %d columns and %d replicates: 1 to 65535 and 1 to %d", fn, cs_len, replicates, HU_SUPPORT_MAX_REPLICATES); return HU_ERR_ARG; }
	if(device < 0 || hu_device_count() <= device) { hu_set_error("%s: device %d asked for, %d gfx950 device(s) visible", fn, device, hu_device_count()); return HU_ERR_DEVICE; }
	TCHK(hipSetDevice(device));
	const int64_t L = cs_len, B = replicates, Bpad = hu_support_bpad(B);
	DevBuf<uint16_t> Wt;
	int rc = weights_dev(fn, L, B, seed, Wt);
	if(rc != HU_OK) return rc;
	std::vector<uint16_t> t((size_t)(L * Bpad));
	TCHK(hipMemcpy(t.data(), Wt.p, t.size() * 2, hipMemcpyDeviceToHost));
	for(int64_t b = 0; b < B; ++b) for(int64_t j = 0; j < L; ++j) w[b * L + j] = t[(size_t)(j * Bpad + b)];
	return HU_OK;
} catch(...) { return hu_catch_all("hu_support_weights_device"); }

extern "C" int hu_tree_nni_support(const hu_support_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f,
		int32_t* count, double* sums) try {
	const char* fn = "hu_tree_nni_support";
	if(!opts) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(!n_edges || !skipped || edge_cap < 0 || (edge_cap > 0 && (!edge_node || !t_star || !f || !count))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	hu_nni_opts no;
	hu_nni_default_opts(&no);
	HuBlenModel m;
	int rc = hu_search_model(fn, &no, model, "the search runs", &m);
	if(rc != HU_OK) return rc;
	g_supTiming[0] = g_supTiming[1] = g_supTiming[2] = g_supTiming[3] = 0;
	if(opts->blen.host != 0 || opts->blen.device < 0)
		return hu_support_host_entry(fn, opts, n, cs_len, parent, blen, seq, m, edge_cap, n_edges, skipped, edge_node, t_star, f, count, sums, g_supTiming);
	HuBlenTopo tp;
	if((rc = hu_support_check(fn, opts, n, cs_len, parent, blen, seq, &tp, &no)) != HU_OK) return rc;
	std::vector<HuNniEdge> edges;
	hu_nni_edges(tp, parent, blen, &edges, skipped);
	*n_edges = (int32_t) edges.size();
	if((int64_t) edges.size() > edge_cap) { hu_set_error("%s: %zu eligible edges, the outputs hold %d", fn, edges.size(), edge_cap); return HU_ERR_ARG; }
	NniDev r;
	if((rc = r.open(fn, &no, n, cs_len, model, m)) != HU_OK) return rc;
	const int64_t L = cs_len, B = opts->replicates, Bpad = hu_support_bpad(B);
	{
		size_t freeB = 0, totB = 0;
		TCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = (size_t) hu_support_need(n, cs_len, opts->replicates);
		if(need > freeB) {
			hu_set_error("%s: %d nodes of %d columns and %d replicates need %zu bytes of device memory (%zu of them for the table of weights), %zu bytes are free", fn,
				n, cs_len, opts->replicates, need, (size_t)(2 * Bpad * L), freeB);
			return HU_ERR_NOMEM;
		}
	}
	if(edges.empty()) return HU_OK;
	const size_t E = edges.size();
	double t0 = hu_now_s();
	if((rc = r.msg.sweep(n, parent, blen, seq, true)) != HU_OK || (rc = r.alloc()) != HU_OK) return rc;
	g_supTiming[0] = hu_now_s() - t0; t0 = hu_now_s();
	int64_t nCap = 0;
	std::vector<double> f0(E), f2(E * 3);
	if((rc = r.score(edges, t_star, f, f0.data(), &nCap)) != HU_OK) return rc;
	g_supTiming[1] = hu_now_s() - t0; t0 = hu_now_s();
	DevBuf<uint16_t> Wt;
	if((rc = weights_dev(fn, L, B, opts->seed, Wt)) != HU_OK) return rc;
	g_supTiming[2] = hu_now_s() - t0; t0 = hu_now_s();
	/* the edges of one launch: all of them, or as many as the buffer of the sums holds */
	const size_t perEdge = (size_t) B * 16, chunk = sums ? std::max<size_t>(((size_t) 16 << 20) / perEdge, 1) : E;
	DevBuf<double> dF2, dSums; DevBuf<int32_t> dCnt;
	TCHK(hipMalloc((void**) &dF2.p, E * 24)); TCHK(hipMalloc((void**) &dCnt.p, E * 8));
	TCHK(hipMemset(dF2.p, 0, E * 24)); TCHK(hipMemset(dCnt.p, 0, E * 8));
	if(sums) TCHK(hipMalloc((void**) &dSums.p, std::min(chunk, E) * perEdge));
	const bool lds = L <= HU_SUPPORT_LDS_COLS;
	/* 81,920 bytes at the most: above the 64 KB a kernel gets unasked */
	const size_t ldsMax = ((size_t) 3 * HU_NNI_WG + (size_t) 2 * HU_SUPPORT_LDS_COLS) * 8;
	if(lds) TCHK(hipFuncSetAttribute((const void*) k_nni_support<true, HU_SUPPORT_RPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) ldsMax));
	if(!lds && !r.ratio) { hu_set_error("%s: no scratch for the columns' values", fn); return HU_ERR_STATE; }
	for(size_t e0 = 0; e0 < E; e0 += chunk) {
		const size_t ne = std::min(chunk, E - e0);
		HuSupportArgs a; memset(&a, 0, sizeof(a));
		a.up = r.msg.up; a.down = r.msg.down; a.edges = r.edges + e0; a.m = r.msg.dm; a.csLen = L; a.B = B; a.Bpad = Bpad; a.n = n; a.nEdges = (int32_t) ne;
		a.tStar = r.vec + 3 * e0; a.Wt = Wt.p; a.dScratch = lds ? nullptr : r.ratio + e0 * 9 * (size_t) L;
		a.f2 = dF2.p + 3 * e0; a.count = dCnt.p + e0; a.bad = dCnt.p + E + e0; a.sums = dSums.p;
		(void) hipGetLastError();
		if(lds) k_nni_support<true, HU_SUPPORT_RPT><<<(unsigned) ne, HU_NNI_WG, ((size_t) 3 * HU_NNI_WG + (size_t) 2 * L) * 8>>>(a);
		else k_nni_support<false, HU_SUPPORT_RPT><<<(unsigned) ne, HU_NNI_WG, (size_t) 3 * HU_NNI_WG * 8>>>(a);
		TCHK(hipGetLastError());
		TCHK(hipDeviceSynchronize());
		if(sums) TCHK(hipMemcpy(sums + e0 * (size_t) B * 2, dSums.p, ne * perEdge, hipMemcpyDeviceToHost));
	}
	std::vector<int32_t> cb(E * 2);
	TCHK(hipMemcpy(f2.data(), dF2.p, E * 24, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(cb.data(), dCnt.p, E * 8, hipMemcpyDeviceToHost));
	g_supTiming[3] = hu_now_s() - t0;
	int64_t bad = -1;
	for(size_t e = 0; e < E && bad < 0; ++e) if(cb[E + e] != 0) bad = (int64_t) e;
	if((rc = hu_support_verify(fn, edges, f, f2.data(), bad)) != HU_OK) return rc;
	for(size_t e = 0; e < E; ++e) { edge_node[e] = edges[e].u; count[e] = cb[e]; }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_tree_nni_support"); }
