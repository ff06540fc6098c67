// The device half behind the NNI search and the local branch supports: the buffers of the scoring and the launch
// of k_nni_score, shared by hu_nni.cpp and hu_support.cpp.  The messages of the level sweeps are hu_tree_dev.h's.
#pragma once
#include "hu_tree_dev.h"
#include "hu_kern_nni.h"

namespace {
/* the buffers of the scoring behind the operations of a round; msg: the messages */
struct NniDev {
	HuTreeDev msg; const char* fn; int32_t n = 0, L = 0; double lo = 0, hi = 0;
	size_t eMax = 0;
	double *ratio = nullptr, *vec = nullptr;                                   /* vec: tStar [3 eMax], f [3 eMax], f0 [eMax] */
	int32_t* iters = nullptr; HuNniEdge* edges = nullptr;
	~NniDev() { release(); }
	void release() {
		(void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(iters); (void) hipFree(edges);
		ratio = vec = nullptr; iters = nullptr; edges = nullptr;
		msg.release();
	}
	int open(const char* fn_, const hu_nni_opts* o, int32_t n_, int32_t cs_len, const hu_model_desc* model, const HuBlenModel& m) {
		fn = fn_; n = n_; L = cs_len; lo = o->blen.min_len; hi = o->blen.max_len;
		eMax = (size_t) std::max((n - 1) / 2, 1);
		char what[64];
		snprintf(what, sizeof(what), "%d nodes of %d columns", n, L);
		return msg.open(fn, o->blen, n, L, model, m, (size_t) hu_nni_need(n, L), what);
	}
	int alloc() {
		if(vec) return HU_OK;
		if(L > HU_NNI_LDS_COLS) TCHK(hipMalloc((void**) &ratio, eMax * 72 * (size_t) L));
		TCHK(hipMalloc((void**) &vec, eMax * 56)); TCHK(hipMalloc((void**) &iters, eMax * 12));
		TCHK(hipMalloc((void**) &edges, eMax * sizeof(HuNniEdge)));
		return HU_OK;
	}
	/* the messages are those of the last full sweep */
	int score(const std::vector<HuNniEdge>& ed, double* ts, double* f, double* f0, int64_t* nCap) {
		const size_t E = ed.size();
		*nCap = 0;
		if(E == 0) return HU_OK;
		if(E > eMax) { hu_set_error("%s: %zu eligible edges in a tree of %d nodes", fn, E, n); return HU_ERR_STATE; }
		for(const HuNniEdge& e : ed) for(int k = 0; k < 4; ++k) if(e.msg[k] < 0 || e.msg[k] >= 2 * n) { hu_set_error("%s: an edge record points outside the messages", fn); return HU_ERR_STATE; }
		const int rc = alloc();
		if(rc != HU_OK) return rc;
		TCHK(hipMemcpy(edges, ed.data(), E * sizeof(HuNniEdge), hipMemcpyHostToDevice));
		TCHK(hipMemset(vec, 0, E * 56)); TCHK(hipMemset(iters, 0, E * 12));
		HuNniArgs a; memset(&a, 0, sizeof(a));
		a.up = msg.up; a.down = msg.down; a.edges = edges; a.m = msg.dm; a.csLen = L; a.n = n; a.nEdges = (int32_t) E; a.lo = lo; a.hi = hi;
		a.ratio = ratio; a.tStar = vec; a.f = vec + 3 * E; a.f0 = vec + 6 * E; a.iters = iters;
		(void) hipGetLastError();
		if(L <= HU_NNI_LDS_COLS) {
			const size_t lds = ((size_t) 3 * HU_NNI_WG + (size_t) 9 * L) * 8;     /* at most 40,920 bytes */
			k_nni_score<true><<<(unsigned) E, HU_NNI_WG, lds>>>(a);
		}
		else k_nni_score<false><<<(unsigned) E, HU_NNI_WG, (size_t) 3 * HU_NNI_WG * 8>>>(a);
		TCHK(hipGetLastError());
		TCHK(hipDeviceSynchronize());
		std::vector<double> out(E * 7); std::vector<int32_t> it(E * 3);
		TCHK(hipMemcpy(out.data(), vec, E * 56, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(it.data(), iters, E * 12, hipMemcpyDeviceToHost));
		memcpy(ts, out.data(), E * 24); memcpy(f, out.data() + 3 * E, E * 24); memcpy(f0, out.data() + 6 * E, E * 8);
		for(int32_t x : it) if(x > HU_BLEN_MAX_NEWTON) ++*nCap;
		return HU_OK;
	}
};

}
