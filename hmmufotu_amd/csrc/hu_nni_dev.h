// The device half behind the NNI search and the local branch supports: the messages of the level sweeps, the
// buffers of the scoring and the launch of k_nni_score, shared by hu_nni.cpp and hu_support.cpp.
#pragma once
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_nni.h"

#define NCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

namespace {
/* the device half behind the operations of a round */
struct NniDev {
	const char* fn; int32_t n = 0, L = 0, device = 0; const int8_t* seq = nullptr; hu_model_desc model; HuBlenModel m; double lo = 0, hi = 0;
	size_t eMax = 0;
	double *up = nullptr, *down = nullptr, *ratio = nullptr, *vec = nullptr;   /* vec: tStar [3 eMax], f [3 eMax], f0 [eMax] */
	int32_t* iters = nullptr; HuNniEdge* edges = nullptr; HuBlenModel* dm = nullptr;
	std::vector<int8_t> rows;
	~NniDev() { release(); }
	void release() {
		(void) hipFree(up); (void) hipFree(down); (void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(iters); (void) hipFree(edges); (void) hipFree(dm);
		up = down = ratio = vec = nullptr; iters = nullptr; edges = nullptr; dm = nullptr;
	}
	int open() {
		if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
		NCHK(hipSetDevice(device));
		size_t freeB = 0, totB = 0;
		NCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = (size_t) hu_nni_need(n, L);
		if(need > freeB) {
			hu_set_error("%s: %d nodes of %d columns need %zu bytes of device memory (%zu of them for the messages), %zu bytes are free", fn, n, L, need,
				(size_t) n * (size_t) L * 64, freeB);
			return HU_ERR_NOMEM;
		}
		eMax = (size_t) std::max((n - 1) / 2, 1);
		return HU_OK;
	}
	int alloc() {
		if(up) return HU_OK;
		const size_t cells = (size_t) n * (size_t) L;
		NCHK(hipMalloc((void**) &up, cells * 32)); NCHK(hipMalloc((void**) &down, cells * 32));
		if(L > HU_NNI_LDS_COLS) NCHK(hipMalloc((void**) &ratio, eMax * 72 * (size_t) L));
		NCHK(hipMalloc((void**) &vec, eMax * 56)); NCHK(hipMalloc((void**) &iters, eMax * 12));
		NCHK(hipMalloc((void**) &edges, eMax * sizeof(HuNniEdge))); NCHK(hipMalloc((void**) &dm, sizeof(HuBlenModel)));
		NCHK(hipMemcpy(dm, &m, sizeof(HuBlenModel), hipMemcpyHostToDevice));
		return HU_OK;
	}
	int sweep(const int32_t* parent, const double* blen, bool withDown) {
		int rc = alloc();
		if(rc != HU_OK) return rc;
		hu_tree_sweep* sw = nullptr;
		if((rc = hu_tree_sweep_create(n, L, parent, blen, device, &sw)) != HU_OK) return rc;
		rows.assign(seq, seq + (size_t) n * (size_t) L);
		rc = hu_tree_sweep_window(sw, &model, rows.data(), 0, L, up, withDown ? down : nullptr);
		hu_tree_sweep_destroy(sw);
		return rc;
	}
	int loglik(const int32_t* parent, double* ll) {
		int32_t root = 0;
		for(int32_t i = 0; i < n; ++i) if(parent[i] < 0) root = i;
		return hu_tree_loglik(device, n, L, root, &model, up, nullptr, ll);
	}
	/* the messages are those of the last full sweep */
	int score(const std::vector<HuNniEdge>& ed, double* ts, double* f, double* f0, int64_t* nCap) {
		const size_t E = ed.size();
		*nCap = 0;
		if(E == 0) return HU_OK;
		if(E > eMax) { hu_set_error("%s: %zu eligible edges in a tree of %d nodes", fn, E, n); return HU_ERR_STATE; }
		for(const HuNniEdge& e : ed) for(int k = 0; k < 4; ++k) if(e.msg[k] < 0 || e.msg[k] >= 2 * n) { hu_set_error("%s: an edge record points outside the messages", fn); return HU_ERR_STATE; }
		NCHK(hipMemcpy(edges, ed.data(), E * sizeof(HuNniEdge), hipMemcpyHostToDevice));
		NCHK(hipMemset(vec, 0, E * 56)); NCHK(hipMemset(iters, 0, E * 12));
		HuNniArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.edges = edges; a.m = dm; a.csLen = L; a.n = n; a.nEdges = (int32_t) E; a.lo = lo; a.hi = hi;
		a.ratio = ratio; a.tStar = vec; a.f = vec + 3 * E; a.f0 = vec + 6 * E; a.iters = iters;
		(void) hipGetLastError();
		if(L <= HU_NNI_LDS_COLS) {
			const size_t lds = ((size_t) 3 * HU_NNI_WG + (size_t) 9 * L) * 8;     /* at most 40,920 bytes */
			k_nni_score<true><<<(unsigned) E, HU_NNI_WG, lds>>>(a);
		}
		else k_nni_score<false><<<(unsigned) E, HU_NNI_WG, (size_t) 3 * HU_NNI_WG * 8>>>(a);
		NCHK(hipGetLastError());
		NCHK(hipDeviceSynchronize());
		std::vector<double> out(E * 7); std::vector<int32_t> it(E * 3);
		NCHK(hipMemcpy(out.data(), vec, E * 56, hipMemcpyDeviceToHost)); NCHK(hipMemcpy(it.data(), iters, E * 12, hipMemcpyDeviceToHost));
		memcpy(ts, out.data(), E * 24); memcpy(f, out.data() + 3 * E, E * 24); memcpy(f0, out.data() + 6 * E, E * 8);
		for(int32_t x : it) if(x > HU_BLEN_MAX_NEWTON) ++*nCap;
		return HU_OK;
	}
};

int nni_model(const char* fn, const hu_nni_opts* o, const hu_model_desc* model, HuBlenModel* m) {
	if(!o || !model) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(model->dg_k != 0) { hu_set_error("%s: a model with %d discrete Gamma categories: the search runs under the fixed-rate model only", fn, model->dg_k); return HU_ERR_ARG; }
	HuModelDev d;
	const int rc = hu_model_prepare(model, &d);
	if(rc != HU_OK) return rc;
	hu_blen_model_set(m, d.U, d.lam, d.U1);
	return HU_OK;
}

int nni_dev_setup(NniDev& r, const char* fn, const hu_nni_opts* o, int32_t n, int32_t cs_len, const int8_t* seq, const hu_model_desc* model, const HuBlenModel& m) {
	r.fn = fn; r.n = n; r.L = cs_len; r.device = o->blen.device; r.seq = seq; r.model = *model; r.m = m; r.lo = o->blen.min_len; r.hi = o->blen.max_len;
	return r.open();
}
}
