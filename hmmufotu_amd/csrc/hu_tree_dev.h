// What the device halves of the tree family share: the check of a HIP call, the model check of the searches, the
// holder of the level sweeps' messages behind the NNI search, the supports, the SPR search and the insertion, and the fit of a
// search's round.  A mode's own holder (NniDev, SprDev, AddDev) keeps its scoring buffers and its score() and holds a HuTreeDev.
#pragma once
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_tree_blen.h"

#define TCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

/* the model of a search in the form the kernels read; what: the clause of the refusal of a discrete Gamma model */
inline int hu_search_model(const char* fn, const void* opts, const hu_model_desc* model, const char* what, HuBlenModel* m) {
	if(!opts || !model) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(model->dg_k != 0) { hu_set_error("%s: a model with %d discrete Gamma categories: %s under the fixed-rate model only", fn, model->dg_k, what); return HU_ERR_ARG; }
	HuModelDev d;
	const int rc = hu_model_prepare(model, &d);
	if(rc != HU_OK) return rc;
	hu_blen_model_set(m, d.U, d.lam, d.U1);
	return HU_OK;
}

namespace {
/* the messages up, down [nCap][L][4] of a tree of up to nCap nodes and the model in a buffer.  A move changes the topology, so every
 * sweep has a sweep handle of its own */
struct HuTreeDev {
	const char* fn = ""; int32_t nCap = 0, L = 0, device = 0; hu_model_desc model; HuBlenModel m;
	double *up = nullptr, *down = nullptr; HuBlenModel* dm = nullptr;
	std::vector<int8_t> rows;
	~HuTreeDev() { release(); }
	void release() {
		(void) hipFree(up); (void) hipFree(down); (void) hipFree(dm);
		up = down = nullptr; dm = nullptr;
	}
	/* the device, and the need held against the free memory before anything is allocated; describe: what needs it, after "<fn>: " */
	int open(const char* fn_, const hu_blen_opts& bo, int32_t n_cap, int32_t cs_len, const hu_model_desc* md, const HuBlenModel& hm, size_t need, const char* describe) {
		fn = fn_; nCap = n_cap; L = cs_len; device = bo.device; model = *md; m = hm;
		if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
		TCHK(hipSetDevice(device));
		size_t freeB = 0, totB = 0;
		TCHK(hipMemGetInfo(&freeB, &totB));
		if(need > freeB) {
			hu_set_error("%s: %s need %zu bytes of device memory (%zu of them for the messages), %zu bytes are free", fn, describe, need,
				(size_t) nCap * (size_t) L * 64, freeB);
			return HU_ERR_NOMEM;
		}
		return HU_OK;
	}
	int alloc() {
		if(up) return HU_OK;
		const size_t cells = (size_t) nCap * (size_t) L;
		TCHK(hipMalloc((void**) &up, cells * 32)); TCHK(hipMalloc((void**) &down, cells * 32));
		TCHK(hipMalloc((void**) &dm, sizeof(HuBlenModel)));
		TCHK(hipMemcpy(dm, &m, sizeof(HuBlenModel), hipMemcpyHostToDevice));
		return HU_OK;
	}
	int sweep(int32_t n, const int32_t* parent, const double* blen, const int8_t* seq, bool withDown) {
		if(n > nCap) { hu_set_error("%s: %d nodes, the buffers hold %d", fn, n, nCap); return HU_ERR_STATE; }
		int rc = alloc();
		if(rc != HU_OK) return rc;
		hu_tree_sweep* sw = nullptr;
		if((rc = hu_tree_sweep_create(n, L, parent, blen, device, &sw)) != HU_OK) return rc;
		rows.assign(seq, seq + (size_t) n * (size_t) L);
		rc = hu_tree_sweep_window(sw, &model, rows.data(), 0, L, up, withDown ? down : nullptr);
		hu_tree_sweep_destroy(sw);
		return rc;
	}
	/* of the last sweep */
	int loglik(int32_t n, const int32_t* parent, double* ll) {
		int32_t root = 0;
		for(int32_t i = 0; i < n; ++i) if(parent[i] < 0) root = i;
		return hu_tree_loglik(device, n, L, root, &model, up, nullptr, ll);
	}
	/* a round's trial: one up sweep and the log-likelihood */
	int trial(int32_t n, const int32_t* parent, const double* blen, const int8_t* seq, double* ll) {
		const int rc = sweep(n, parent, blen, seq, false);
		return rc == HU_OK ? loglik(n, parent, ll) : rc;
	}
};

/* a round's fit on the device: hu_tree_optimize_lengths in place under the search's options.  The fit holds messages of its own, so
 * the mode's holder r (its scoring buffers and its HuTreeDev msg) releases everything first */
template<class Dev> int hu_search_fit_device(Dev& r, const hu_blen_opts& o, int32_t n, const int32_t* parent, double* blen, const int8_t* seq, double* ll) {
	r.release();
	hu_blen_opts bo = hu_search_fit_opts(o);
	const int rc = hu_tree_optimize_lengths(&bo, n, r.msg.L, parent, blen, seq, &r.msg.model);
	*ll = bo.ll_final;
	return rc;
}
}
