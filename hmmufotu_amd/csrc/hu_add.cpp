// hu_tree_add_scores and hu_tree_add_search: the entries and the device path of hmmufotu-amd-tree --ml-lengths
// --start-tree T --add.  The checks, the host path, the insertion and the round loop are hu_add_host.cpp's; the scoring kernels are
// hu_kern_add.h's; the messages come from the level sweeps of the build (hu_tree_sweep_*) and the fit from hu_tree_optimize_lengths.
// An insertion changes the topology, so every sweep of a round has a sweep handle of its own.  The need is held against the budget
// and the free memory before anything is allocated; the buffers of the scoring are released while a fit holds its own.
#include <chrono>
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_kern_add.h"

#define ACHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

static thread_local double g_addTiming[4] = {0, 0, 0, 0};

extern "C" int hu_add_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_addTiming, sizeof(g_addTiming));
	return HU_OK;
}

namespace {
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* the device half behind the operations of a round; nCap: the nodes of the final tree */
struct AddDev {
	const char* fn; int32_t nCap = 0, L = 0, nQuery = 0, device = 0; const hu_add_opts* o = nullptr; hu_model_desc model; HuBlenModel m; double lo = 0, hi = 0;
	size_t qCap = 0, nOutCap = 0, ratioCap = 0;
	double *up = nullptr, *down = nullptr, *dblen = nullptr, *ratio = nullptr, *vec = nullptr, *best = nullptr;   /* vec: tStar, f [qCap][n]; best: t, f [qCap] */
	int32_t* bestW = nullptr; int8_t* rowsDev = nullptr; HuBlenModel* dm = nullptr;
	std::vector<int8_t> rows;
	~AddDev() { release(); }
	void release_slab() {
		(void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(best); (void) hipFree(bestW); (void) hipFree(rowsDev);
		ratio = vec = best = nullptr; bestW = nullptr; rowsDev = nullptr; qCap = nOutCap = ratioCap = 0;
	}
	void release() {
		release_slab();
		(void) hipFree(up); (void) hipFree(down); (void) hipFree(dblen); (void) hipFree(dm);
		up = down = dblen = nullptr; dm = nullptr;
	}
	int open() {
		if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
		ACHK(hipSetDevice(device));
		size_t freeB = 0, totB = 0;
		ACHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = (size_t) hu_add_need(nCap, L, nQuery);
		if(need > freeB) {
			hu_set_error("%s: %d nodes of %d columns and %d new sequences need %zu bytes of device memory (%zu of them for the messages), %zu bytes are free", fn, nCap, L,
				nQuery, need, (size_t) nCap * (size_t) L * 64, freeB);
			return HU_ERR_NOMEM;
		}
		return HU_OK;
	}
	int alloc() {
		if(up) return HU_OK;
		const size_t cells = (size_t) nCap * (size_t) L;
		ACHK(hipMalloc((void**) &up, cells * 32)); ACHK(hipMalloc((void**) &down, cells * 32));
		ACHK(hipMalloc((void**) &dblen, (size_t) nCap * 8));
		ACHK(hipMalloc((void**) &dm, sizeof(HuBlenModel)));
		ACHK(hipMemcpy(dm, &m, sizeof(HuBlenModel), hipMemcpyHostToDevice));
		return HU_OK;
	}
	int sweep(int32_t n, const int32_t* parent, const double* blen, const int8_t* seq) {
		if(n > nCap) { hu_set_error("%s: %d nodes, the buffers hold %d", fn, n, nCap); return HU_ERR_STATE; }
		int rc = alloc();
		if(rc != HU_OK) return rc;
		hu_tree_sweep* sw = nullptr;
		if((rc = hu_tree_sweep_create(n, L, parent, blen, device, &sw)) != HU_OK) return rc;
		rows.assign(seq, seq + (size_t) n * (size_t) L);
		rc = hu_tree_sweep_window(sw, &model, rows.data(), 0, L, up, down);
		hu_tree_sweep_destroy(sw);
		if(rc != HU_OK) return rc;
		ACHK(hipMemcpy(dblen, blen, (size_t) n * 8, hipMemcpyHostToDevice));
		return HU_OK;
	}
	/* the queries rows [nq][L] against the messages of the last sweep, slab by slab; ts, f [nq][n] may be NULL */
	int score(int32_t n, int32_t root, double t0, int32_t nq, const int8_t* qrows, double* ts, double* f, int32_t* bw, double* bt, double* bf) {
		if(nq == 0) return HU_OK;
		if(n > nCap || root < 0 || root >= n) { hu_set_error("%s: %d nodes with the top node %d, the buffers hold %d", fn, n, root, nCap); return HU_ERR_STATE; }
		const int32_t tile = hu_add_tile(o);
		const size_t sL = (size_t) L, sN = (size_t) n;
		const size_t slab = (size_t) std::min<int64_t>(hu_add_slab_queries(o, n, L), nq), tilesMax = (slab + tile - 1) / tile;
		const size_t ratioNeed = L > HU_BLEN_LDS_COLS ? tilesMax * sN * 3 * sL : 0;
		if(slab > qCap || slab * sN > nOutCap || ratioNeed > ratioCap) {
			release_slab();
			if(ratioNeed) ACHK(hipMalloc((void**) &ratio, ratioNeed * 8));
			ACHK(hipMalloc((void**) &vec, slab * sN * 16)); ACHK(hipMalloc((void**) &best, slab * 16)); ACHK(hipMalloc((void**) &bestW, slab * 4));
			ACHK(hipMalloc((void**) &rowsDev, slab * sL));
			qCap = slab; nOutCap = slab * sN; ratioCap = ratioNeed;
		}
		for(size_t q0 = 0; q0 < (size_t) nq; q0 += slab) {
			const size_t k = std::min(slab, (size_t) nq - q0), tiles = (k + tile - 1) / tile;
			ACHK(hipMemcpy(rowsDev, qrows + q0 * sL, k * sL, hipMemcpyHostToDevice));
			ACHK(hipMemset(vec, 0, k * sN * 16));
			HuAddArgs a; memset(&a, 0, sizeof(a));
			a.up = up; a.down = down; a.blen = dblen; a.q = rowsDev; a.m = dm; a.csLen = L; a.n = n; a.root = root; a.nq = (int32_t) k; a.tile = tile;
			a.lo = lo; a.hi = hi; a.t0 = t0; a.ratio = ratio; a.tStar = vec; a.f = vec + k * sN; a.bestW = bestW; a.bestT = best; a.bestF = best + k;
			(void) hipGetLastError();
			const dim3 grid((unsigned) n, (unsigned) tiles);
			if(L <= HU_BLEN_LDS_COLS) {
				const size_t lds = ((size_t) 3 * HU_ADD_WG + (size_t) 3 * sL) * 8;       /* at most 40,944 bytes */
				k_add_score<true><<<grid, HU_ADD_WG, lds>>>(a);
			}
			else k_add_score<false><<<grid, HU_ADD_WG, (size_t) 3 * HU_ADD_WG * 8>>>(a);
			ACHK(hipGetLastError());
			k_add_best<<<(unsigned) k, HU_ADD_WG>>>(a);
			ACHK(hipGetLastError());
			ACHK(hipDeviceSynchronize());
			if(ts && f) {
				ACHK(hipMemcpy(ts + q0 * sN, vec, k * sN * 8, hipMemcpyDeviceToHost));
				ACHK(hipMemcpy(f + q0 * sN, vec + k * sN, k * sN * 8, hipMemcpyDeviceToHost));
			}
			ACHK(hipMemcpy(bw + q0, bestW, k * 4, hipMemcpyDeviceToHost));
			ACHK(hipMemcpy(bt + q0, best, k * 8, hipMemcpyDeviceToHost));
			ACHK(hipMemcpy(bf + q0, best + k, k * 8, hipMemcpyDeviceToHost));
		}
		return HU_OK;
	}
};

int add_model(const char* fn, const hu_add_opts* o, const hu_model_desc* model, HuBlenModel* m) {
	if(!o || !model) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(model->dg_k != 0) { hu_set_error("%s: a model with %d discrete Gamma categories: sequences are inserted under the fixed-rate model only", fn, model->dg_k); return HU_ERR_ARG; }
	HuModelDev d;
	const int rc = hu_model_prepare(model, &d);
	if(rc != HU_OK) return rc;
	hu_blen_model_set(m, d.U, d.lam, d.U1);
	return HU_OK;
}

int add_dev_setup(AddDev& r, const char* fn, const hu_add_opts* o, int32_t n_final, int32_t cs_len, int32_t n_query, const hu_model_desc* model, const HuBlenModel& m) {
	r.fn = fn; r.nCap = n_final; r.L = cs_len; r.nQuery = n_query; r.device = o->blen.device; r.o = o; r.model = *model; r.m = m; r.lo = o->blen.min_len; r.hi = o->blen.max_len;
	return r.open();
}
}

extern "C" int hu_tree_add_scores(const hu_add_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t n_query, const int8_t* qseq, double* t_star, double* f, int32_t* best_w, double* best_t, double* best_f) try {
	const char* fn = "hu_tree_add_scores";
	HuBlenModel m;
	int rc = add_model(fn, opts, model, &m);
	if(rc != HU_OK) return rc;
	if((t_star == nullptr) != (f == nullptr) || (n_query > 0 && (!best_w || !best_t || !best_f))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	if(opts->blen.host != 0 || opts->blen.device < 0) return hu_add_host_scores_entry(fn, opts, n, cs_len, parent, blen, seq, m, n_query, qseq, t_star, f, best_w, best_t, best_f);
	HuBlenTopo tp;
	/* the need of the tree as it stands: nothing is inserted here */
	if((rc = hu_add_check(fn, opts, n, cs_len, parent, blen, seq, n_query, qseq, false, 0, &tp)) != HU_OK) return rc;
	AddDev r;
	if((rc = add_dev_setup(r, fn, opts, n, cs_len, n_query, model, m)) != HU_OK) return rc;
	if(n_query == 0) return HU_OK;
	if((rc = r.sweep(n, parent, blen, seq)) != HU_OK) return rc;
	return r.score(n, tp.root, hu_add_start(n, parent, blen, opts->blen.min_len, opts->blen.max_len), n_query, qseq, t_star, f, best_w, best_t, best_f);
} catch(...) { return hu_catch_all("hu_tree_add_scores"); }

extern "C" int hu_tree_add_search(hu_add_opts* opts, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const hu_model_desc* model) try {
	const char* fn = "hu_tree_add_search";
	HuBlenModel m;
	int rc = add_model(fn, opts, model, &m);
	if(rc != HU_OK) return rc;
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	g_addTiming[0] = g_addTiming[1] = g_addTiming[2] = g_addTiming[3] = 0;
	const double t0 = now_s();
	if(opts->blen.host != 0 || opts->blen.device < 0) rc = hu_add_host_search_entry(fn, opts, n, cs_len, n_query, parent, blen, seq, child_off, child_idx, qseq, query_node, m, g_addTiming);
	else {
		HuBlenTopo tp;
		if((rc = hu_add_check(fn, opts, n, cs_len, parent, blen, seq, n_query, qseq, true, 0, &tp)) != HU_OK) return rc;
		AddDev r;
		if((rc = add_dev_setup(r, fn, opts, n + 2 * n_query, cs_len, n_query, model, m)) != HU_OK) return rc;
		HuAddOps ops;
		ops.fit = [&](int32_t nn, const int32_t* par, double* b, const int8_t* sq, double* ll) {
			r.release();                                       /* the fit holds messages of its own */
			hu_blen_opts bo = opts->blen;
			bo.rounds = nullptr; bo.rounds_cap = 0; bo.mem_budget = 0;
			const int rc2 = hu_tree_optimize_lengths(&bo, nn, cs_len, par, b, sq, model);
			*ll = bo.ll_final;
			return rc2;
		};
		ops.sweep = [&](int32_t nn, const int32_t* par, const double* b, const int8_t* sq, const HuBlenTopo&) { return r.sweep(nn, par, b, sq); };
		ops.score = [&](int32_t nn, int32_t root, const double*, double ts0, int32_t nq, const int8_t* rows, int32_t* bw, double* bt, double* bf) {
			return r.score(nn, root, ts0, nq, rows, nullptr, nullptr, bw, bt, bf);
		};
		rc = hu_add_rounds(fn, opts, n, cs_len, n_query, parent, blen, seq, child_off, child_idx, qseq, query_node, ops, g_addTiming);
	}
	g_addTiming[3] = now_s() - t0 - g_addTiming[0] - g_addTiming[1] - g_addTiming[2];
	return rc;
} catch(...) { return hu_catch_all("hu_tree_add_search"); }
