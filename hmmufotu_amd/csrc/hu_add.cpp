// hu_tree_add_scores and hu_tree_add_search: the entries and the device path of hmmufotu-amd-tree --ml-lengths
// --start-tree T --add.  The checks, the host path, the insertion and the round loop are hu_add_host.cpp's; the scoring kernels are
// hu_kern_add.h's; the messages come from the level sweeps of the build (hu_tree_sweep_*) and the fit from hu_tree_optimize_lengths.
// An insertion changes the topology, so every sweep of a round has a sweep handle of its own.  The need is held against the budget
// and the free memory before anything is allocated; the buffers of the scoring are released while a fit holds its own.
#include <cstring>
#include <vector>
#include "hu_tree_dev.h"
#include "hu_kern_add.h"

static thread_local double g_addTiming[4] = {0, 0, 0, 0};

extern "C" int hu_add_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_addTiming, sizeof(g_addTiming));
	return HU_OK;
}

namespace {
/* the buffers of the scoring behind the operations of a round; msg: the messages, for the nodes of the final tree */
struct AddDev {
	HuTreeDev msg; const char* fn; int32_t nCap = 0, L = 0; const hu_add_opts* o = nullptr; double lo = 0, hi = 0;
	size_t qCap = 0, nOutCap = 0, ratioCap = 0;
	double *dblen = nullptr, *ratio = nullptr, *vec = nullptr, *best = nullptr;   /* vec: tStar, f [qCap][n]; best: t, f [qCap] */
	int32_t* bestW = nullptr; int8_t* rowsDev = nullptr;
	~AddDev() { release(); }
	void release_slab() {
		(void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(best); (void) hipFree(bestW); (void) hipFree(rowsDev);
		ratio = vec = best = nullptr; bestW = nullptr; rowsDev = nullptr; qCap = nOutCap = ratioCap = 0;
	}
	void release() { release_slab(); (void) hipFree(dblen); dblen = nullptr; msg.release(); }
	int open(const char* fn_, const hu_add_opts* o_, int32_t n_final, int32_t cs_len, int32_t n_query, const hu_model_desc* model, const HuBlenModel& m) {
		fn = fn_; nCap = n_final; L = cs_len; o = o_; lo = o->blen.min_len; hi = o->blen.max_len;
		char what[96];
		snprintf(what, sizeof(what), "%d nodes of %d columns and %d new sequences", nCap, L, n_query);
		return msg.open(fn, o->blen, nCap, L, model, m, (size_t) hu_add_need(nCap, L, n_query), what);
	}
	/* the messages of the tree as it stands, and its lengths for the kernel */
	int sweep(int32_t n, const int32_t* parent, const double* blen, const int8_t* seq) {
		const int rc = msg.sweep(n, parent, blen, seq, true);
		if(rc != HU_OK) return rc;
		if(!dblen) TCHK(hipMalloc((void**) &dblen, (size_t) nCap * 8));
		TCHK(hipMemcpy(dblen, blen, (size_t) n * 8, hipMemcpyHostToDevice));
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
			if(ratioNeed) TCHK(hipMalloc((void**) &ratio, ratioNeed * 8));
			TCHK(hipMalloc((void**) &vec, slab * sN * 16)); TCHK(hipMalloc((void**) &best, slab * 16)); TCHK(hipMalloc((void**) &bestW, slab * 4));
			TCHK(hipMalloc((void**) &rowsDev, slab * sL));
			qCap = slab; nOutCap = slab * sN; ratioCap = ratioNeed;
		}
		for(size_t q0 = 0; q0 < (size_t) nq; q0 += slab) {
			const size_t k = std::min(slab, (size_t) nq - q0), tiles = (k + tile - 1) / tile;
			TCHK(hipMemcpy(rowsDev, qrows + q0 * sL, k * sL, hipMemcpyHostToDevice));
			TCHK(hipMemset(vec, 0, k * sN * 16));
			HuAddArgs a; memset(&a, 0, sizeof(a));
			a.up = msg.up; a.down = msg.down; a.blen = dblen; a.q = rowsDev; a.m = msg.dm; a.csLen = L; a.n = n; a.root = root; a.nq = (int32_t) k; a.tile = tile;
			a.lo = lo; a.hi = hi; a.t0 = t0; a.ratio = ratio; a.tStar = vec; a.f = vec + k * sN; a.bestW = bestW; a.bestT = best; a.bestF = best + k;
			(void) hipGetLastError();
			const dim3 grid((unsigned) n, (unsigned) tiles);
			if(L <= HU_BLEN_LDS_COLS) {
				const size_t lds = ((size_t) 3 * HU_ADD_WG + (size_t) 3 * sL) * 8;       /* at most 40,944 bytes */
				k_add_score<true><<<grid, HU_ADD_WG, lds>>>(a);
			}
			else k_add_score<false><<<grid, HU_ADD_WG, (size_t) 3 * HU_ADD_WG * 8>>>(a);
			TCHK(hipGetLastError());
			k_add_best<<<(unsigned) k, HU_ADD_WG>>>(a);
			TCHK(hipGetLastError());
			TCHK(hipDeviceSynchronize());
			if(ts && f) {
				TCHK(hipMemcpy(ts + q0 * sN, vec, k * sN * 8, hipMemcpyDeviceToHost));
				TCHK(hipMemcpy(f + q0 * sN, vec + k * sN, k * sN * 8, hipMemcpyDeviceToHost));
			}
			TCHK(hipMemcpy(bw + q0, bestW, k * 4, hipMemcpyDeviceToHost));
			TCHK(hipMemcpy(bt + q0, best, k * 8, hipMemcpyDeviceToHost));
			TCHK(hipMemcpy(bf + q0, best + k, k * 8, hipMemcpyDeviceToHost));
		}
		return HU_OK;
	}
};

}

extern "C" int hu_tree_add_scores(const hu_add_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t n_query, const int8_t* qseq, double* t_star, double* f, int32_t* best_w, double* best_t, double* best_f) try {
	const char* fn = "hu_tree_add_scores";
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "sequences are inserted", &m);
	if(rc != HU_OK) return rc;
	if((t_star == nullptr) != (f == nullptr) || (n_query > 0 && (!best_w || !best_t || !best_f))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	if(opts->blen.host != 0 || opts->blen.device < 0) return hu_add_host_scores_entry(fn, opts, n, cs_len, parent, blen, seq, m, n_query, qseq, t_star, f, best_w, best_t, best_f);
	HuBlenTopo tp;
	/* the need of the tree as it stands: nothing is inserted here */
	if((rc = hu_add_check(fn, opts, n, cs_len, parent, blen, seq, n_query, qseq, false, 0, &tp)) != HU_OK) return rc;
	AddDev r;
	if((rc = r.open(fn, opts, n, cs_len, n_query, model, m)) != HU_OK) return rc;
	if(n_query == 0) return HU_OK;
	if((rc = r.sweep(n, parent, blen, seq)) != HU_OK) return rc;
	return r.score(n, tp.root, hu_add_start(n, parent, blen, opts->blen.min_len, opts->blen.max_len), n_query, qseq, t_star, f, best_w, best_t, best_f);
} catch(...) { return hu_catch_all("hu_tree_add_scores"); }

extern "C" int hu_tree_add_search(hu_add_opts* opts, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const hu_model_desc* model) try {
	const char* fn = "hu_tree_add_search";
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "sequences are inserted", &m);
	if(rc != HU_OK) return rc;
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	g_addTiming[0] = g_addTiming[1] = g_addTiming[2] = g_addTiming[3] = 0;
	const double t0 = hu_now_s();
	if(opts->blen.host != 0 || opts->blen.device < 0) rc = hu_add_host_search_entry(fn, opts, n, cs_len, n_query, parent, blen, seq, child_off, child_idx, qseq, query_node, m, g_addTiming);
	else {
		HuBlenTopo tp;
		if((rc = hu_add_check(fn, opts, n, cs_len, parent, blen, seq, n_query, qseq, true, 0, &tp)) != HU_OK) return rc;
		AddDev r;
		if((rc = r.open(fn, opts, n + 2 * n_query, cs_len, n_query, model, m)) != HU_OK) return rc;
		HuAddOps ops;
		ops.fit = [&](int32_t nn, const int32_t* par, double* b, const int8_t* sq, double* ll) { return hu_search_fit_device(r, opts->blen, nn, par, b, sq, ll); };
		ops.sweep = [&](int32_t nn, const int32_t* par, const double* b, const int8_t* sq, const HuBlenTopo&) { return r.sweep(nn, par, b, sq); };
		ops.score = [&](int32_t nn, int32_t root, const double*, double ts0, int32_t nq, const int8_t* rows, int32_t* bw, double* bt, double* bf) {
			return r.score(nn, root, ts0, nq, rows, nullptr, nullptr, bw, bt, bf);
		};
		rc = hu_add_rounds(fn, opts, n, cs_len, n_query, parent, blen, seq, child_off, child_idx, qseq, query_node, ops, g_addTiming);
	}
	g_addTiming[3] = hu_now_s() - t0 - g_addTiming[0] - g_addTiming[1] - g_addTiming[2];
	return rc;
} catch(...) { return hu_catch_all("hu_tree_add_search"); }
