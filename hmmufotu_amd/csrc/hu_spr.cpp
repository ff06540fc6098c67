// hu_tree_spr_scores and hu_tree_spr_search: the entries and the device path of hmmufotu-amd-tree --ml-lengths --spr.
// The checks, the walk, the host path, the selection and the round loop are hu_spr_host.cpp's; the scoring kernel is hu_kern_spr.h's;
// the messages come from the level sweeps of the build (hu_tree_sweep_*), the fit from hu_tree_optimize_lengths and the objective from
// hu_tree_loglik.  A move changes the topology, so every sweep of a round has a sweep handle of its own.  The need is held against the
// budget and the free memory before anything is allocated; the buffers of the scoring are released while a fit holds its own.
#include <cstring>
#include <vector>
#include "hu_tree_dev.h"
#include "hu_kern_spr.h"

static thread_local double g_sprTiming[4] = {0, 0, 0, 0};

extern "C" int hu_spr_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_sprTiming, sizeof(g_sprTiming));
	return HU_OK;
}

namespace {
/* the buffers of the scoring behind the operations of a round; msg: the messages */
struct SprDev {
	HuTreeDev msg; const char* fn; int32_t n = 0, L = 0, radius = 0; double lo = 0, hi = 0;
	size_t nodeCap = 0, recCap = 0, outCap = 0;
	double *stack = nullptr, *ratio = nullptr, *vec = nullptr, *f0 = nullptr;   /* vec: tStar [outCap], f [outCap] */
	int32_t* iters = nullptr; HuSprNode* nodes = nullptr; HuSprRec* recs = nullptr;
	~SprDev() { release(); }
	void release_slab() {
		(void) hipFree(stack); (void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(f0); (void) hipFree(iters); (void) hipFree(nodes); (void) hipFree(recs);
		stack = ratio = vec = f0 = nullptr; iters = nullptr; nodes = nullptr; recs = nullptr; nodeCap = recCap = outCap = 0;
	}
	void release() { release_slab(); msg.release(); }
	int open(const char* fn_, const hu_spr_opts* o, int32_t n_, int32_t cs_len, const hu_model_desc* model, const HuBlenModel& m) {
		fn = fn_; n = n_; L = cs_len; radius = o->radius; lo = o->blen.min_len; hi = o->blen.max_len;
		char what[80];
		snprintf(what, sizeof(what), "%d nodes of %d columns at radius %d", n, L, radius);
		return msg.open(fn, o->blen, n, L, model, m, (size_t) hu_spr_need(n, L, radius), what);
	}
	/* one slab; the messages are those of the last full sweep */
	int score(const HuSprNode* nd, size_t nNodes, const HuSprRec* rc, size_t nRecs, int64_t recBase, int64_t outBase, size_t nOut, double* ts, double* f, double* f0h) {
		if(nNodes == 0) return HU_OK;
		/* nothing a record names lies outside the messages, the stack or the outputs */
		for(size_t b = 0; b < nNodes; ++b) {
			const HuSprNode& x = nd[b];
			if(x.v < 0 || x.v >= n || x.nRec < 0 || x.recOff < recBase || (size_t)(x.recOff - recBase) + (size_t) x.nRec > nRecs || x.outOff < outBase) {
				hu_set_error("%s: a node record points outside its slab", fn); return HU_ERR_STATE; }
			for(int32_t i = 0; i < x.nRec; ++i) {
				const HuSprRec& r = rc[(size_t)(x.recOff - recBase) + (size_t) i];
				auto bad = [&](int32_t id) { return id < 0 || id >= 2 * n + radius; };
				if(r.dst >= radius || (r.dst >= 0 && (bad(r.src0) || (r.src1 >= 0 && bad(r.src1)))) || (r.tnode >= 0 && (bad(r.sa) || bad(r.sb) || r.out < 0 ||
						(size_t)(x.outOff - outBase) + (size_t) r.out >= nOut))) {
					hu_set_error("%s: a step record points outside the messages", fn); return HU_ERR_STATE; }
			}
		}
		if(nNodes > nodeCap || nRecs > recCap || nOut > outCap) {
			release_slab();
			const size_t sL = (size_t) L;
			TCHK(hipMalloc((void**) &stack, nNodes * (size_t) radius * sL * 32));
			if(L > HU_BLEN_LDS_COLS) TCHK(hipMalloc((void**) &ratio, nNodes * 24 * sL));
			TCHK(hipMalloc((void**) &vec, nOut * 16)); TCHK(hipMalloc((void**) &iters, nOut * 4)); TCHK(hipMalloc((void**) &f0, nNodes * 8));
			TCHK(hipMalloc((void**) &nodes, nNodes * sizeof(HuSprNode))); TCHK(hipMalloc((void**) &recs, nRecs * sizeof(HuSprRec)));
			nodeCap = nNodes; recCap = nRecs; outCap = nOut;
		}
		TCHK(hipMemcpy(nodes, nd, nNodes * sizeof(HuSprNode), hipMemcpyHostToDevice));
		TCHK(hipMemcpy(recs, rc, nRecs * sizeof(HuSprRec), hipMemcpyHostToDevice));
		TCHK(hipMemset(vec, 0, nOut * 16)); TCHK(hipMemset(iters, 0, nOut * 4)); TCHK(hipMemset(f0, 0, nNodes * 8));
		HuSprArgs a; memset(&a, 0, sizeof(a));
		a.up = msg.up; a.down = msg.down; a.nodes = nodes; a.recs = recs; a.m = msg.dm; a.csLen = L; a.recBase = recBase; a.outBase = outBase;
		a.n = n; a.nNodes = (int32_t) nNodes; a.slots = radius; a.lo = lo; a.hi = hi;
		a.stack = stack; a.ratio = ratio; a.tStar = vec; a.f = vec + nOut; a.f0 = f0; a.iters = iters;
		(void) hipGetLastError();
		if(L <= HU_BLEN_LDS_COLS) {
			const size_t lds = ((size_t) 3 * HU_SPR_WG + (size_t) 3 * L) * 8;       /* at most 40,944 bytes */
			k_spr_score<true><<<(unsigned) nNodes, HU_SPR_WG, lds>>>(a);
		}
		else k_spr_score<false><<<(unsigned) nNodes, HU_SPR_WG, (size_t) 3 * HU_SPR_WG * 8>>>(a);
		TCHK(hipGetLastError());
		TCHK(hipDeviceSynchronize());
		TCHK(hipMemcpy(ts, vec, nOut * 8, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(f, vec + nOut, nOut * 8, hipMemcpyDeviceToHost));
		TCHK(hipMemcpy(f0h, f0, nNodes * 8, hipMemcpyDeviceToHost));
		return HU_OK;
	}
	HuSprSlabFn slab() {
		return [this](const HuSprNode* nd, size_t nNodes, const HuSprRec* rc, size_t nRecs, int64_t recBase, int64_t outBase, size_t nOut, double* ts, double* f, double* f0h) {
			return score(nd, nNodes, rc, nRecs, recBase, outBase, nOut, ts, f, f0h);
		};
	}
};

}

extern "C" int hu_tree_spr_scores(const hu_spr_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t node_cap, int64_t target_cap, int32_t* n_pruned, int64_t* n_targets, int64_t* skipped,
		int32_t* prune_node, int64_t* v_off, double* base_t, double* base_f, double* f_at_blen,
		int32_t* target_node, int32_t* dist, double* t_star, double* f) try {
	const char* fn = "hu_tree_spr_scores";
	if(!n_pruned || !n_targets || !skipped || node_cap < 0 || target_cap < 0 || (node_cap > 0 && (!prune_node || !v_off || !base_t || !base_f || !f_at_blen)) ||
			(target_cap > 0 && (!target_node || !dist || !t_star || !f))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "the search runs", &m);
	if(rc != HU_OK) return rc;
	const bool host = opts->blen.host != 0 || opts->blen.device < 0;
	HuSprScores sc;
	/* the sizes first: held against the caps before anything is computed */
	HuBlenTopo tp;
	if((rc = hu_spr_check(fn, opts, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
	if((rc = hu_spr_scores(fn, opts, tp, cs_len, parent, blen, true, HuSprSlabFn(), &sc)) != HU_OK) return rc;
	*n_pruned = (int32_t) sc.v.size(); *n_targets = sc.off.back(); *skipped = sc.skipped;
	if(node_cap == 0 && target_cap == 0) return HU_OK;
	if((int64_t) sc.v.size() > node_cap || sc.off.back() > target_cap) {
		hu_set_error("%s: %zu prunable nodes with %lld targets, the outputs hold %d and %lld", fn, sc.v.size(), (long long) sc.off.back(), node_cap, (long long) target_cap);
		return HU_ERR_ARG;
	}
	if(host) rc = hu_spr_host_scores_entry(fn, opts, n, cs_len, parent, blen, seq, m, false, &sc);
	else {
		SprDev r;
		if((rc = r.open(fn, opts, n, cs_len, model, m)) != HU_OK) return rc;
		if(sc.v.empty()) { if(v_off) v_off[0] = 0; return HU_OK; }
		if((rc = r.msg.sweep(n, parent, blen, seq, true)) != HU_OK) return rc;
		rc = hu_spr_scores(fn, opts, tp, cs_len, parent, blen, false, r.slab(), &sc);
	}
	if(rc != HU_OK) return rc;
	const size_t P = sc.v.size(), T = sc.w.size();
	if(v_off) memcpy(v_off, sc.off.data(), (P + 1) * 8);
	if(P) { memcpy(prune_node, sc.v.data(), P * 4); memcpy(base_t, sc.baseT.data(), P * 8); memcpy(base_f, sc.baseF.data(), P * 8); memcpy(f_at_blen, sc.f0.data(), P * 8); }
	if(T) { memcpy(target_node, sc.w.data(), T * 4); memcpy(dist, sc.dist.data(), T * 4); memcpy(t_star, sc.t.data(), T * 8); memcpy(f, sc.f.data(), T * 8); }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_tree_spr_scores"); }

extern "C" int hu_tree_spr_search(hu_spr_opts* opts, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const hu_model_desc* model) try {
	const char* fn = "hu_tree_spr_search";
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "the search runs", &m);
	if(rc != HU_OK) return rc;
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	g_sprTiming[0] = g_sprTiming[1] = g_sprTiming[2] = g_sprTiming[3] = 0;
	const double t0 = hu_now_s();
	if(opts->blen.host != 0 || opts->blen.device < 0) rc = hu_spr_host_search_entry(fn, opts, n, cs_len, parent, blen, seq, child_off, child_idx, m, g_sprTiming);
	else {
		HuBlenTopo tp;
		if((rc = hu_spr_check(fn, opts, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
		SprDev r;
		if((rc = r.open(fn, opts, n, cs_len, model, m)) != HU_OK) return rc;
		HuSprOps ops;
		ops.fit = [&](const int32_t* par, double* b, double* ll) { return hu_search_fit_device(r, opts->blen, n, par, b, seq, ll); };
		ops.score = [&](const int32_t* par, const double* b, const HuBlenTopo& tpr, HuSprScores* out) {
			int rc2 = r.msg.sweep(n, par, b, seq, true);
			if(rc2 == HU_OK) rc2 = hu_spr_scores(fn, opts, tpr, cs_len, par, b, false, r.slab(), out);
			return rc2;
		};
		ops.trial = [&](const int32_t* par, const double* b, double* ll) { return r.msg.trial(n, par, b, seq, ll); };
		rc = hu_spr_rounds(fn, opts, n, cs_len, parent, blen, seq, child_off, child_idx, ops, g_sprTiming);
	}
	g_sprTiming[3] = hu_now_s() - t0 - g_sprTiming[0] - g_sprTiming[1] - g_sprTiming[2];
	return rc;
} catch(...) { return hu_catch_all("hu_tree_spr_search"); }
