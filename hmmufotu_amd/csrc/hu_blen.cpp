// hu_tree_branch_scores, hu_tree_branch_step and hu_tree_optimize_lengths: the entries and the device path of
// hmmufotu-amd-tree --ml-lengths.  The checks, the host path and the round loop are hu_blen_host.cpp's; the step kernel is
// hu_kern_blen.h's; the messages come from the level sweeps of the build (hu_tree_sweep_*) and the objective from hu_tree_loglik.
// The need is held against the budget and the free memory before anything is allocated.
#include <cstring>
#include <vector>
#include "hu_tree_dev.h"
#include "hu_kern_blen.h"

static thread_local double g_blenTiming[4] = {0, 0, 0, 0};

extern "C" int hu_blen_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_blenTiming, sizeof(g_blenTiming));
	return HU_OK;
}

namespace {
/* either half behind the three operations of a round */
struct BlenRun {
	const char* fn; int32_t n = 0, L = 0; const int32_t* parent = nullptr; const int8_t* seq = nullptr; hu_model_desc model;
	HuBlenTopo tp; HuBlenModel m; double lo = 0, hi = 0;
	bool host = true; int device = 0;
	/* host */
	std::vector<double> hUp, hDown;
	/* device */
	hu_tree_sweep* sw = nullptr; std::vector<int8_t> rows;
	double *up = nullptr, *down = nullptr, *ratio = nullptr, *vec = nullptr; int32_t* iters = nullptr;   /* vec: t, tStar, f, d1, d2 [5][n] */
	~BlenRun() {
		if(host) return;                                   /* the host path never touches the runtime */
		if(sw) hu_tree_sweep_destroy(sw);
		(void) hipFree(up); (void) hipFree(down); (void) hipFree(ratio); (void) hipFree(vec); (void) hipFree(iters);
	}
	int open() {
		const size_t cells = (size_t) n * (size_t) L;
		if(host) { hUp.resize(cells * 4); hDown.resize(cells * 4); return HU_OK; }
		if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
		TCHK(hipSetDevice(device));
		size_t freeB = 0, totB = 0;
		TCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = (size_t) hu_blen_need(n, L);
		if(need > freeB) {
			hu_set_error("%s: %d nodes of %d columns need %zu bytes of device memory (%zu of them for the messages), %zu bytes are free", fn, n, L, need, cells * 64, freeB);
			return HU_ERR_NOMEM;
		}
		TCHK(hipMalloc((void**) &up, cells * 32)); TCHK(hipMalloc((void**) &down, cells * 32));
		if(L > HU_BLEN_LDS_COLS) TCHK(hipMalloc((void**) &ratio, cells * 24));
		TCHK(hipMalloc((void**) &vec, (size_t) n * 40)); TCHK(hipMalloc((void**) &iters, (size_t) n * 4));
		rows.assign(seq, seq + cells);
		return HU_OK;
	}
	int sweep(const double* blen, bool withDown) {
		if(host) { hu_blen_host_sweep(tp, m, parent, L, blen, seq, hUp.data(), withDown ? hDown.data() : nullptr); return HU_OK; }
		if(!sw) {
			/* the first sweep sends the topology and the rows; they stay on the device for the later ones */
			int rc = hu_tree_sweep_create(n, L, parent, blen, device, &sw);
			if(rc == HU_OK) rc = hu_tree_sweep_window(sw, &model, rows.data(), 0, L, up, withDown ? down : nullptr);
			std::vector<int8_t>().swap(rows);
			return rc;
		}
		return hu_tree_sweep_rerun(sw, &model, blen, L, up, withDown ? down : nullptr);
	}
	int loglik(double* ll) {
		if(host) { *ll = hu_blen_host_loglik(m, L, hUp.data() + (size_t) tp.root * L * 4); return HU_OK; }
		return hu_tree_loglik(device, n, L, tp.root, &model, up, nullptr, ll);
	}
	/* scores at t, and with tStar the step; the messages are those of the last full sweep */
	int step(const double* t, double* tStar, double* f, double* d1, double* d2, uint8_t* capped, int64_t* nCap) {
		*nCap = 0;
		if(host) { *nCap = hu_blen_host_step(tp, m, L, t, hUp.data(), hDown.data(), lo, hi, tStar, f, d1, d2, capped); return HU_OK; }
		const size_t N = (size_t) n;
		TCHK(hipMemcpy(vec, t, N * 8, hipMemcpyHostToDevice));
		TCHK(hipMemset(vec + N, 0, N * 32)); TCHK(hipMemset(iters, 0, N * 4));
		HuBlenArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.t = vec; a.csLen = L; a.n = n; a.root = tp.root; a.doStep = tStar ? 1 : 0; a.lo = lo; a.hi = hi;
		a.ratio = ratio; a.tStar = vec + N; a.f = vec + 2 * N; a.d1 = vec + 3 * N; a.d2 = vec + 4 * N; a.iters = iters; a.m = m;
		(void) hipGetLastError();
		if(L <= HU_BLEN_LDS_COLS) {
			const size_t lds = ((size_t) 3 * HU_BLEN_WG + (size_t) 3 * L) * 8;     /* at most 40,944 bytes */
			k_blen_step<true><<<(unsigned) n, HU_BLEN_WG, lds>>>(a);
		}
		else k_blen_step<false><<<(unsigned) n, HU_BLEN_WG, (size_t) 3 * HU_BLEN_WG * 8>>>(a);
		TCHK(hipGetLastError());
		TCHK(hipDeviceSynchronize());
		std::vector<double> out(N * 4); std::vector<int32_t> it(N);
		TCHK(hipMemcpy(out.data(), vec + N, N * 32, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(it.data(), iters, N * 4, hipMemcpyDeviceToHost));
		for(size_t u = 0; u < N; ++u) {
			const bool cap = it[u] > HU_BLEN_MAX_NEWTON;
			if(tStar) tStar[u] = (int32_t) u == tp.root ? t[u] : out[u];
			if(f) f[u] = out[N + u];
			if(d1) d1[u] = out[2 * N + u];
			if(d2) d2[u] = out[3 * N + u];
			if(capped) capped[u] = cap ? 1 : 0;
			if(cap) ++*nCap;
		}
		return HU_OK;
	}
};

int blen_setup(BlenRun& r, const char* fn, const hu_blen_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model) {
	if(!o || !model) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	int rc = hu_blen_check(fn, o, n, cs_len, parent, blen, seq, model->dg_k, &r.tp);
	if(rc != HU_OK) return rc;
	HuModelDev d;
	if((rc = hu_model_prepare(model, &d)) != HU_OK) return rc;
	hu_blen_model_set(&r.m, d.U, d.lam, d.U1);
	r.fn = fn; r.n = n; r.L = cs_len; r.parent = parent; r.seq = seq; r.model = *model; r.lo = o->min_len; r.hi = o->max_len;
	r.host = o->host != 0 || o->device < 0; r.device = o->device;
	return r.open();
}
}

extern "C" int hu_tree_branch_scores(const hu_blen_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, const double* t, double* f, double* d1, double* d2) try {
	const char* fn = "hu_tree_branch_scores";
	if(!f || !d1 || !d2) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	BlenRun r;
	int rc = blen_setup(r, fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if(t) for(int32_t u = 0; u < n; ++u) if(u != r.tp.root && (!(t[u] >= 0) || t[u] - t[u] != 0.0)) { hu_set_error("%s: t of node %d is %g", fn, u, t[u]); return HU_ERR_ARG; }
	if((rc = r.sweep(blen, true)) != HU_OK) return rc;
	int64_t nCap = 0;
	return r.step(t ? t : blen, nullptr, f, d1, d2, nullptr, &nCap);
} catch(...) { return hu_catch_all("hu_tree_branch_scores"); }

extern "C" int hu_tree_branch_step(hu_blen_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* t_star, double* f, double* d1, double* d2, uint8_t* capped) try {
	const char* fn = "hu_tree_branch_step";
	if(!t_star) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	BlenRun r;
	int rc = blen_setup(r, fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if((rc = r.sweep(blen, true)) != HU_OK) return rc;
	int64_t nCap = 0;
	rc = r.step(blen, t_star, f, d1, d2, capped, &nCap);
	opts->n_capped = nCap;
	return rc;
} catch(...) { return hu_catch_all("hu_tree_branch_step"); }

extern "C" int hu_tree_optimize_lengths(hu_blen_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, double* blen, const int8_t* seq,
		const hu_model_desc* model) try {
	const char* fn = "hu_tree_optimize_lengths";
	BlenRun r;
	int rc = blen_setup(r, fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if(opts->rounds_cap < 0 || (opts->rounds_cap > 0 && !opts->rounds)) { hu_set_error("%s: %d round records without a place for them", fn, opts->rounds_cap); return HU_ERR_ARG; }
	HuBlenOps ops;
	ops.sweep = [&](const double* b, bool withDown) { return r.sweep(b, withDown); };
	ops.loglik = [&](double* ll) { return r.loglik(ll); };
	ops.step = [&](const double* b, double* ts, int64_t* nCap) { return r.step(b, ts, nullptr, nullptr, nullptr, nullptr, nCap); };
	g_blenTiming[0] = g_blenTiming[1] = g_blenTiming[2] = g_blenTiming[3] = 0;
	const double t0 = hu_now_s();
	rc = hu_blen_rounds(fn, opts, n, r.tp.root, blen, ops, g_blenTiming);
	g_blenTiming[3] = hu_now_s() - t0 - g_blenTiming[0] - g_blenTiming[1] - g_blenTiming[2];
	return rc;
} catch(...) { return hu_catch_all("hu_tree_optimize_lengths"); }
