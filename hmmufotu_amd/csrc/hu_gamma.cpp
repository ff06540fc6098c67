// hu_tree_gamma_loglik, hu_tree_gamma_branch_scores, hu_tree_gamma_branch_step and hu_tree_gamma_fit: the entries and
// the device path of hmmufotu-amd-tree --ml-lengths --gamma K.  The rates, the checks, the host path and the passes of the fit are
// hu_gamma_host.cpp's; the step kernel is hu_kern_gamma.h's; the messages of all categories come from the level sweeps over the
// categories (hu_tree_sweep_cat) and the column values of a category from hu_tree_loglik.  The need is held against the budget and the
// free memory before anything is allocated.
#include <cstring>
#include <memory>
#include <vector>
#include "hu_tree_dev.h"
#include "hu_kern_gamma.h"

static thread_local double g_gammaTiming[5] = {0, 0, 0, 0, 0};

extern "C" int hu_gamma_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_gammaTiming, sizeof(g_gammaTiming));
	return HU_OK;
}

namespace {
struct GammaDev : HuGammaRun {
	const char* fn; int32_t n, L, K, device; bool reruns; const int32_t* parent; hu_model_desc model; const HuBlenTopo& tp; HuBlenModel m; double lo, hi;
	hu_tree_sweep* sw = nullptr; std::vector<int8_t> rows; std::vector<double> lenCat, rate;
	double *up = nullptr, *down = nullptr, *scratch = nullptr, *vec = nullptr, *lr = nullptr; int32_t* iters = nullptr;   /* vec: t, tStar, f, d1, d2 [5][n] */
	size_t cells4;
	GammaDev(const char* fn_, const hu_gamma_opts& o, const HuBlenTopo& t, const HuBlenModel& hm, int32_t cs_len, const int32_t* par, const int8_t* seq, const hu_model_desc* md)
		: fn(fn_), n(t.n), L(cs_len), K(o.k), device(o.blen.device), reruns(o.sweep_reruns != 0), parent(par), model(*md), tp(t), m(hm), lo(o.blen.min_len), hi(o.blen.max_len),
		  rows(seq, seq + (size_t) t.n * (size_t) cs_len), lenCat((size_t) o.k * (size_t) t.n), rate((size_t) o.k, 1.0), cells4((size_t) t.n * (size_t) cs_len * 4) {}
	~GammaDev() override {
		if(sw) hu_tree_sweep_destroy(sw);
		(void) hipFree(up); (void) hipFree(down); (void) hipFree(scratch); (void) hipFree(vec); (void) hipFree(lr); (void) hipFree(iters);
	}
	int open() {
		if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
		TCHK(hipSetDevice(device));
		size_t freeB = 0, totB = 0;
		TCHK(hipMemGetInfo(&freeB, &totB));
		const size_t need = (size_t) hu_gamma_need(n, L, K);
		if(need > freeB) {
			hu_set_error("%s: %d nodes of %d columns in %d rate categories need %zu bytes of device memory (%zu of them for the messages), %zu bytes are free", fn, n, L, K, need,
				cells4 * 16 * (size_t) K, freeB);
			return HU_ERR_NOMEM;
		}
		TCHK(hipMalloc((void**) &up, cells4 * 8 * (size_t) K)); TCHK(hipMalloc((void**) &down, cells4 * 8 * (size_t) K));
		if(!hu_gamma_in_lds(K, L)) TCHK(hipMalloc((void**) &scratch, (size_t) hu_gamma_slab(n) * 32 * (size_t) K * (size_t) L));
		TCHK(hipMalloc((void**) &vec, (size_t) n * 40)); TCHK(hipMalloc((void**) &iters, (size_t) n * 4)); TCHK(hipMalloc((void**) &lr, (size_t) 3 * K * 8));
		return HU_OK;
	}
	int set_rates(const double* r) override {
		rate.assign(r, r + K);
		double h[3 * HU_MAX_DGK];
		hu_gamma_lr(m, K, r, h);
		TCHK(hipMemcpy(lr, h, (size_t) 3 * K * 8, hipMemcpyHostToDevice));
		return HU_OK;
	}
	int sweep(const double* blen, bool withDown) override {
		const size_t N = (size_t) n;
		for(int32_t c = 0; c < K; ++c) for(size_t u = 0; u < N; ++u) lenCat[(size_t) c * N + u] = rate[(size_t) c] * blen[u];
		const bool first = !sw;
		int rc = HU_OK;
		/* the first sweep sends the topology and the rows; they stay on the device for the later ones */
		if(first && (rc = hu_tree_sweep_create(n, L, parent, lenCat.data(), device, &sw)) != HU_OK) return rc;
		if(!reruns) rc = hu_tree_sweep_cat(sw, &model, first ? rows.data() : nullptr, K, lenCat.data(), L, up, withDown ? down : nullptr);
		else for(int32_t c = 0; c < K && rc == HU_OK; ++c) {
			double* dn = withDown ? down + cells4 * (size_t) c : nullptr;
			rc = first && c == 0 ? hu_tree_sweep_window(sw, &model, rows.data(), 0, L, up, dn) : hu_tree_sweep_rerun(sw, &model, lenCat.data() + (size_t) c * N, L, up + cells4 * (size_t) c, dn);
		}
		if(first) std::vector<int8_t>().swap(rows);
		return rc;
	}
	int loglik(double* per_col, double* per_cat, double* ll) override {
		std::vector<double> v((size_t) K * (size_t) L);
		for(int32_t c = 0; c < K; ++c) {
			double s = 0;
			const int rc = hu_tree_loglik(device, n, L, tp.root, &model, up + cells4 * (size_t) c, v.data() + (size_t) c * (size_t) L, &s);
			if(rc != HU_OK) return rc;
		}
		if(per_cat) memcpy(per_cat, v.data(), v.size() * 8);
		double sum = 0;
		for(int64_t j = 0; j < L; ++j) { const double x = hu_gamma_logmean(v.data() + j, L, K); if(per_col) per_col[j] = x; sum += x; }
		*ll = sum;
		return HU_OK;
	}
	int step(const double* t, double* tStar, double* f, double* d1, double* d2, uint8_t* capped, int64_t* nCap) override {
		*nCap = 0;
		const size_t N = (size_t) n;
		TCHK(hipMemcpy(vec, t, N * 8, hipMemcpyHostToDevice));
		TCHK(hipMemset(vec + N, 0, N * 32)); TCHK(hipMemset(iters, 0, N * 4));
		HuGammaArgs a; memset(&a, 0, sizeof(a));
		a.up = up; a.down = down; a.t = vec; a.lr = lr; a.csLen = L; a.n = n; a.root = tp.root; a.doStep = tStar ? 1 : 0; a.K = K; a.lo = lo; a.hi = hi; a.logK = log((double) K);
		a.scratch = scratch; a.tStar = vec + N; a.f = vec + 2 * N; a.d1 = vec + 3 * N; a.d2 = vec + 4 * N; a.iters = iters; a.m = m;
		(void) hipGetLastError();
		if(hu_gamma_in_lds(K, L)) k_gamma_step<true><<<(unsigned) n, HU_BLEN_WG, hu_gamma_lds_bytes(K, L)>>>(a);
		else {
			/* a slab of branches per launch: the launches run one after another on the stream, so they share the scratch */
			const int64_t slab = hu_gamma_slab(n);
			const size_t lds = ((size_t) 3 * HU_BLEN_WG + (size_t)(9 * K + (9 * K & 1))) * 8;
			for(int64_t u0 = 0; u0 < n; u0 += slab) {
				a.node0 = (int32_t) u0;
				k_gamma_step<false><<<(unsigned) std::min<int64_t>(slab, n - u0), HU_BLEN_WG, lds>>>(a);
			}
		}
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

/* the checks, the model, and either half under the rates of the options' alpha (0: alpha = 1) */
struct GammaSetup {
	HuBlenTopo tp; HuBlenModel m; std::unique_ptr<HuGammaRun> run;
	int open(const char* fn, const hu_gamma_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq, const hu_model_desc* model) {
		if(!o || !model) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
		int rc = hu_gamma_check(fn, o, n, cs_len, parent, blen, seq, model->dg_k, &tp);
		if(rc != HU_OK) return rc;
		HuModelDev d;
		if((rc = hu_model_prepare(model, &d)) != HU_OK) return rc;
		hu_blen_model_set(&m, d.U, d.lam, d.U1);
		if(o->blen.host != 0 || o->blen.device < 0) run.reset(hu_gamma_host_run(tp, m, o->k, cs_len, parent, seq, o->blen.min_len, o->blen.max_len));
		else {
			std::unique_ptr<GammaDev> dev(new GammaDev(fn, *o, tp, m, cs_len, parent, seq, model));
			if((rc = dev->open()) != HU_OK) return rc;
			run = std::move(dev);
		}
		double rate[HU_MAX_DGK];
		if((rc = hu_gamma_rates(o->k, o->alpha == 0.0 ? 1.0 : o->alpha, rate)) != HU_OK) return rc;
		return run->set_rates(rate);
	}
};
}

extern "C" int hu_tree_gamma_loglik(const hu_gamma_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* per_col, double* per_cat, double* ll) try {
	const char* fn = "hu_tree_gamma_loglik";
	if(!ll) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	GammaSetup s;
	int rc = s.open(fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if((rc = s.run->sweep(blen, false)) != HU_OK) return rc;
	return s.run->loglik(per_col, per_cat, ll);
} catch(...) { return hu_catch_all("hu_tree_gamma_loglik"); }

extern "C" int hu_tree_gamma_branch_scores(const hu_gamma_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, const double* t, double* f, double* d1, double* d2) try {
	const char* fn = "hu_tree_gamma_branch_scores";
	if(!f || !d1 || !d2) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	GammaSetup s;
	int rc = s.open(fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if(t) for(int32_t u = 0; u < n; ++u) if(u != s.tp.root && (!(t[u] >= 0) || t[u] - t[u] != 0.0)) { hu_set_error("%s: t of node %d is %g", fn, u, t[u]); return HU_ERR_ARG; }
	if((rc = s.run->sweep(blen, true)) != HU_OK) return rc;
	int64_t nCap = 0;
	return s.run->step(t ? t : blen, nullptr, f, d1, d2, nullptr, &nCap);
} catch(...) { return hu_catch_all("hu_tree_gamma_branch_scores"); }

extern "C" int hu_tree_gamma_branch_step(hu_gamma_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* t_star, double* f, double* d1, double* d2, uint8_t* capped) try {
	const char* fn = "hu_tree_gamma_branch_step";
	if(!t_star) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	GammaSetup s;
	int rc = s.open(fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	if((rc = s.run->sweep(blen, true)) != HU_OK) return rc;
	int64_t nCap = 0;
	rc = s.run->step(blen, t_star, f, d1, d2, capped, &nCap);
	opts->n_capped = nCap;
	return rc;
} catch(...) { return hu_catch_all("hu_tree_gamma_branch_step"); }

/* the phases of a round one by one, reps times each, on the device: seconds [reps][3] = a full sweep (up and down), a step, a trial (the
 * up sweep and the log-likelihood), by the host clock around calls that end in a synchronise.  The first repetition also sends the rows */
extern "C" int hu_gamma_profile(const hu_gamma_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t reps, double* seconds) try {
	const char* fn = "hu_gamma_profile";
	if(reps < 1 || !seconds || !opts || opts->blen.host != 0 || opts->blen.device < 0) { hu_set_error("%s: the repetitions, a place for their seconds, and the device path", fn); return HU_ERR_ARG; }
	GammaSetup s;
	int rc = s.open(fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	std::vector<double> ts((size_t) n);
	for(int32_t r = 0; r < reps; ++r) {
		double t0 = hu_now_s(), ll = 0;
		int64_t nCap = 0;
		if((rc = s.run->sweep(blen, true)) != HU_OK) return rc;
		seconds[3 * r] = hu_now_s() - t0; t0 = hu_now_s();
		if((rc = s.run->step(blen, ts.data(), nullptr, nullptr, nullptr, nullptr, &nCap)) != HU_OK) return rc;
		seconds[3 * r + 1] = hu_now_s() - t0; t0 = hu_now_s();
		if((rc = s.run->sweep(blen, false)) != HU_OK || (rc = s.run->loglik(nullptr, nullptr, &ll)) != HU_OK) return rc;
		seconds[3 * r + 2] = hu_now_s() - t0;
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_gamma_profile"); }

extern "C" int hu_tree_gamma_fit(hu_gamma_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, double* blen, const int8_t* seq,
		const hu_model_desc* model) try {
	const char* fn = "hu_tree_gamma_fit";
	GammaSetup s;
	const int rc = s.open(fn, opts, n, cs_len, parent, blen, seq, model);
	if(rc != HU_OK) return rc;
	return hu_gamma_fit_run(fn, opts, n, s.tp.root, blen, *s.run, g_gammaTiming);
} catch(...) { return hu_catch_all("hu_tree_gamma_fit"); }
