// hu_tree_nni_scores and hu_tree_nni_search: the entries and the device path of hmmufotu-amd-tree --ml-lengths --nni.
// The checks, the host path, the selection and the round loop are hu_nni_host.cpp's; the scoring kernel is hu_kern_nni.h's; the
// messages come from the level sweeps of the build (hu_tree_sweep_*), the fit from hu_tree_optimize_lengths and the objective from
// hu_tree_loglik.  A swap changes the topology, so every sweep of a round has a sweep handle of its own.  The need is held against the
// budget and the free memory before anything is allocated; the buffers of the scoring are released while a fit holds its own.
#include <cstring>
#include <vector>
#include "hu_common.h"
#include "hu_nni_dev.h"

static thread_local double g_nniTiming[4] = {0, 0, 0, 0};

extern "C" int hu_nni_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_nniTiming, sizeof(g_nniTiming));
	return HU_OK;
}

extern "C" int hu_tree_nni_scores(const hu_nni_opts* opts, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, double* f0) try {
	const char* fn = "hu_tree_nni_scores";
	if(!n_edges || !skipped || edge_cap < 0 || (edge_cap > 0 && (!edge_node || !t_star || !f || !f0))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "the search runs", &m);
	if(rc != HU_OK) return rc;
	if(opts->blen.host != 0 || opts->blen.device < 0)
		return hu_nni_host_scores_entry(fn, opts, n, cs_len, parent, blen, seq, m, edge_cap, n_edges, skipped, edge_node, t_star, f, f0);
	HuBlenTopo tp;
	if((rc = hu_nni_check(fn, opts, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
	std::vector<HuNniEdge> edges;
	hu_nni_edges(tp, parent, blen, &edges, skipped);
	*n_edges = (int32_t) edges.size();
	if((int64_t) edges.size() > edge_cap) { hu_set_error("%s: %zu eligible edges, the outputs hold %d", fn, edges.size(), edge_cap); return HU_ERR_ARG; }
	NniDev r;
	if((rc = r.open(fn, opts, n, cs_len, model, m)) != HU_OK) return rc;
	if(edges.empty()) return HU_OK;
	if((rc = r.msg.sweep(n, parent, blen, seq, true)) != HU_OK) return rc;
	int64_t nCap = 0;
	if((rc = r.score(edges, t_star, f, f0, &nCap)) != HU_OK) return rc;
	for(size_t e = 0; e < edges.size(); ++e) edge_node[e] = edges[e].u;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_tree_nni_scores"); }

extern "C" int hu_tree_nni_search(hu_nni_opts* opts, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const hu_model_desc* model) try {
	const char* fn = "hu_tree_nni_search";
	HuBlenModel m;
	int rc = hu_search_model(fn, opts, model, "the search runs", &m);
	if(rc != HU_OK) return rc;
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	g_nniTiming[0] = g_nniTiming[1] = g_nniTiming[2] = g_nniTiming[3] = 0;
	const double t0 = hu_now_s();
	if(opts->blen.host != 0 || opts->blen.device < 0) rc = hu_nni_host_search_entry(fn, opts, n, cs_len, parent, blen, seq, child_off, child_idx, m, g_nniTiming);
	else {
		HuBlenTopo tp;
		if((rc = hu_nni_check(fn, opts, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
		NniDev r;
		if((rc = r.open(fn, opts, n, cs_len, model, m)) != HU_OK) return rc;
		HuNniOps ops;
		ops.fit = [&](const int32_t* par, double* b, double* ll) { return hu_search_fit_device(r, opts->blen, n, par, b, seq, ll); };
		ops.score = [&](const int32_t* par, const double* b, const std::vector<HuNniEdge>& edges, double* ts, double* f, double* f0) {
			int rc2 = r.msg.sweep(n, par, b, seq, true);
			int64_t nCap = 0;
			if(rc2 == HU_OK) rc2 = r.score(edges, ts, f, f0, &nCap);
			return rc2;
		};
		ops.trial = [&](const int32_t* par, const double* b, double* ll) { return r.msg.trial(n, par, b, seq, ll); };
		rc = hu_nni_rounds(fn, opts, n, cs_len, parent, blen, seq, child_off, child_idx, ops, g_nniTiming);
	}
	g_nniTiming[3] = hu_now_s() - t0 - g_nniTiming[0] - g_nniTiming[1] - g_nniTiming[2];
	return rc;
} catch(...) { return hu_catch_all("hu_tree_nni_search"); }
