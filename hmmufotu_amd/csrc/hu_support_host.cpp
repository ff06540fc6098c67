// The checks, the weights and the host path of the local branch supports: hmmufotu-amd-tree --support --host, the
// reference of the device tests, and what tests/san/support_driver.cpp runs under the sanitizers.  No HIP headers: a plain C++
// compiler builds this file.  The arithmetic of a column is hu_tree_support.h's, shared with the kernel; the sweeps are
// hu_blen_host.cpp's and the scoring is hu_nni_host.cpp's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "hu_tree_support.h"

extern "C" void hu_support_default_opts(hu_support_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	hu_blen_default_opts(&o->blen);
	o->replicates = 1000; o->seed = 1;
}

static bool support_shape_ok(const char* fn, int64_t cs_len, int64_t replicates) {
	if(cs_len < 1 || cs_len > 65535) { hu_set_error("%s: %lld columns: 1 to 65535, a count of draws is 16 bits wide", fn, (long long) cs_len); return false; }
	if(replicates < 1 || replicates > HU_SUPPORT_MAX_REPLICATES) {
		hu_set_error("%s: %lld replicates: 1 to %d", fn, (long long) replicates, HU_SUPPORT_MAX_REPLICATES); return false; }
	return true;
}

extern "C" int hu_support_weights(int32_t cs_len, int32_t replicates, uint64_t seed, uint16_t* w) try {
	const char* fn = "hu_support_weights";
	if(!w) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(!support_shape_ok(fn, cs_len, replicates)) return HU_ERR_ARG;
	const uint32_t L = (uint32_t) cs_len;
	memset(w, 0, (size_t) replicates * L * sizeof(uint16_t));
	for(uint32_t b = 0; b < (uint32_t) replicates; ++b) {
		uint16_t* row = w + (size_t) b * L;
		for(uint32_t i = 0; i < L; i += 4) {
			uint32_t col[4];
			hu_support_draw4(seed, b, i / 4, L, col);
			for(uint32_t k = 0; k < 4 && i + k < L; ++k) row[col[k]]++;
		}
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_support_weights"); }

/* hu_nni_need, the table, 32 bytes of outputs per inner node and the sums of one launch's edges */
extern "C" int64_t hu_support_need(int32_t n, int32_t cs_len, int32_t replicates) {
	if(n < 1 || cs_len < 1 || replicates < 1) return 0;
	const int64_t inner = (n - 1) / 2 > 0 ? (n - 1) / 2 : 1, B = replicates;
	static_assert(HU_SUPPORT_LDS_COLS >= HU_NNI_LDS_COLS, "beyond LDS, d lies in the ratio scratch of the scoring");
	const int64_t sums = std::max<int64_t>(std::min<int64_t>(inner * B * 16, (int64_t) 16 << 20), B * 16);
	return hu_nni_need(n, cs_len) + 2 * hu_support_bpad(B) * (int64_t) cs_len + 32 * inner + sums;
}

int hu_support_check(const char* fn, const hu_support_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		HuBlenTopo* tp, hu_nni_opts* no) {
	if(!o) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(o->blen.mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	hu_nni_default_opts(no);
	no->blen.min_len = o->blen.min_len; no->blen.max_len = o->blen.max_len; no->blen.device = o->blen.device; no->blen.host = o->blen.host;
	no->blen.mem_budget = 0;                                  /* the budget is held against the supports' need below */
	int rc = hu_nni_check(fn, no, n, cs_len, parent, blen, seq, 0, tp);
	if(rc != HU_OK) return rc;
	if(!support_shape_ok(fn, cs_len, o->replicates)) return HU_ERR_ARG;
	const int64_t need = hu_support_need(n, cs_len, o->replicates);
	if(o->blen.mem_budget > 0 && need > o->blen.mem_budget) {
		hu_set_error("%s: %d nodes of %d columns and %d replicates need %lld bytes (%lld of them for the table of weights), the memory budget is %lld bytes", fn, n,
			cs_len, o->replicates, (long long) need, (long long)(2 * hu_support_bpad(o->replicates) * (int64_t) cs_len), (long long) o->blen.mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

void hu_support_host_edges(const HuBlenModel& m, int32_t n, int64_t L, int64_t B, const std::vector<HuNniEdge>& edges, const double* up, const double* down,
		const double* t_star, const uint16_t* w, double* f2, int32_t* count, double* sums, int64_t* bad) {
	std::vector<double> d((size_t) L * 2);
	*bad = -1;
	for(size_t ei = 0; ei < edges.size(); ++ei) {
		const HuNniEdge& e = edges[ei];
		double P[64], sK[3] = {0, 0, 0}, sD[3] = {0, 0, 0};
		const double* src[4];
		HuBlenExp E[3];
		for(int k = 0; k < 4; ++k) {
			for(int i = 0; i < 16; ++i) P[k * 16 + i] = hu_nni_pentry(m, e.len[k], i / 4, i % 4);
			src[k] = e.msg[k] < n ? up + (size_t) e.msg[k] * L * 4 : down + (size_t)(e.msg[k] - n) * L * 4;
		}
		for(int q = 0; q < 3; ++q) hu_blen_exp(m, t_star[ei * 3 + q], &E[q]);
		for(int64_t j = 0; j < L; ++j) {
			double M[16], K[3], lD[3];
			for(int k = 0; k < 4; ++k) for(int i = 0; i < 4; ++i) M[k * 4 + i] = src[k][j * 4 + i];
			if(!hu_support_column(m, P, M, E, K, lD, &d[(size_t) j * 2]) && *bad < 0) *bad = (int64_t) ei;
			for(int q = 0; q < 3; ++q) { sK[q] += K[q]; sD[q] += lD[q]; }
		}
		for(int q = 0; q < 3; ++q) f2[ei * 3 + q] = sK[q] + sD[q];
		const double eta = hu_support_eta(f2[ei * 3]);
		int32_t c = 0;
		for(int64_t b = 0; b < B; ++b) {
			const uint16_t* wb = w + (size_t) b * L;
			double S1 = 0.0, S2 = 0.0;
			for(int64_t j = 0; j < L; ++j) { const double x = (double) wb[j]; S1 += x * d[(size_t) j * 2]; S2 += x * d[(size_t) j * 2 + 1]; }
			if(sums) { sums[(ei * (size_t) B + (size_t) b) * 2] = S1; sums[(ei * (size_t) B + (size_t) b) * 2 + 1] = S2; }
			if(hu_support_supports(S1, S2, eta)) ++c;
		}
		count[ei] = c;
	}
}

int hu_support_verify(const char* fn, const std::vector<HuNniEdge>& edges, const double* f, const double* f2, int64_t bad) {
	if(bad >= 0) {
		hu_set_error("%s: the edge above node %d has a column of likelihood 0 in the tree as it stands: the tree's log-likelihood is -inf, no support is defined",
			fn, edges[(size_t) bad].u);
		return HU_ERR_ARG;
	}
	for(size_t e = 0; e < edges.size(); ++e) for(int q = 0; q < 3; ++q) if(memcmp(&f[e * 3 + q], &f2[e * 3 + q], sizeof(double)) != 0) {
		hu_set_error("%s: the edge above node %d: the columns of arrangement %d sum to %.17g, the scoring gave %.17g", fn, edges[e].u, q, f2[e * 3 + q], f[e * 3 + q]);
		return HU_ERR_STATE;
	}
	return HU_OK;
}

int hu_support_host_entry(const char* fn, const hu_support_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, int32_t* count,
		double* sums, double* sec) {
	HuBlenTopo tp;
	hu_nni_opts no;
	int rc = hu_support_check(fn, o, n, cs_len, parent, blen, seq, &tp, &no);
	if(rc != HU_OK) return rc;
	std::vector<HuNniEdge> edges;
	hu_nni_edges(tp, parent, blen, &edges, skipped);
	*n_edges = (int32_t) edges.size();
	if((int64_t) edges.size() > edge_cap) { hu_set_error("%s: %zu eligible edges, the outputs hold %d", fn, edges.size(), edge_cap); return HU_ERR_ARG; }
	if(edges.empty()) return HU_OK;
	const size_t E = edges.size(), cells = (size_t) n * (size_t) cs_len * 4;
	const int64_t L = cs_len, B = o->replicates;
	double t0 = hu_now_s();
	std::vector<double> up(cells), down(cells), f0(E), f2(E * 3);
	hu_blen_host_sweep(tp, m, parent, L, blen, seq, up.data(), down.data());
	sec[0] = hu_now_s() - t0; t0 = hu_now_s();
	hu_nni_host_score(m, n, L, edges, up.data(), down.data(), o->blen.min_len, o->blen.max_len, t_star, f, f0.data());
	sec[1] = hu_now_s() - t0; t0 = hu_now_s();
	std::vector<uint16_t> w((size_t) B * (size_t) L);
	if((rc = hu_support_weights(cs_len, o->replicates, o->seed, w.data())) != HU_OK) return rc;
	sec[2] = hu_now_s() - t0; t0 = hu_now_s();
	int64_t bad = -1;
	hu_support_host_edges(m, n, L, B, edges, up.data(), down.data(), t_star, w.data(), f2.data(), count, sums, &bad);
	sec[3] = hu_now_s() - t0;
	if((rc = hu_support_verify(fn, edges, f, f2.data(), bad)) != HU_OK) return rc;
	for(size_t e = 0; e < E; ++e) edge_node[e] = edges[e].u;
	return HU_OK;
}
