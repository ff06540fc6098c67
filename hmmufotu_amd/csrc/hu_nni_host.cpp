// The checks, the host path and the round loop of the NNI search: hmmufotu-amd-tree --ml-lengths --nni --host, the
// reference of the device tests, and what tests/san/nni_driver.cpp runs under the sanitizers.  No HIP headers: a plain C++ compiler
// builds this file.  The arithmetic of a column is hu_tree_nni.h's, shared with the kernel; the sweeps, the fit's round loop and the
// Newton rule are hu_blen_host.cpp's and hu_tree_blen.h's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_set>
#include "hu_tree_nni.h"

extern "C" void hu_nni_default_opts(hu_nni_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	hu_blen_default_opts(&o->blen);
	o->min_gain = 1e-3; o->nni_rounds = 20;
}

/* the fit's need, an edge record (88 bytes) and the outputs (68) per inner node, the nine ratios beyond what LDS holds */
extern "C" int64_t hu_nni_need(int32_t n, int32_t cs_len) {
	if(n < 1 || cs_len < 1) return 0;
	const int64_t inner = (n - 1) / 2 > 0 ? (n - 1) / 2 : 1;      /* a tree of n nodes has at most (n - 1) / 2 inner nodes */
	return hu_blen_need(n, cs_len) + 160 * inner + (cs_len > HU_NNI_LDS_COLS ? 72 * inner * (int64_t) cs_len : 0);
}

int hu_nni_check(const char* fn, const hu_nni_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp) {
	if(!o) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(o->blen.mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	hu_blen_opts bo = o->blen;
	bo.mem_budget = 0;                                          /* the budget is held against the search's need below, not the fit's */
	int rc = hu_blen_check(fn, &bo, n, cs_len, parent, blen, seq, dg_k, tp);
	if(rc != HU_OK) return rc;
	if(o->nni_rounds < 1) { hu_set_error("%s: %d NNI rounds: at least 1", fn, o->nni_rounds); return HU_ERR_ARG; }
	if(!(o->min_gain > 0) || !std::isfinite(o->min_gain)) { hu_set_error("%s: a smallest gain of %g: it must be above 0", fn, o->min_gain); return HU_ERR_ARG; }
	if(o->rounds_cap < 0 || (o->rounds_cap > 0 && !o->rounds) || o->swaps_cap < 0 || (o->swaps_cap > 0 && !o->swaps)) {
		hu_set_error("%s: round or swap records without a place for them", fn); return HU_ERR_ARG; }
	const int64_t need = hu_nni_need(n, cs_len);
	if(o->blen.mem_budget > 0 && need > o->blen.mem_budget) {
		hu_set_error("%s: %d nodes of %d columns need %lld bytes (%lld of them for the messages), the memory budget is %lld bytes", fn, n, cs_len,
			(long long) need, (long long)(64 * (int64_t) n * cs_len), (long long) o->blen.mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

void hu_nni_edges(const HuBlenTopo& tp, const int32_t* parent, const double* blen, std::vector<HuNniEdge>* edges, int64_t* skipped) {
	edges->clear(); *skipped = 0;
	auto kids = [&](int32_t x) { return tp.childOff[x + 1] - tp.childOff[x]; };
	auto kid = [&](int32_t x, int k) { return tp.childIdx[tp.childOff[x] + k]; };
	for(int32_t u = 0; u < tp.n; ++u) {
		if(u == tp.root || kids(u) == 0) continue;
		const int32_t p = parent[u];
		HuNniEdge e; memset(&e, 0, sizeof(e));
		e.u = u; e.v = p; e.D = -1;
		if(p != tp.root) {
			if(kids(u) != 2 || kids(p) != 2) { ++*skipped; continue; }
			e.kind = HU_NNI_INNER;
			e.C = kid(p, 0) == u ? kid(p, 1) : kid(p, 0);
			e.msg[3] = tp.n + p; e.len[3] = blen[p]; e.t0 = blen[u];
		}
		else if(kids(p) >= 3) {
			if(kids(u) != 2 || kids(p) != 3) { ++*skipped; continue; }
			e.kind = HU_NNI_ROOT3;
			int k = 0; int32_t cd[2] = {-1, -1};
			for(int c = 0; c < 3; ++c) if(kid(p, c) != u) cd[k++] = kid(p, c);
			e.C = cd[0]; e.D = cd[1];
			e.msg[3] = e.D; e.len[3] = blen[e.D]; e.t0 = blen[u];
		}
		else if(kids(p) == 2) {
			const int32_t s = kid(p, 0) == u ? kid(p, 1) : kid(p, 0);
			if(kids(s) == 0 || u > s) continue;                 /* a leaf edge; or the edge is scored from s */
			if(kids(u) != 2 || kids(s) != 2) { ++*skipped; continue; }
			e.kind = HU_NNI_ROOT2; e.v = s;
			e.C = kid(s, 0); e.D = kid(s, 1);
			e.msg[3] = e.D; e.len[3] = blen[e.D]; e.t0 = blen[u] + blen[s];
		}
		else continue;                                          /* a root with one child: a leaf of the unrooted tree */
		e.A = kid(u, 0); e.B = kid(u, 1);
		e.msg[0] = e.A; e.msg[1] = e.B; e.msg[2] = e.C;
		e.len[0] = blen[e.A]; e.len[1] = blen[e.B]; e.len[2] = blen[e.C];
		edges->push_back(e);
	}
}

int64_t hu_nni_host_score(const HuBlenModel& m, int32_t n, int64_t L, const std::vector<HuNniEdge>& edges, const double* up, const double* down,
		double lo, double hi, double* t_star, double* f, double* f0) {
	std::vector<double> R((size_t) L * 9);
	int64_t nCap = 0;
	for(size_t ei = 0; ei < edges.size(); ++ei) {
		const HuNniEdge& e = edges[ei];
		double P[64], sumK[3] = {0, 0, 0};
		const double* src[4];
		for(int k = 0; k < 4; ++k) {
			for(int i = 0; i < 16; ++i) P[k * 16 + i] = hu_nni_pentry(m, e.len[k], i / 4, i % 4);
			src[k] = e.msg[k] < n ? up + (size_t) e.msg[k] * L * 4 : down + (size_t)(e.msg[k] - n) * L * 4;
		}
		for(int64_t j = 0; j < L; ++j) {
			double M[16], K[3];
			for(int k = 0; k < 4; ++k) for(int i = 0; i < 4; ++i) M[k * 4 + i] = src[k][j * 4 + i];
			hu_nni_column(m, P, M, &R[(size_t) j * 9], K);
			for(int q = 0; q < 3; ++q) sumK[q] += K[q];
		}
		for(int q = 0; q < 3; ++q) {
			HuBlenExp E;
			auto eval = [&](double x, double* g, double* h) {
				hu_blen_exp(m, x, &E);
				double sg = 0, sh = 0;
				for(int64_t j = 0; j < L; ++j) { double a, b; hu_blen_terms(E, &R[(size_t) j * 9 + q * 3], &a, &b); sg += a; sh += b; }
				*g = sg; *h = sh;
			};
			auto value = [&](double x) {
				hu_blen_exp(m, x, &E);
				double s = 0;
				for(int64_t j = 0; j < L; ++j) s += log(hu_blen_den(E, &R[(size_t) j * 9 + q * 3]));
				return sumK[q] + s;
			};
			double g0, h0;
			eval(e.t0, &g0, &h0);
			if(q == 0) f0[ei] = value(e.t0);
			int its = 0;
			const double x = hu_blen_solve(e.t0, g0, h0, lo, hi, eval, &its);
			if(its > HU_BLEN_MAX_NEWTON) ++nCap;
			t_star[ei * 3 + q] = x;
			f[ei * 3 + q] = value(x);
		}
	}
	return nCap;
}

void hu_nni_apply_edge(const HuNniEdge& e, int q, double t, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx) {
	const int32_t X = q == 1 ? e.B : e.A, Y = e.C, py = parent[Y];
	if(child_off && child_idx) {
		int32_t ix = -1, iy = -1;
		for(int32_t c = child_off[e.u]; c < child_off[e.u + 1]; ++c) if(child_idx[c] == X) ix = c;
		for(int32_t c = child_off[py]; c < child_off[py + 1]; ++c) if(child_idx[c] == Y) iy = c;
		if(ix >= 0 && iy >= 0) std::swap(child_idx[ix], child_idx[iy]);
	}
	parent[X] = py; parent[Y] = e.u;
	if(e.kind == HU_NNI_ROOT2) {
		const double sum = blen[e.u] + blen[e.v];
		const double bu = sum > 0 ? t * (blen[e.u] / sum) : 0.5 * t;
		blen[e.u] = bu; blen[e.v] = t - bu;
	}
	else blen[e.u] = t;
}

void hu_nni_select(const std::vector<HuNniEdge>& edges, const double* gain, double min_gain, std::vector<int32_t>* order, std::vector<int32_t>* taken) {
	order->clear(); taken->clear();
	for(size_t e = 0; e < edges.size(); ++e) if(gain[e] > min_gain) order->push_back((int32_t) e);
	std::sort(order->begin(), order->end(), [&](int32_t a, int32_t b) { return gain[a] != gain[b] ? gain[a] > gain[b] : edges[(size_t) a].u < edges[(size_t) b].u; });
	std::unordered_set<int32_t> used;
	for(int32_t e : *order) {
		const HuNniEdge& x = edges[(size_t) e];
		if(used.count(x.u) || used.count(x.v)) continue;
		used.insert(x.u); used.insert(x.v);
		taken->push_back(e);
	}
}

int hu_nni_rounds(const char* fn, hu_nni_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq, const int32_t* child_off,
		int32_t* child_idx, const HuNniOps& ops, double* sec) {
	std::vector<int32_t> order;
	std::vector<double> ts, f, f0, gain;
	std::vector<HuNniEdge> edges;
	o->n_rounds = 0; o->n_swaps = 0; o->skipped = 0;
	auto better = [&](int32_t e) { return f[(size_t) e * 3 + 1] >= f[(size_t) e * 3 + 2] ? 1 : 2; };
	HuSearchOps so;
	so.fit = ops.fit; so.trial = ops.trial;
	so.score = [&](const HuBlenTopo& tp) {
		hu_nni_edges(tp, parent, blen, &edges, &o->skipped);
		const size_t E = edges.size();
		ts.assign(E * 3, 0.0); f.assign(E * 3, 0.0); f0.assign(E, 0.0); gain.assign(E, 0.0);
		return E == 0 ? (int) HU_OK : ops.score(parent, blen, edges, ts.data(), f.data(), f0.data());
	};
	so.select = [&](const HuBlenTopo&, std::vector<int32_t>* taken) {
		for(size_t e = 0; e < edges.size(); ++e) gain[e] = std::fmax(f[e * 3 + 1], f[e * 3 + 2]) - f[e * 3];
		hu_nni_select(edges, gain.data(), o->min_gain, &order, taken);
	};
	so.apply = [&](const std::vector<int32_t>& taken, int32_t* par, double* bl, int32_t* idx) {
		for(int32_t e : taken) hu_nni_apply_edge(edges[(size_t) e], better(e), ts[(size_t) e * 3 + better(e)], par, bl, child_off, idx);
		return (int) HU_OK;
	};
	so.record = [&](int32_t round, double ll, size_t nTaken, const std::vector<int32_t>& taken) {
		if(o->rounds && o->n_rounds < o->rounds_cap) {
			hu_nni_round& R = o->rounds[o->n_rounds];
			R.ll = ll; R.scored = (int32_t) edges.size(); R.candidates = (int32_t) order.size(); R.taken = (int32_t) nTaken; R.applied = (int32_t) taken.size();
		}
		for(int32_t e : taken) {
			if(o->swaps && o->n_swaps < o->swaps_cap) { int32_t* s = o->swaps + o->n_swaps * 3; s[0] = round; s[1] = edges[(size_t) e].u; s[2] = better(e); }
			o->n_swaps++;
		}
		o->n_rounds++;
	};
	return hu_search_rounds(fn, &o->blen, o->nni_rounds, n, cs_len, parent, blen, seq, child_off, child_idx, so, &o->ll_start, &o->ll_final, &o->stop, sec);
}

/* ---- the host path of the two entries ---- */
int hu_nni_host_scores_entry(const char* fn, const hu_nni_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, double* f0) {
	HuBlenTopo tp;
	int rc = hu_nni_check(fn, o, n, cs_len, parent, blen, seq, 0, &tp);
	if(rc != HU_OK) return rc;
	std::vector<HuNniEdge> edges;
	hu_nni_edges(tp, parent, blen, &edges, skipped);
	*n_edges = (int32_t) edges.size();
	if((int64_t) edges.size() > edge_cap) { hu_set_error("%s: %zu eligible edges, the outputs hold %d", fn, edges.size(), edge_cap); return HU_ERR_ARG; }
	if(edges.empty()) return HU_OK;
	const size_t cells = (size_t) n * (size_t) cs_len * 4;
	std::vector<double> up(cells), down(cells);
	hu_blen_host_sweep(tp, m, parent, cs_len, blen, seq, up.data(), down.data());
	hu_nni_host_score(m, n, cs_len, edges, up.data(), down.data(), o->blen.min_len, o->blen.max_len, t_star, f, f0);
	for(size_t e = 0; e < edges.size(); ++e) edge_node[e] = edges[e].u;
	return HU_OK;
}

int hu_nni_host_search_entry(const char* fn, hu_nni_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuBlenModel& m, double* sec) {
	HuBlenTopo tp0;
	int rc = hu_nni_check(fn, o, n, cs_len, parent, blen, seq, 0, &tp0);
	if(rc != HU_OK) return rc;
	HuBlenHost h(m, n, cs_len, o->blen);
	HuNniOps ops;
	ops.fit = [&](const int32_t* par, double* b, double* ll) { return h.fit(fn, &o->blen, n, par, b, seq, ll); };
	ops.score = [&](const int32_t* par, const double* b, const std::vector<HuNniEdge>& edges, double* ts, double* f, double* f0) {
		HuBlenTopo tp;
		const int rc2 = hu_blen_check(fn, &o->blen, n, cs_len, par, b, seq, 0, &tp);
		if(rc2 != HU_OK) return rc2;
		h.sweep(tp, par, b, seq, true);
		hu_nni_host_score(m, n, cs_len, edges, h.up.data(), h.down.data(), h.lo, h.hi, ts, f, f0);
		return (int) HU_OK;
	};
	ops.trial = [&](const int32_t* par, const double* b, double* ll) { return h.trial(fn, &o->blen, n, par, b, seq, ll); };
	return hu_nni_rounds(fn, o, n, cs_len, parent, blen, seq, child_off, child_idx, ops, sec);
}

/* ---- one swap on the arrays ---- */
extern "C" int hu_tree_nni_apply(int32_t n, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t u, int32_t q, double t) try {
	const char* fn = "hu_tree_nni_apply";
	if(!parent || !blen || n < 2) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(q != 1 && q != 2) { hu_set_error("%s: arrangement %d: 1 (B and C exchanged) or 2 (A and C exchanged)", fn, q); return HU_ERR_ARG; }
	if(!(t >= 0) || !std::isfinite(t)) { hu_set_error("%s: a central length of %g", fn, t); return HU_ERR_ARG; }
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	/* the topology alone is read: the checks of the tree, without rows or options */
	HuBlenTopo tp;
	tp.n = n; tp.root = -1; tp.childOff.assign((size_t) n + 1, 0);
	for(int32_t i = 0; i < n; ++i) {
		if(parent[i] < 0) { if(tp.root >= 0) { hu_set_error("%s: the tree has more than one root", fn); return HU_ERR_ARG; } tp.root = i; }
		else if(parent[i] >= n || parent[i] == i) { hu_set_error("%s: parent of node %d out of range", fn, i); return HU_ERR_ARG; }
		else tp.childOff[(size_t) parent[i] + 1]++;
	}
	if(tp.root < 0) { hu_set_error("%s: the tree has no root", fn); return HU_ERR_ARG; }
	for(int32_t i = 0; i < n; ++i) tp.childOff[(size_t) i + 1] += tp.childOff[i];
	tp.childIdx.assign((size_t) n - 1, 0);
	std::vector<int32_t> fill(tp.childOff.begin(), tp.childOff.end() - 1);
	for(int32_t i = 0; i < n; ++i) if(parent[i] >= 0) tp.childIdx[(size_t) fill[parent[i]]++] = i;
	if(child_off) for(int32_t i = 0; i < n; ++i) if(child_off[i + 1] - child_off[i] != tp.childOff[i + 1] - tp.childOff[i]) {
		hu_set_error("%s: child_off gives node %d another number of children than parent", fn, i); return HU_ERR_ARG; }
	std::vector<HuNniEdge> edges; int64_t skipped = 0;
	hu_nni_edges(tp, parent, blen, &edges, &skipped);
	for(const HuNniEdge& e : edges) if(e.u == u || (e.kind == HU_NNI_ROOT2 && e.v == u)) {
		hu_nni_apply_edge(e, q, t, parent, blen, child_off, child_idx);
		return HU_OK;
	}
	hu_set_error("%s: the edge above node %d is not eligible: both its ends must have degree three", fn, u);
	return HU_ERR_ARG;
} catch(...) { return hu_catch_all("hu_tree_nni_apply"); }

/* ---- Newick from the arrays: the writer of hu_newick_write on parent and the order of children ---- */
extern "C" int64_t hu_newick_from_arrays(int32_t n, const int32_t* parent, const int32_t* child_off, const int32_t* child_idx, const char* const* names,
		const double* blen, char* buf, int64_t cap) try {
	const char* fn = "hu_newick_from_arrays";
	if(n < 1 || !parent || !child_off || (n > 1 && !child_idx) || !blen || cap < 0 || (cap > 0 && !buf)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	int32_t root = -1;
	for(int32_t i = 0; i < n; ++i) if(parent[i] < 0) { if(root >= 0) { hu_set_error("%s: the tree has more than one root", fn); return HU_ERR_ARG; } root = i; }
	if(root < 0 || child_off[0] != 0 || child_off[n] != n - 1) { hu_set_error("%s: no root, or child_off does not hold n - 1 children", fn); return HU_ERR_ARG; }
	std::vector<char> listed((size_t) n, 0);
	for(int32_t i = 0; i < n; ++i) {
		if(child_off[i + 1] < child_off[i]) { hu_set_error("%s: child_off decreases at node %d", fn, i); return HU_ERR_ARG; }
		for(int32_t c = child_off[i]; c < child_off[i + 1]; ++c) {
			if(child_idx[c] < 0 || child_idx[c] >= n || parent[child_idx[c]] != i || listed[(size_t) child_idx[c]]) {
				hu_set_error("%s: child_idx and parent disagree at node %d", fn, i); return HU_ERR_ARG; }
			listed[(size_t) child_idx[c]] = 1;
		}
	}
	auto unquoted = [](unsigned char c) { return c > 0x20 && c < 0x7f && !strchr("()[]':;,", c); };
	std::string out;
	char num[40];
	size_t written = 0;
	auto close_node = [&](int32_t v) {
		const char* s = names && names[v] ? names[v] : "";
		bool plain = true;
		for(const char* c = s; *c; ++c) if(!unquoted((unsigned char) *c)) plain = false;
		if(plain) out += s; else { out += '\''; out += s; out += '\''; }
		if(parent[v] >= 0) { snprintf(num, sizeof(num), ":%.17g", blen[v]); out += num; }
		++written;
	};
	std::vector<std::pair<int32_t, int32_t>> st;       /* node, next child */
	st.push_back({root, child_off[root]});
	if(n > 1) out += '(';
	while(!st.empty()) {
		auto& fr = st.back();
		const int32_t v = fr.first;
		if(fr.second < child_off[v + 1]) {
			if(fr.second > child_off[v]) out += ',';
			const int32_t c = child_idx[fr.second++];
			if(child_off[c] != child_off[c + 1]) out += '(';
			st.push_back({c, child_off[c]});
			continue;
		}
		if(child_off[v] != child_off[v + 1]) out += ')';
		close_node(v);
		st.pop_back();
	}
	if(written != (size_t) n) { hu_set_error("%s: the tree is not connected", fn); return HU_ERR_ARG; }
	out += ";\n";
	if(cap > 0) { const size_t k = std::min<size_t>(out.size(), (size_t) cap - 1); memcpy(buf, out.data(), k); buf[k] = 0; }
	return (int64_t) out.size();
} catch(...) { return hu_catch_all("hu_newick_from_arrays"); }
