// The checks, the host path, the insertion on the arrays and the round loop of hmmufotu-amd-tree --add: the loop is one
// text for the host path and the device path, which differ in the three operations of HuAddOps; the host path is the reference of the
// device tests and what tests/san/add_driver.cpp runs under the sanitizers.  No HIP headers: a plain C++ compiler builds this file.
// The arithmetic of a column is hu_tree_add.h's, shared with the kernel; the sweeps, the fit's round loop and the Newton rule are
// hu_blen_host.cpp's and hu_tree_blen.h's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "hu_tree_add.h"

extern "C" void hu_add_default_opts(hu_add_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	hu_blen_default_opts(&o->blen);
}

extern "C" int64_t hu_add_need(int32_t final_nodes, int32_t cs_len, int32_t n_query) {
	if(final_nodes < 1 || cs_len < 1 || n_query < 0) return 0;
	const int64_t one = hu_add_tile_bytes(final_nodes, cs_len, HU_ADD_TILE), tiles = ((int64_t) n_query + HU_ADD_TILE - 1) / HU_ADD_TILE;
	return hu_blen_need(final_nodes, cs_len) + (n_query > 0 ? std::max(one, std::min<int64_t>(one * tiles, HU_ADD_SLAB_BYTES)) : 0);
}

int hu_add_check(const char* fn, const hu_add_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t n_query, const int8_t* qseq, bool grows, int32_t dg_k, HuBlenTopo* tp) {
	if(!o) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(o->blen.mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	hu_blen_opts bo = o->blen;
	bo.mem_budget = 0;                                          /* the budget is held against the insertion's need below, not the fit's */
	int rc = hu_blen_check(fn, &bo, n, cs_len, parent, blen, seq, dg_k, tp);
	if(rc != HU_OK) return rc;
	if(n_query < 0 || (n_query > 0 && !qseq)) { hu_set_error("%s: %d queries without their rows", fn, n_query); return HU_ERR_ARG; }
	if((int64_t) n + 2 * (int64_t) n_query > INT32_MAX) { hu_set_error("%s: %d nodes and %d queries: the grown tree has too many nodes", fn, n, n_query); return HU_ERR_ARG; }
	if(o->slab < 0 || o->tile < 0) { hu_set_error("%s: a slab of %d queries in tiles of %d", fn, o->slab, o->tile); return HU_ERR_ARG; }
	if(o->rounds_cap < 0 || (o->rounds_cap > 0 && !o->rounds) || o->inserts_cap < 0 || (o->inserts_cap > 0 && !o->inserts)) {
		hu_set_error("%s: round or insertion records without a place for them", fn); return HU_ERR_ARG; }
	for(int32_t r = 0; r < n_query; ++r) {
		const int8_t* row = qseq + (size_t) r * cs_len;
		for(int32_t j = 0; j < cs_len; ++j) if(row[j] > 3) { hu_set_error("%s: query %d holds the code %d at column %d", fn, r, (int) row[j], j); return HU_ERR_ARG; }
	}
	const int32_t fin = grows ? n + 2 * n_query : n;
	const int64_t need = hu_add_need(fin, cs_len, n_query);
	if(o->blen.mem_budget > 0 && need > o->blen.mem_budget) {
		hu_set_error("%s: %d nodes of %d columns and %d new sequences need %lld bytes (%lld of them for the messages), the memory budget is %lld bytes", fn, fin, cs_len,
			n_query, (long long) need, (long long)(64 * (int64_t) fin * cs_len), (long long) o->blen.mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

void hu_add_host_score(const HuBlenModel& m, int32_t n, int64_t L, int32_t root, const double* blen, const double* up, const double* down,
		double lo, double hi, double t0, int32_t nq, const int8_t* qseq, double* t_star, double* f) {
	std::vector<double> R((size_t) L * 3);
	double tab[HU_ADD_TAB];
	for(int i = 0; i < HU_ADD_TAB; ++i) tab[i] = hu_add_tab_entry(m, i);
	for(int32_t w = 0; w < n; ++w) {
		if(w == root) { for(int32_t q = 0; q < nq; ++q) { t_star[(size_t) q * n + w] = 0.0; f[(size_t) q * n + w] = -INFINITY; } continue; }
		double P[16];
		for(int i = 0; i < 16; ++i) P[i] = hu_nni_pentry(m, 0.5 * blen[w], i >> 2, i & 3);
		double sumK = 0;
		for(int64_t j = 0; j < L; ++j) { double K; hu_add_edge_column(m, P, up + ((size_t) w * L + j) * 4, down + ((size_t) w * L + j) * 4, &R[(size_t) j * 3], &K); sumK += K; }
		for(int32_t q = 0; q < nq; ++q) {
			const int8_t* row = qseq + (size_t) q * L;
			HuBlenExp E;
			auto eval = [&](double x, double* g, double* h) {
				hu_blen_exp(m, x, &E);
				double sg = 0, sh = 0;
				for(int64_t j = 0; j < L; ++j) {
					double r[3], a, c;
					hu_add_ratio(tab, hu_add_sym(row[j]), R[(size_t) j * 3], R[(size_t) j * 3 + 1], R[(size_t) j * 3 + 2], r);
					hu_blen_terms(E, r, &a, &c); sg += a; sh += c;
				}
				*g = sg; *h = sh;
			};
			double kap = 0;
			for(int64_t j = 0; j < L; ++j) kap += tab[15 + hu_add_sym(row[j])];
			double g0, h0;
			eval(t0, &g0, &h0);
			int its = 0;
			const double x = hu_blen_solve(t0, g0, h0, lo, hi, eval, &its);
			hu_blen_exp(m, x, &E);
			double s = 0;
			for(int64_t j = 0; j < L; ++j) {
				double r[3];
				hu_add_ratio(tab, hu_add_sym(row[j]), R[(size_t) j * 3], R[(size_t) j * 3 + 1], R[(size_t) j * 3 + 2], r);
				s += log(hu_blen_den(E, r));
			}
			t_star[(size_t) q * n + w] = x; f[(size_t) q * n + w] = (sumK + kap) + s;
		}
	}
}

void hu_add_host_best(int32_t n, int32_t root, int32_t nq, const double* t_star, const double* f, int32_t* best_w, double* best_t, double* best_f) {
	for(int32_t q = 0; q < nq; ++q) {
		int32_t bw = -1; double bf = -INFINITY;
		for(int32_t w = 0; w < n; ++w) {
			if(w == root) continue;
			if(hu_add_better(f[(size_t) q * n + w], w, bf, bw)) { bw = w; bf = f[(size_t) q * n + w]; }
		}
		best_w[q] = bw; best_t[q] = t_star[(size_t) q * n + bw]; best_f[q] = bf;
	}
}

/* ---- the insertion on the arrays ---- */
int hu_add_apply(const char* fn, int32_t n, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx, int32_t w, double t, double lo, double hi) {
	if(!parent || !blen || n < 2) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	if(n > INT32_MAX - 2) { hu_set_error("%s: %d nodes: no room for two more", fn, n); return HU_ERR_ARG; }
	if(!(lo >= 0) || !(lo < hi) || !std::isfinite(hi)) { hu_set_error("%s: pendant lengths in [%g, %g]: 0 <= min_len < max_len is required", fn, lo, hi); return HU_ERR_ARG; }
	int32_t root = -1;
	std::vector<int32_t> deg((size_t) n, 0);
	for(int32_t i = 0; i < n; ++i) {
		if(parent[i] < 0) { if(root >= 0) { hu_set_error("%s: the tree has more than one root", fn); return HU_ERR_ARG; } root = i; }
		else if(parent[i] >= n || parent[i] == i) { hu_set_error("%s: parent of node %d out of range", fn, i); return HU_ERR_ARG; }
		else deg[(size_t) parent[i]]++;
	}
	if(root < 0) { hu_set_error("%s: the tree has no root", fn); return HU_ERR_ARG; }
	if(w < 0 || w >= n || w == root) { hu_set_error("%s: node %d names no edge: the top node has none above it, and the tree has the nodes 0 to %d", fn, w, n - 1); return HU_ERR_ARG; }
	if(!(t >= lo) || !(t <= hi)) { hu_set_error("%s: a pendant length of %g outside [%g, %g]", fn, t, lo, hi); return HU_ERR_ARG; }
	const int32_t p = n, v = n + 1, pw = parent[w];
	if(child_off) {
		if(child_off[0] != 0) { hu_set_error("%s: child_off does not begin at 0", fn); return HU_ERR_ARG; }
		for(int32_t i = 0; i < n; ++i) if(child_off[i + 1] - child_off[i] != deg[(size_t) i]) {
			hu_set_error("%s: child_off gives node %d another number of children than parent", fn, i); return HU_ERR_ARG; }
		int32_t iw = -1;
		for(int32_t c = child_off[pw]; c < child_off[pw + 1]; ++c) { if(child_idx[c] < 0 || child_idx[c] >= n) { hu_set_error("%s: child_idx out of range", fn); return HU_ERR_ARG; } if(child_idx[c] == w) iw = c; }
		if(iw < 0) { hu_set_error("%s: child_idx and parent disagree", fn); return HU_ERR_ARG; }
		/* p takes w's place; the lists of the two new nodes follow the old ones: p holds w, then v, and v holds none */
		child_idx[iw] = p;
		child_idx[n - 1] = w; child_idx[n] = v;
		child_off[p + 1] = child_off[p] + 2; child_off[v + 1] = child_off[p + 1];
	}
	const double half = 0.5 * blen[w];
	parent[p] = pw; parent[w] = p; parent[v] = p;
	blen[w] = half; blen[p] = half; blen[v] = t;
	return HU_OK;
}

extern "C" int hu_tree_add_apply(int32_t n, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx, int32_t w, double t, double min_len, double max_len) try {
	return hu_add_apply("hu_tree_add_apply", n, parent, blen, child_off, child_idx, w, t, min_len, max_len);
} catch(...) { return hu_catch_all("hu_tree_add_apply"); }

/* ---- the round loop ---- */
int hu_add_rounds(const char* fn, hu_add_opts* o, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const HuAddOps& ops, double* sec) {
	const size_t L = (size_t) cs_len;
	o->n_rounds = 0; o->n_inserted = 0;
	int rc;
	double ll = 0, t0 = hu_now_s();
	if((rc = ops.fit(n, parent, blen, seq, &ll)) != HU_OK) return rc;
	sec[2] += hu_now_s() - t0;
	o->ll_start = o->ll_final = ll;
	std::vector<int32_t> rem((size_t) n_query), bw, owner, take;
	for(int32_t r = 0; r < n_query; ++r) rem[(size_t) r] = r;
	std::vector<int8_t> rows;
	std::vector<double> bt, bf;
	HuBlenTopo tp;
	for(int32_t round = 1; !rem.empty(); ++round) {
		const int32_t nq = (int32_t) rem.size();
		hu_blen_opts bo = o->blen;
		bo.mem_budget = 0;
		if((rc = hu_blen_check(fn, &bo, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
		t0 = hu_now_s();
		if((rc = ops.sweep(n, parent, blen, seq, tp)) != HU_OK) return rc;
		sec[0] += hu_now_s() - t0;
		rows.resize((size_t) nq * L);
		for(int32_t i = 0; i < nq; ++i) memcpy(rows.data() + (size_t) i * L, qseq + (size_t) rem[(size_t) i] * L, L);
		bw.assign((size_t) nq, -1); bt.assign((size_t) nq, 0.0); bf.assign((size_t) nq, 0.0);
		t0 = hu_now_s();
		if((rc = ops.score(n, tp.root, blen, hu_add_start(n, parent, blen, o->blen.min_len, o->blen.max_len), nq, rows.data(), bw.data(), bt.data(), bf.data())) != HU_OK) return rc;
		sec[1] += hu_now_s() - t0;
		/* per edge the one query with the largest f among those whose best edge it is; rem is ascending, so a tie keeps the smaller query */
		owner.assign((size_t) n, -1);
		for(int32_t i = 0; i < nq; ++i) {
			const int32_t w = bw[(size_t) i];
			if(w < 0 || w >= n || w == tp.root) { hu_set_error("%s: query %d has no best edge", fn, rem[(size_t) i]); return HU_ERR_STATE; }
			if(owner[(size_t) w] < 0 || bf[(size_t) i] > bf[(size_t) owner[(size_t) w]]) owner[(size_t) w] = i;
		}
		take.clear();
		for(int32_t i = 0; i < nq; ++i) if(owner[(size_t) bw[(size_t) i]] == i) take.push_back(i);
		/* inserted in ascending query: the new ids */
		for(int32_t i : take) {
			const int32_t r = rem[(size_t) i], w = bw[(size_t) i];
			if(hu_add_apply(fn, n, parent, blen, child_off, child_idx, w, bt[(size_t) i], o->blen.min_len, o->blen.max_len) != HU_OK) return HU_ERR_STATE;
			memset(seq + (size_t) n * L, -2, L);
			memcpy(seq + (size_t)(n + 1) * L, qseq + (size_t) r * L, L);
			if(query_node) query_node[r] = n + 1;
			if(o->inserts && o->n_inserted < o->inserts_cap) {
				hu_add_insert& I = o->inserts[o->n_inserted];
				I.round = round; I.query = r; I.v = n + 1; I.w = w; I.t = bt[(size_t) i]; I.f = bf[(size_t) i];
			}
			o->n_inserted++;
			n += 2;
		}
		for(size_t k = take.size(); k-- > 0;) rem.erase(rem.begin() + take[k]);
		t0 = hu_now_s();
		if((rc = ops.fit(n, parent, blen, seq, &ll)) != HU_OK) return rc;
		sec[2] += hu_now_s() - t0;
		o->ll_final = ll;
		if(o->rounds && o->n_rounds < o->rounds_cap) { hu_add_round& R = o->rounds[o->n_rounds]; R.ll = ll; R.scored = nq; R.inserted = (int32_t) take.size(); }
		o->n_rounds++;
	}
	return HU_OK;
}

/* ---- the host path of the two entries ---- */
int hu_add_host_scores_entry(const char* fn, const hu_add_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, int32_t n_query, const int8_t* qseq, double* t_star, double* f, int32_t* best_w, double* best_t, double* best_f) {
	HuBlenTopo tp;
	int rc = hu_add_check(fn, o, n, cs_len, parent, blen, seq, n_query, qseq, false, 0, &tp);
	if(rc != HU_OK || n_query == 0) return rc;
	const size_t cells = (size_t) n * (size_t) cs_len * 4, nOut = (size_t) n_query * (size_t) n;
	std::vector<double> up(cells), down(cells), ts, fv;
	if(!t_star || !f) { ts.resize(nOut); fv.resize(nOut); t_star = ts.data(); f = fv.data(); }
	hu_blen_host_sweep(tp, m, parent, cs_len, blen, seq, up.data(), down.data());
	hu_add_host_score(m, n, cs_len, tp.root, blen, up.data(), down.data(), o->blen.min_len, o->blen.max_len,
		hu_add_start(n, parent, blen, o->blen.min_len, o->blen.max_len), n_query, qseq, t_star, f);
	hu_add_host_best(n, tp.root, n_query, t_star, f, best_w, best_t, best_f);
	return HU_OK;
}

int hu_add_host_search_entry(const char* fn, hu_add_opts* o, int32_t n, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const HuBlenModel& m, double* sec) {
	HuBlenTopo tp0;
	int rc = hu_add_check(fn, o, n, cs_len, parent, blen, seq, n_query, qseq, true, 0, &tp0);
	if(rc != HU_OK) return rc;
	HuBlenHost h(m, (int64_t) n + 2 * (int64_t) n_query, cs_len, o->blen);
	std::vector<double> ts, fv;
	HuAddOps ops;
	ops.fit = [&](int32_t nn, const int32_t* par, double* b, const int8_t* sq, double* ll) { return h.fit(fn, &o->blen, nn, par, b, sq, ll); };
	ops.sweep = [&](int32_t, const int32_t* par, const double* b, const int8_t* sq, const HuBlenTopo& tp) { h.sweep(tp, par, b, sq, true); return (int) HU_OK; };
	ops.score = [&](int32_t nn, int32_t root, const double* b, double t0, int32_t nq, const int8_t* rows, int32_t* bw, double* bt, double* bf) {
		ts.resize((size_t) nq * (size_t) nn); fv.resize((size_t) nq * (size_t) nn);
		hu_add_host_score(m, nn, cs_len, root, b, h.up.data(), h.down.data(), h.lo, h.hi, t0, nq, rows, ts.data(), fv.data());
		hu_add_host_best(nn, root, nq, ts.data(), fv.data(), bw, bt, bf);
		return (int) HU_OK;
	};
	return hu_add_rounds(fn, o, n, cs_len, n_query, parent, blen, seq, child_off, child_idx, qseq, query_node, ops, sec);
}
