// The checks, the host path and the round loop of the branch-length fit: hmmufotu-amd-tree --ml-lengths --host, the
// reference of the device tests, and what tests/san/blen_driver.cpp runs under the sanitizers.  No HIP headers: a plain C++ compiler
// builds this file.  The arithmetic of a column and the rule of a Newton step are hu_tree_blen.h's, shared with the kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "hu_tree_blen.h"

extern "C" void hu_blen_default_opts(hu_blen_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	o->eps = 1e-5; o->min_len = 0.0; o->max_len = 10.0; o->max_rounds = 50;
}

/* the messages, the rows, the ratios beyond what LDS holds, the column values, 1 MB of slack */
extern "C" int64_t hu_blen_need(int32_t n, int32_t cs_len) {
	if(n < 1 || cs_len < 1) return 0;
	const int64_t cells = (int64_t) n * cs_len;
	return 64 * cells + cells + (cs_len > HU_BLEN_LDS_COLS ? 24 * cells : 0) + 8 * (int64_t) cs_len + (1 << 20);
}

int hu_blen_check(const char* fn, const hu_blen_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp) {
	if(!o || !parent || !blen || !seq || !tp) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(n < 2 || cs_len < 1 || cs_len > 65535) { hu_set_error("%s: %d nodes of %d columns: at least 2 nodes and 1 to 65535 columns", fn, n, cs_len); return HU_ERR_ARG; }
	if(dg_k != 0) { hu_set_error("%s: a model with %d discrete Gamma categories: branch lengths are fitted under the fixed-rate model only", fn, dg_k); return HU_ERR_ARG; }
	if(!(o->eps >= 100 * HU_BLEN_TAU) || !std::isfinite(o->eps)) { hu_set_error("%s: eps %g: at least %g (100 times the step's tolerance)", fn, o->eps, 100 * HU_BLEN_TAU); return HU_ERR_ARG; }
	if(!(o->min_len >= 0) || !std::isfinite(o->max_len) || !(o->max_len > 0) || !(o->min_len < o->max_len)) {
		hu_set_error("%s: branch lengths in [%g, %g]: 0 <= min_len < max_len is required", fn, o->min_len, o->max_len); return HU_ERR_ARG; }
	if(o->max_rounds < 1) { hu_set_error("%s: %d rounds: at least 1", fn, o->max_rounds); return HU_ERR_ARG; }
	if(o->mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	tp->n = n; tp->root = -1;
	tp->childOff.assign((size_t) n + 1, 0);
	for(int32_t i = 0; i < n; ++i) {
		if(parent[i] < 0) { if(tp->root >= 0) { hu_set_error("%s: the tree has more than one root", fn); return HU_ERR_ARG; } tp->root = i; }
		else if(parent[i] >= n || parent[i] == i) { hu_set_error("%s: parent of node %d out of range", fn, i); return HU_ERR_ARG; }
		else tp->childOff[(size_t) parent[i] + 1]++;
	}
	if(tp->root < 0) { hu_set_error("%s: the tree has no root", fn); return HU_ERR_ARG; }
	for(int32_t i = 0; i < n; ++i) tp->childOff[(size_t) i + 1] += tp->childOff[i];
	tp->childIdx.assign((size_t) n - 1, 0);
	std::vector<int32_t> fill(tp->childOff.begin(), tp->childOff.end() - 1);
	for(int32_t i = 0; i < n; ++i) if(parent[i] >= 0) tp->childIdx[(size_t) fill[parent[i]]++] = i;
	tp->order.clear(); tp->order.reserve(n); tp->order.push_back(tp->root);
	for(size_t h = 0; h < tp->order.size(); ++h) { const int32_t u = tp->order[h]; for(int32_t c = tp->childOff[u]; c < tp->childOff[u + 1]; ++c) tp->order.push_back(tp->childIdx[c]); }
	if((int32_t) tp->order.size() != n) { hu_set_error("%s: the tree is not connected", fn); return HU_ERR_ARG; }
	for(int32_t i = 0; i < n; ++i) {
		if(i != tp->root && (!(blen[i] >= 0) || !std::isfinite(blen[i]))) { hu_set_error("%s: the length of the branch above node %d is %g", fn, i, blen[i]); return HU_ERR_ARG; }
		if(tp->childOff[i] == tp->childOff[i + 1]) {
			const int8_t* row = seq + (size_t) i * cs_len;
			for(int32_t j = 0; j < cs_len; ++j) if(row[j] > 3) { hu_set_error("%s: leaf %d holds the code %d at column %d", fn, i, (int) row[j], j); return HU_ERR_ARG; }
		}
	}
	const int64_t need = hu_blen_need(n, cs_len);
	if(o->mem_budget > 0 && need > o->mem_budget) {
		hu_set_error("%s: %d nodes of %d columns need %lld bytes (%lld of them for the messages), the memory budget is %lld bytes", fn, n, cs_len,
			(long long) need, (long long)(64 * (int64_t) n * cs_len), (long long) o->mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

/* log(P(t) . exp(M + scale)) - scale, scale = -510 - max M when max M < -510 (src/PhyloTreeUnrooted.h:1495-1503), as hu_kern_tree.h has it */
static void blen_conv(const HuBlenModel& m, double t, const double* M, double* Y) {
	const double mx = hu_blen_max4(M);
	const double scale = (mx != -INFINITY && mx < HU_BLEN_MIN_LOGLIK_EXP) ? HU_BLEN_MIN_LOGLIK_EXP - mx : 0.0;
	double e[4], c[4];
	for(int i = 0; i < 4; ++i) e[i] = exp(M[i] + scale);
	if(t == 0) { for(int i = 0; i < 4; ++i) c[i] = e[i]; }
	else {
		double s[4];
		for(int k = 0; k < 4; ++k) s[k] = exp(m.lam[k] * t) * ((m.U1[k * 4 + 0] * e[0] + m.U1[k * 4 + 1] * e[1]) + (m.U1[k * 4 + 2] * e[2] + m.U1[k * 4 + 3] * e[3]));
		for(int i = 0; i < 4; ++i) c[i] = fmax((m.U[i * 4 + 0] * s[0] + m.U[i * 4 + 1] * s[1]) + (m.U[i * 4 + 2] * s[2] + m.U[i * 4 + 3] * s[3]), 0.0);
	}
	for(int i = 0; i < 4; ++i) Y[i] = log(c[i]) - scale;
}

void hu_blen_host_sweep(const HuBlenTopo& tp, const HuBlenModel& m, const int32_t* parent, int64_t L, const double* blen, const int8_t* seq,
		double* up, double* down) {
	for(size_t h = tp.order.size(); h-- > 0;) {
		const int32_t u = tp.order[h];
		double* dst = up + (size_t) u * L * 4;
		const int32_t c0 = tp.childOff[u], c1 = tp.childOff[u + 1];
		if(c0 == c1) {
			const int8_t* row = seq + (size_t) u * L;
			for(int64_t j = 0; j < L; ++j) for(int i = 0; i < 4; ++i) dst[j * 4 + i] = row[j] >= 0 ? (i == row[j] ? 0.0 : -INFINITY) : m.logpi[i];
			continue;
		}
		for(int64_t j = 0; j < L; ++j) {
			double X[4] = {0, 0, 0, 0}, Y[4];
			for(int32_t c = c0; c < c1; ++c) { const int32_t v = tp.childIdx[c]; blen_conv(m, blen[v], up + ((size_t) v * L + j) * 4, Y); for(int i = 0; i < 4; ++i) X[i] += Y[i]; }
			for(int i = 0; i < 4; ++i) dst[j * 4 + i] = X[i];
		}
	}
	if(!down) return;
	for(size_t h = 1; h < tp.order.size(); ++h) {
		const int32_t u = tp.order[h], p = parent[u];
		double* dst = down + (size_t) u * L * 4;
		for(int64_t j = 0; j < L; ++j) {
			double X[4] = {0, 0, 0, 0}, Y[4];
			if(p != tp.root) { blen_conv(m, blen[p], down + ((size_t) p * L + j) * 4, Y); for(int i = 0; i < 4; ++i) X[i] += Y[i]; }
			for(int32_t c = tp.childOff[p]; c < tp.childOff[p + 1]; ++c) {
				const int32_t v = tp.childIdx[c];
				if(v == u) continue;
				blen_conv(m, blen[v], up + ((size_t) v * L + j) * 4, Y);
				for(int i = 0; i < 4; ++i) X[i] += Y[i];
			}
			for(int i = 0; i < 4; ++i) dst[j * 4 + i] = X[i];
		}
	}
}

double hu_blen_host_loglik(const HuBlenModel& m, int64_t L, const double* v) {
	double sum = 0;
	for(int64_t j = 0; j < L; ++j) sum += hu_blen_host_loglik_column(m, v + j * 4);
	return sum;
}

int64_t hu_blen_host_step(const HuBlenTopo& tp, const HuBlenModel& m, int64_t L, const double* t, const double* up, const double* down,
		double lo0, double hi0, double* t_star, double* f, double* d1, double* d2, uint8_t* capped) {
	std::vector<double> R((size_t) L * 3), K((size_t) L);
	int64_t nCap = 0;
	for(int32_t u = 0; u < tp.n; ++u) {
		if(capped) capped[u] = 0;
		if(u == tp.root) { if(t_star) t_star[u] = t[u]; if(f) f[u] = 0; if(d1) d1[u] = 0; if(d2) d2[u] = 0; continue; }
		for(int64_t j = 0; j < L; ++j) hu_blen_column(m, up + ((size_t) u * L + j) * 4, down + ((size_t) u * L + j) * 4, &R[(size_t) j * 3], &K[(size_t) j]);
		HuBlenExp E;
		auto eval = [&](double x, double* g, double* h) {
			hu_blen_exp(m, x, &E);
			double sg = 0, sh = 0;
			for(int64_t j = 0; j < L; ++j) { double a, b; hu_blen_terms(E, &R[(size_t) j * 3], &a, &b); sg += a; sh += b; }
			*g = sg; *h = sh;
		};
		double g0, h0;
		eval(t[u], &g0, &h0);
		if(f) { double s = 0; for(int64_t j = 0; j < L; ++j) s += K[(size_t) j] + log(hu_blen_den(E, &R[(size_t) j * 3])); f[u] = s; }
		if(d1) d1[u] = g0;
		if(d2) d2[u] = h0;
		if(!t_star) continue;
		int its = 0;
		t_star[u] = hu_blen_solve(t[u], g0, h0, lo0, hi0, eval, &its);
		if(its > HU_BLEN_MAX_NEWTON) { ++nCap; if(capped) capped[u] = 1; }
	}
	return nCap;
}

int hu_blen_rounds(const char* fn, hu_blen_opts* o, int32_t n, int32_t root, double* blen, const HuBlenOps& ops, double* sec) {
	std::vector<double> ts((size_t) n), cand((size_t) n);
	int rc;
	double t0 = hu_now_s();
	double ll = 0;
	if((rc = ops.sweep(blen, true)) != HU_OK || (rc = ops.loglik(&ll)) != HU_OK) return rc;
	sec[0] += hu_now_s() - t0;
	if(!(ll == ll) || ll == -INFINITY) { hu_set_error("%s: the log-likelihood of the start tree is %g: no objective to improve", fn, ll); return HU_ERR_ARG; }
	o->ll_start = o->ll_final = ll; o->n_rounds = 0; o->n_capped = 0; o->stop = HU_BLEN_MAX_ROUNDS;
	for(int32_t r = 0; r < o->max_rounds; ++r) {
		if(r > 0) { t0 = hu_now_s(); if((rc = ops.sweep(blen, true)) != HU_OK) return rc; sec[0] += hu_now_s() - t0; }
		t0 = hu_now_s();
		int64_t nCap = 0;
		if((rc = ops.step(blen, ts.data(), &nCap)) != HU_OK) return rc;
		sec[1] += hu_now_s() - t0;
		double delta = 0;
		for(int32_t u = 0; u < n; ++u) if(u != root) delta = std::max(delta, std::fabs(ts[(size_t) u] - blen[u]));
		if(delta <= o->eps) { o->stop = HU_BLEN_CONVERGED; return HU_OK; }
		t0 = hu_now_s();
		double s = 1.0, llNew = ll;
		bool taken = false;
		for(int k = 0; k < HU_BLEN_MAX_HALVINGS; ++k, s *= 0.5) {
			for(int32_t u = 0; u < n; ++u) cand[(size_t) u] = u == root ? blen[u] : blen[u] + s * (ts[(size_t) u] - blen[u]);
			if((rc = ops.sweep(cand.data(), false)) != HU_OK || (rc = ops.loglik(&llNew)) != HU_OK) return rc;
			if(llNew > ll) { taken = true; break; }
		}
		sec[2] += hu_now_s() - t0;
		if(!taken) { o->stop = HU_BLEN_NO_STEP; return HU_OK; }
		memcpy(blen, cand.data(), (size_t) n * 8);
		ll = llNew;
		if(o->rounds && o->n_rounds < o->rounds_cap) { hu_blen_round& R = o->rounds[o->n_rounds]; R.ll = ll; R.s = s; R.delta = delta; R.n_capped = nCap; }
		o->n_rounds++; o->n_capped += nCap; o->ll_final = ll;
	}
	return HU_OK;
}

/* ---- what the searches over topologies share ---- */
int HuBlenHost::fit(const char* fn, const hu_blen_opts* o, int32_t n, const int32_t* parent, double* blen, const int8_t* seq, double* ll) {
	hu_blen_opts bo = hu_search_fit_opts(*o);
	HuBlenTopo tp;
	int rc = hu_blen_check(fn, &bo, n, (int32_t) L, parent, blen, seq, 0, &tp);
	if(rc != HU_OK) return rc;
	HuBlenOps ops;
	ops.sweep = [&](const double* x, bool withDown) { sweep(tp, parent, x, seq, withDown); return (int) HU_OK; };
	ops.loglik = [&](double* out) { *out = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4); return (int) HU_OK; };
	ops.step = [&](const double* x, double* t, int64_t* c) { *c = hu_blen_host_step(tp, m, L, x, up.data(), down.data(), lo, hi, t, nullptr, nullptr, nullptr, nullptr); return (int) HU_OK; };
	double s4[4] = {0, 0, 0, 0};
	rc = hu_blen_rounds(fn, &bo, n, tp.root, blen, ops, s4);
	*ll = bo.ll_final;
	return rc;
}

int HuBlenHost::trial(const char* fn, const hu_blen_opts* o, int32_t n, const int32_t* parent, const double* blen, const int8_t* seq, double* ll) {
	HuBlenTopo tp;
	const int rc = hu_blen_check(fn, o, n, (int32_t) L, parent, blen, seq, 0, &tp);
	if(rc != HU_OK) return rc;
	sweep(tp, parent, blen, seq, false);
	*ll = hu_blen_host_loglik(m, L, up.data() + (size_t) tp.root * L * 4);
	return HU_OK;
}

bool hu_nni_halve(std::vector<int32_t>* taken) {
	if(taken->size() <= 1) return false;
	taken->resize((taken->size() + 1) / 2);
	return true;
}

int hu_search_rounds(const char* fn, const hu_blen_opts* bo, int32_t rounds, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuSearchOps& ops, double* ll_start, double* ll_final, int32_t* stop, double* sec) {
	const size_t N = (size_t) n, nIdx = child_off && child_idx ? (size_t) child_off[n] : 0;
	std::vector<int32_t> par(N), idx(nIdx), taken;
	std::vector<double> bl(N);
	HuBlenTopo tp;
	*stop = HU_SEARCH_MAX_ROUNDS;
	int rc;
	double ll = 0;
	for(int32_t r = 0; r <= rounds; ++r) {
		double t0 = hu_now_s();
		if((rc = ops.fit(parent, blen, &ll)) != HU_OK) return rc;
		sec[0] += hu_now_s() - t0;
		if(r == 0) *ll_start = ll;
		*ll_final = ll;
		if(r == rounds) break;                                  /* the fit after the last round allowed */
		t0 = hu_now_s();
		if((rc = hu_blen_check(fn, bo, n, cs_len, parent, blen, seq, 0, &tp)) != HU_OK) return rc;
		if((rc = ops.score(tp)) != HU_OK) return rc;
		sec[1] += hu_now_s() - t0;
		taken.clear();
		ops.select(tp, &taken);
		if(taken.empty()) { *stop = HU_SEARCH_LOCAL_OPTIMUM; return HU_OK; }
		const size_t nTaken = taken.size();
		t0 = hu_now_s();
		double llNew = ll;
		for(;;) {
			par.assign(parent, parent + N); bl.assign(blen, blen + N);
			if(nIdx) idx.assign(child_idx, child_idx + nIdx);
			if((rc = ops.apply(taken, par.data(), bl.data(), nIdx ? idx.data() : nullptr)) != HU_OK) return rc;
			if((rc = ops.trial(par.data(), bl.data(), &llNew)) != HU_OK) return rc;
			if(llNew > ll) break;
			if(!hu_nni_halve(&taken)) { sec[2] += hu_now_s() - t0; *stop = HU_SEARCH_NO_MOVE; return HU_OK; }
		}
		sec[2] += hu_now_s() - t0;
		memcpy(parent, par.data(), N * 4); memcpy(blen, bl.data(), N * 8);
		if(nIdx) memcpy(child_idx, idx.data(), nIdx * 4);
		ll = llNew; *ll_final = ll;
		ops.record(r + 1, ll, nTaken, taken);
	}
	return HU_OK;
}
