// The checks, the walk, the host path, the selection and the round loop of the SPR search: hmmufotu-amd-tree
// --ml-lengths --spr --host, the reference of the device tests, and what tests/san/spr_driver.cpp runs under the sanitizers.  No HIP
// headers: a plain C++ compiler builds this file.  The arithmetic of a column is hu_tree_spr.h's, shared with the kernel; the sweeps,
// the fit's round loop, the search's round loop (hu_search_rounds) and the Newton rule are hu_blen_host.cpp's and hu_tree_blen.h's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include "hu_tree_spr.h"

extern "C" void hu_spr_default_opts(hu_spr_opts* o) {
	if(!o) return;
	memset(o, 0, sizeof(*o));
	hu_blen_default_opts(&o->blen);
	o->min_gain = 1e-3; o->radius = 5; o->spr_rounds = 10;
}

/* the scratch of one workgroup: the stack of recomputed messages and, beyond what LDS holds, the ratios */
static int64_t spr_wg_bytes(int32_t cs_len, int32_t radius) {
	return (int64_t) radius * 32 * cs_len + (cs_len > HU_BLEN_LDS_COLS ? 24 * (int64_t) cs_len : 0);
}

extern "C" int64_t hu_spr_need(int32_t n, int32_t cs_len, int32_t radius) {
	if(n < 1 || cs_len < 1 || radius < 1 || radius > HU_SPR_MAX_RADIUS) return 0;
	const int64_t nodes = n > 1 ? n - 1 : 1;
	const int64_t perNode = std::min<int64_t>(((int64_t) 1 << (radius + 2)) - 3, n);
	const int64_t wg = spr_wg_bytes(cs_len, radius);
	return hu_blen_need(n, cs_len) + 32 * nodes + std::min<int64_t>(96 * perNode * nodes, HU_SPR_REC_BYTES) + std::max(wg, std::min<int64_t>(wg * nodes, HU_SPR_SLAB_BYTES));
}

int64_t hu_spr_slab_nodes(const hu_spr_opts* o, int32_t cs_len) {
	const int64_t fit = std::max<int64_t>(HU_SPR_SLAB_BYTES / spr_wg_bytes(cs_len, o->radius), 1);
	return o->slab > 0 ? std::min<int64_t>(o->slab, fit) : fit;
}

int hu_spr_check(const char* fn, const hu_spr_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		int32_t dg_k, HuBlenTopo* tp) {
	if(!o) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(o->blen.mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	hu_blen_opts bo = o->blen;
	bo.mem_budget = 0;                                          /* the budget is held against the search's need below, not the fit's */
	int rc = hu_blen_check(fn, &bo, n, cs_len, parent, blen, seq, dg_k, tp);
	if(rc != HU_OK) return rc;
	if(o->radius < 1 || o->radius > HU_SPR_MAX_RADIUS) { hu_set_error("%s: a radius of %d: 1 to %d", fn, o->radius, HU_SPR_MAX_RADIUS); return HU_ERR_ARG; }
	if(o->spr_rounds < 1) { hu_set_error("%s: %d SPR rounds: at least 1", fn, o->spr_rounds); return HU_ERR_ARG; }
	if(!(o->min_gain > 0) || !std::isfinite(o->min_gain)) { hu_set_error("%s: a smallest gain of %g: it must be above 0", fn, o->min_gain); return HU_ERR_ARG; }
	if(o->slab < 0) { hu_set_error("%s: a slab of %d prune nodes", fn, o->slab); return HU_ERR_ARG; }
	if(o->rounds_cap < 0 || (o->rounds_cap > 0 && !o->rounds) || o->moves_cap < 0 || (o->moves_cap > 0 && !o->moves)) {
		hu_set_error("%s: round or move records without a place for them", fn); return HU_ERR_ARG; }
	const int64_t need = hu_spr_need(n, cs_len, o->radius);
	if(o->blen.mem_budget > 0 && need > o->blen.mem_budget) {
		hu_set_error("%s: %d nodes of %d columns at radius %d need %lld bytes (%lld of them for the messages), the memory budget is %lld bytes", fn, n, cs_len,
			o->radius, (long long) need, (long long)(64 * (int64_t) n * cs_len), (long long) o->blen.mem_budget);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

void hu_spr_prunable(const HuBlenTopo& tp, const int32_t* parent, std::vector<int32_t>* nodes, int64_t* skipped) {
	nodes->clear(); *skipped = 0;
	for(int32_t v = 0; v < tp.n; ++v) {
		if(v == tp.root) continue;
		const int32_t p = parent[v];
		if(p == tp.root || tp.childOff[p + 1] - tp.childOff[p] != 2) { ++*skipped; continue; }
		nodes->push_back(v);
	}
}

namespace {
struct Walk {
	const HuBlenTopo& tp; const int32_t* parent; const double* blen; int32_t n, radius, out;
	std::vector<HuSprRec>* recs;
	struct Nb { int32_t node, msg, w; double len; };           /* a neighbour, its message towards the node, the edge's lower end and length */

	/* arrived at X over an edge of length inLen whose far side is the message inSrc: from the child fromChild, or from the parent (-1).
	 * Every other edge at X is a target at distance d; slot d - 1 holds the message that leaves X through it */
	void visit(int32_t X, int32_t fromChild, int32_t inSrc, double inLen, int32_t d) {
		std::vector<Nb> nb;
		for(int32_t c = tp.childOff[X]; c < tp.childOff[X + 1]; ++c) { const int32_t ch = tp.childIdx[c]; if(ch != fromChild) nb.push_back({ch, ch, ch, blen[ch]}); }
		if(fromChild >= 0 && X != tp.root) nb.push_back({parent[X], n + X, X, blen[X]});
		const int32_t slot = d - 1;
		for(size_t k = 0; k < nb.size(); ++k) {
			HuSprRec r; memset(&r, 0, sizeof(r));
			r.src0 = inSrc; r.len0 = inLen; r.src1 = -1; r.dst = slot; r.sa = r.sb = r.tnode = -1;
			bool open = true;                                       /* r holds a message and waits for a second one */
			for(size_t i = 0; i < nb.size(); ++i) {
				if(i == k) continue;
				if(open) { r.src1 = nb[i].msg; r.len1 = nb[i].len; recs->push_back(r); open = false; continue; }
				memset(&r, 0, sizeof(r));
				r.src0 = nb[i].msg; r.len0 = nb[i].len; r.src1 = -1; r.dst = slot; r.acc = 1; r.sa = r.sb = r.tnode = -1;
				open = true;
			}
			if(open) recs->push_back(r);
			HuSprRec& last = recs->back();
			last.sa = 2 * n + slot; last.sb = nb[k].msg; last.la = last.lb = 0.5 * nb[k].len; last.tnode = nb[k].w; last.dist = d; last.out = out++;
			if(d < radius) {
				if(nb[k].w == nb[k].node) visit(nb[k].node, -1, 2 * n + slot, nb[k].len, d + 1);
				else visit(nb[k].node, X, 2 * n + slot, nb[k].len, d + 1);
			}
		}
	}
};
}

int32_t hu_spr_walk(const HuBlenTopo& tp, const int32_t* parent, const double* blen, int32_t radius, int32_t v, std::vector<HuSprRec>* recs) {
	const int32_t n = tp.n, p = parent[v], g = parent[p];
	const int32_t s = tp.childIdx[tp.childOff[p]] == v ? tp.childIdx[tp.childOff[p] + 1] : tp.childIdx[tp.childOff[p]];
	HuSprRec b; memset(&b, 0, sizeof(b));
	b.src0 = b.src1 = b.dst = -1; b.sa = s; b.la = blen[s]; b.sb = n + p; b.lb = blen[p]; b.tnode = s; b.dist = 0; b.out = 0;
	recs->push_back(b);
	Walk w{tp, parent, blen, n, radius, 1, recs};
	const double merged = blen[s] + blen[p];
	w.visit(s, -1, n + p, merged, 1);
	w.visit(g, p, s, merged, 1);
	return w.out;
}

void hu_spr_host_score(const HuBlenModel& m, int32_t n, int64_t L, const HuSprNode* nodes, size_t nNodes, const HuSprRec* recs, int64_t recBase, int64_t outBase,
		const double* up, const double* down, double lo, double hi, double* stack, double* t_star, double* f, double* f0) {
	std::vector<double> R((size_t) L * 3);
	auto msg = [&](int32_t id) -> const double* { return id < n ? up + (size_t) id * L * 4 : id < 2 * n ? down + (size_t)(id - n) * L * 4 : stack + (size_t)(id - 2 * n) * L * 4; };
	for(size_t b = 0; b < nNodes; ++b) {
		const HuSprNode& nd = nodes[b];
		const double* yv = up + (size_t) nd.v * L * 4;
		for(int32_t ri = 0; ri < nd.nRec; ++ri) {
			const HuSprRec& rc = recs[nd.recOff - recBase + ri];
			double P[64];
			for(int i = 0; i < 64; ++i) P[i] = hu_nni_pentry(m, i < 16 ? rc.len0 : i < 32 ? rc.len1 : i < 48 ? rc.la : rc.lb, (i >> 2) & 3, i & 3);
			if(rc.dst >= 0) {
				const double* s0 = msg(rc.src0); const double* s1 = rc.src1 >= 0 ? msg(rc.src1) : nullptr;
				double* dst = stack + (size_t) rc.dst * L * 4;
				for(int64_t j = 0; j < L; ++j) {
					double Y[4], Z[4];
					hu_spr_conv(P, s0 + j * 4, Y);
					if(s1) { hu_spr_conv(P + 16, s1 + j * 4, Z); for(int i = 0; i < 4; ++i) Y[i] += Z[i]; }
					if(rc.acc) for(int i = 0; i < 4; ++i) Y[i] += dst[j * 4 + i];
					for(int i = 0; i < 4; ++i) dst[j * 4 + i] = Y[i];
				}
			}
			if(rc.tnode < 0) continue;
			const double* A = msg(rc.sa); const double* B = msg(rc.sb);
			double sumK = 0;
			for(int64_t j = 0; j < L; ++j) { double K; hu_spr_column(m, P + 32, A + j * 4, P + 48, B + j * 4, yv + j * 4, &R[(size_t) j * 3], &K); sumK += K; }
			HuBlenExp E;
			auto eval = [&](double x, double* g, double* h) {
				hu_blen_exp(m, x, &E);
				double sg = 0, sh = 0;
				for(int64_t j = 0; j < L; ++j) { double a, c; hu_blen_terms(E, &R[(size_t) j * 3], &a, &c); sg += a; sh += c; }
				*g = sg; *h = sh;
			};
			auto value = [&](double x) {
				hu_blen_exp(m, x, &E);
				double s = 0;
				for(int64_t j = 0; j < L; ++j) s += log(hu_blen_den(E, &R[(size_t) j * 3]));
				return sumK + s;
			};
			double g0, h0;
			eval(nd.t0, &g0, &h0);
			if(rc.dist == 0) f0[b] = value(nd.t0);
			int its = 0;
			const double x = hu_blen_solve(nd.t0, g0, h0, lo, hi, eval, &its);
			const int64_t o = nd.outOff - outBase + rc.out;
			t_star[o] = x; f[o] = value(x);
		}
	}
}

int hu_spr_scores(const char* fn, const hu_spr_opts* o, const HuBlenTopo& tp, int32_t cs_len, const int32_t* parent, const double* blen, bool count_only,
		const HuSprSlabFn& slab, HuSprScores* out) {
	std::vector<int32_t> pr;
	hu_spr_prunable(tp, parent, &pr, &out->skipped);
	out->v = pr; out->off.assign(pr.size() + 1, 0);
	out->w.clear(); out->dist.clear(); out->t.clear(); out->f.clear();
	out->baseT.assign(pr.size(), 0.0); out->baseF.assign(pr.size(), 0.0); out->f0.assign(pr.size(), 0.0);
	const size_t maxNodes = (size_t) hu_spr_slab_nodes(o, cs_len), maxRecs = (size_t)(HU_SPR_REC_BYTES / 96);
	std::vector<HuSprRec> recs, one;
	std::vector<HuSprNode> nodes;
	std::vector<double> ts, f, f0;
	int64_t nOut = 0;
	auto flush = [&](size_t first) -> int {
		if(nodes.empty()) return HU_OK;
		ts.assign((size_t) nOut, 0.0); f.assign((size_t) nOut, 0.0); f0.assign(nodes.size(), 0.0);
		const int rc = slab(nodes.data(), nodes.size(), recs.data(), recs.size(), 0, 0, (size_t) nOut, ts.data(), f.data(), f0.data());
		if(rc != HU_OK) return rc;
		for(size_t b = 0; b < nodes.size(); ++b) {
			const size_t o0 = (size_t) nodes[b].outOff;
			out->baseT[first + b] = ts[o0]; out->baseF[first + b] = f[o0]; out->f0[first + b] = f0[b];
			for(int32_t ri = 0; ri < nodes[b].nRec; ++ri) {
				const HuSprRec& r = recs[(size_t) nodes[b].recOff + ri];
				if(r.tnode < 0 || r.dist == 0) continue;
				out->w.push_back(r.tnode); out->dist.push_back(r.dist); out->t.push_back(ts[o0 + r.out]); out->f.push_back(f[o0 + r.out]);
			}
		}
		nodes.clear(); recs.clear(); nOut = 0;
		return HU_OK;
	};
	size_t first = 0;
	for(size_t i = 0; i < pr.size(); ++i) {
		one.clear();
		const int32_t k = hu_spr_walk(tp, parent, blen, o->radius, pr[i], &one);
		out->off[i + 1] = out->off[i] + (k - 1);
		if(count_only) continue;
		if(one.size() > maxRecs) { hu_set_error("%s: the walk of node %d takes %zu steps, a launch holds %zu: polytomies this large are not walked", fn, pr[i], one.size(), maxRecs); return HU_ERR_NOMEM; }
		if(nodes.size() >= maxNodes || recs.size() + one.size() > maxRecs) { const int rc = flush(first); if(rc != HU_OK) return rc; first = i; }
		HuSprNode nd; memset(&nd, 0, sizeof(nd));
		nd.recOff = (int64_t) recs.size(); nd.outOff = nOut; nd.nRec = (int32_t) one.size(); nd.v = pr[i]; nd.t0 = blen[pr[i]];
		nodes.push_back(nd); recs.insert(recs.end(), one.begin(), one.end()); nOut += k;
	}
	return count_only ? (int) HU_OK : flush(first);
}

/* ---- the regraft on the arrays ---- */
int hu_spr_apply(const char* fn, int32_t n, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t v, int32_t w, double t) {
	if(!parent || !blen || n < 2) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(!(t >= 0) || !std::isfinite(t)) { hu_set_error("%s: a pendant length of %g", fn, t); return HU_ERR_ARG; }
	if((child_off == nullptr) != (child_idx == nullptr)) { hu_set_error("%s: child_off and child_idx go together", fn); return HU_ERR_ARG; }
	int32_t root = -1;
	std::vector<int32_t> deg((size_t) n, 0);
	for(int32_t i = 0; i < n; ++i) {
		if(parent[i] < 0) { if(root >= 0) { hu_set_error("%s: the tree has more than one root", fn); return HU_ERR_ARG; } root = i; }
		else if(parent[i] >= n || parent[i] == i) { hu_set_error("%s: parent of node %d out of range", fn, i); return HU_ERR_ARG; }
		else deg[(size_t) parent[i]]++;
	}
	if(root < 0) { hu_set_error("%s: the tree has no root", fn); return HU_ERR_ARG; }
	if(child_off) for(int32_t i = 0; i < n; ++i) if(child_off[i + 1] - child_off[i] != deg[(size_t) i]) {
		hu_set_error("%s: child_off gives node %d another number of children than parent", fn, i); return HU_ERR_ARG; }
	if(v < 0 || v >= n || v == root || parent[v] == root || deg[(size_t) parent[v]] != 2) {
		hu_set_error("%s: node %d is not prunable: its parent must have two children and must not be the root", fn, v); return HU_ERR_ARG; }
	const int32_t p = parent[v], g = parent[p];
	int32_t s = -1;
	for(int32_t i = 0; i < n; ++i) if(parent[i] == p && i != v) s = i;
	if(w < 0 || w >= n || w == root || w == v || w == p) { hu_set_error("%s: node %d names no edge the subtree of %d can go into", fn, w, v); return HU_ERR_ARG; }
	if(w == s) { hu_set_error("%s: the edge above node %d is where the subtree of %d hangs: no move", fn, w, v); return HU_ERR_ARG; }
	int32_t steps = 0;
	for(int32_t x = w; x >= 0; x = parent[x]) {
		if(x == v) { hu_set_error("%s: node %d lies inside the subtree of %d", fn, w, v); return HU_ERR_ARG; }
		if(++steps > n) { hu_set_error("%s: the tree is not connected", fn); return HU_ERR_ARG; }
	}
	const int32_t pw = parent[w];
	if(child_off) {
		int32_t ip = -1, iw = -1, is = -1;
		for(int32_t c = child_off[g]; c < child_off[g + 1]; ++c) if(child_idx[c] == p) ip = c;
		for(int32_t c = child_off[pw]; c < child_off[pw + 1]; ++c) if(child_idx[c] == w) iw = c;
		for(int32_t c = child_off[p]; c < child_off[p + 1]; ++c) if(child_idx[c] == s) is = c;
		if(ip < 0 || iw < 0 || is < 0) { hu_set_error("%s: child_idx and parent disagree", fn); return HU_ERR_ARG; }
		child_idx[ip] = s; child_idx[iw] = p; child_idx[is] = w;
	}
	const double half = 0.5 * blen[w];
	parent[s] = g; parent[p] = pw; parent[w] = p;
	blen[s] = blen[s] + blen[p]; blen[w] = half; blen[p] = half; blen[v] = t;
	return HU_OK;
}

extern "C" int hu_tree_spr_apply(int32_t n, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t v, int32_t w, double t) try {
	return hu_spr_apply("hu_tree_spr_apply", n, parent, blen, child_off, child_idx, v, w, t);
} catch(...) { return hu_catch_all("hu_tree_spr_apply"); }

/* ---- the round loop ---- */
namespace {
struct Cand { int32_t v, w, dist, s; double t, gain; };
}

int hu_spr_rounds(const char* fn, hu_spr_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq, const int32_t* child_off,
		int32_t* child_idx, const HuSprOps& ops, double* sec) {
	const size_t N = (size_t) n;
	std::vector<int32_t> stamp(N);
	std::vector<Cand> cand;
	HuSprScores sc;
	o->n_rounds = 0; o->n_moves = 0; o->skipped = 0;
	HuSearchOps so;
	so.fit = ops.fit; so.trial = ops.trial;
	so.score = [&](const HuBlenTopo& tp) { return ops.score(parent, blen, tp, &sc); };
	so.select = [&](const HuBlenTopo& tp, std::vector<int32_t>* taken) {
		o->skipped = sc.skipped;
		/* the best target of every pruned node: the largest f, the smaller w among equals */
		cand.clear();
		for(size_t i = 0; i < sc.v.size(); ++i) {
			int64_t best = -1;
			for(int64_t k = sc.off[i]; k < sc.off[i + 1]; ++k)
				if(best < 0 || sc.f[(size_t) k] > sc.f[(size_t) best] || (sc.f[(size_t) k] == sc.f[(size_t) best] && sc.w[(size_t) k] < sc.w[(size_t) best])) best = k;
			if(best < 0) continue;
			const double gain = sc.f[(size_t) best] - sc.baseF[i];
			if(!(gain > o->min_gain)) continue;
			const int32_t v = sc.v[i], p = parent[v];
			const int32_t s = tp.childIdx[tp.childOff[p]] == v ? tp.childIdx[tp.childOff[p] + 1] : tp.childIdx[tp.childOff[p]];
			cand.push_back({v, sc.w[(size_t) best], sc.dist[(size_t) best], s, sc.t[(size_t) best], gain});
		}
		std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.gain != b.gain ? a.gain > b.gain : a.v != b.v ? a.v < b.v : a.w < b.w; });
		/* taken: none of its own nodes and none on the path from p to w is marked by one taken before */
		std::vector<char> used(N, 0);
		std::vector<int32_t> mine;
		std::fill(stamp.begin(), stamp.end(), -1);
		for(size_t c = 0; c < cand.size(); ++c) {
			const Cand& x = cand[c];
			const int32_t p = parent[x.v], g = parent[p];
			mine.assign({x.v, p, x.s, g, x.w, parent[x.w]});
			for(int32_t a = p; a >= 0; a = parent[a]) stamp[(size_t) a] = (int32_t) c;
			int32_t meet = x.w;
			for(; stamp[(size_t) meet] != (int32_t) c; meet = parent[meet]) mine.push_back(meet);
			for(int32_t a = p; a != meet; a = parent[a]) mine.push_back(a);
			mine.push_back(meet);
			bool freeOf = true;
			for(int32_t a : mine) if(used[(size_t) a]) freeOf = false;
			if(!freeOf) continue;
			for(int32_t a : mine) used[(size_t) a] = 1;
			taken->push_back((int32_t) c);
		}
	};
	so.apply = [&](const std::vector<int32_t>& taken, int32_t* par, double* bl, int32_t* idx) {
		for(int32_t c : taken) {
			const Cand& x = cand[(size_t) c];
			if(hu_spr_apply(fn, n, par, bl, idx ? child_off : nullptr, idx, x.v, x.w, x.t) != HU_OK) return (int) HU_ERR_STATE;
		}
		return (int) HU_OK;
	};
	so.record = [&](int32_t round, double ll, size_t nTaken, const std::vector<int32_t>& taken) {
		if(o->rounds && o->n_rounds < o->rounds_cap) {
			hu_spr_round& R = o->rounds[o->n_rounds];
			R.ll = ll; R.targets = (int64_t) sc.w.size(); R.pruned = (int32_t) sc.v.size(); R.candidates = (int32_t) cand.size(); R.taken = (int32_t) nTaken; R.applied = (int32_t) taken.size();
		}
		for(int32_t c : taken) {
			if(o->moves && o->n_moves < o->moves_cap) {
				const Cand& x = cand[(size_t) c];
				int32_t* mv = o->moves + o->n_moves * 5;
				mv[0] = round; mv[1] = x.v; mv[2] = x.s; mv[3] = x.w; mv[4] = x.dist;
			}
			o->n_moves++;
		}
		o->n_rounds++;
	};
	return hu_search_rounds(fn, &o->blen, o->spr_rounds, n, cs_len, parent, blen, seq, child_off, child_idx, so, &o->ll_start, &o->ll_final, &o->stop, sec);
}

/* ---- the host path of the two entries ---- */
static HuSprSlabFn host_slab(const hu_spr_opts* o, const HuBlenModel& m, int32_t n, int64_t L, const double* up, const double* down, std::vector<double>* stack) {
	return [=, &m](const HuSprNode* nodes, size_t nNodes, const HuSprRec* recs, size_t, int64_t recBase, int64_t outBase, size_t, double* ts, double* f, double* f0) {
		stack->assign((size_t) o->radius * (size_t) L * 4, 0.0);
		hu_spr_host_score(m, n, L, nodes, nNodes, recs, recBase, outBase, up, down, o->blen.min_len, o->blen.max_len, stack->data(), ts, f, f0);
		return (int) HU_OK;
	};
}

int hu_spr_host_scores_entry(const char* fn, const hu_spr_opts* o, int32_t n, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const HuBlenModel& m, bool count_only, HuSprScores* out) {
	HuBlenTopo tp;
	int rc = hu_spr_check(fn, o, n, cs_len, parent, blen, seq, 0, &tp);
	if(rc != HU_OK) return rc;
	if(count_only) return hu_spr_scores(fn, o, tp, cs_len, parent, blen, true, HuSprSlabFn(), out);
	const size_t cells = (size_t) n * (size_t) cs_len * 4;
	std::vector<double> up(cells), down(cells), stack;
	hu_blen_host_sweep(tp, m, parent, cs_len, blen, seq, up.data(), down.data());
	return hu_spr_scores(fn, o, tp, cs_len, parent, blen, false, host_slab(o, m, n, cs_len, up.data(), down.data(), &stack), out);
}

int hu_spr_host_search_entry(const char* fn, hu_spr_opts* o, int32_t n, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const HuBlenModel& m, double* sec) {
	HuBlenTopo tp0;
	int rc = hu_spr_check(fn, o, n, cs_len, parent, blen, seq, 0, &tp0);
	if(rc != HU_OK) return rc;
	HuBlenHost h(m, n, cs_len, o->blen);
	std::vector<double> stack;
	HuSprOps ops;
	ops.fit = [&](const int32_t* par, double* b, double* ll) { return h.fit(fn, &o->blen, n, par, b, seq, ll); };
	ops.score = [&](const int32_t* par, const double* b, const HuBlenTopo& tp, HuSprScores* out) {
		h.sweep(tp, par, b, seq, true);
		return hu_spr_scores(fn, o, tp, cs_len, par, b, false, host_slab(o, m, n, cs_len, h.up.data(), h.down.data(), &stack), out);
	};
	ops.trial = [&](const int32_t* par, const double* b, double* ll) { return h.trial(fn, &o->blen, n, par, b, seq, ll); };
	return hu_spr_rounds(fn, o, n, cs_len, parent, blen, seq, child_off, child_idx, ops, sec);
}
