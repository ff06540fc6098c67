// hu_unifrac without a device: the checks, the plan of a call and the host path.  No HIP headers: a plain C++ compiler
// builds this file (tests/san/unifrac_driver.cpp).  The host path restates the definition of include/hmmufotu_amd.h in plain loops with
// the summation order of the kernels (hu_kern_unifrac.h): the column scan in blocks of HU_UF_SCAN_ROWS rows, the terms of a pair in
// ascending branch order within a slab, each product fused into its sum (fma), the slabs then in ascending order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>
#include "hu_unifrac.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_unifrac_default_opts(hu_unifrac_opts* o) {
	if(!o) return;
	o->method = HU_UF_WEIGHTED; o->host = 0; o->alpha = 0.5; o->slab = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_unifrac_default_slab(int64_t n_sample, int64_t n_branch) {
	if(n_sample < 1 || n_branch < 1) return 1;
	const int64_t tiles = hu_uf_tiles(n_sample);
	if(tiles >= HU_UF_WANT_WG) return n_branch;
	const int64_t want = (HU_UF_WANT_WG + tiles - 1) / tiles;
	const int64_t per = (n_branch + want - 1) / want;
	return std::max<int64_t>(256, (per + 31) / 32 * 32);
}

int hu_uf_plan(const char* fn, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, HuUfPlan& pl) {
	hu_unifrac_opts o;
	if(opts) o = *opts; else hu_unifrac_default_opts(&o);
	if(n_sample < 1) { hu_set_error("%s: a table without samples", fn); return HU_ERR_ARG; }
	if(n_otu < 0 || n_otu >= 0x7fffffffll || n_sample >= 0x7fffffffll || (n_otu > 0 && !counts)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(o.method < HU_UF_UNWEIGHTED || o.method > HU_UF_JACCARD) { hu_set_error("%s: unknown method %d", fn, o.method); return HU_ERR_ARG; }
	if(!(o.alpha >= 0 && o.alpha <= 1)) { hu_set_error("%s: alpha %g outside [0, 1]", fn, o.alpha); return HU_ERR_ARG; }
	if(o.method != HU_UF_GENERALIZED && o.alpha != 0.5) { hu_set_error("%s: alpha goes with the generalized method only", fn); return HU_ERR_ARG; }
	if(o.slab < 0) { hu_set_error("%s: slab %lld below 0", fn, (long long) o.slab); return HU_ERR_ARG; }
	const bool identity = o.method == HU_UF_BRAY_CURTIS || o.method == HU_UF_JACCARD;
	if(identity && tree) { hu_set_error("%s: bray-curtis and jaccard take no tree", fn); return HU_ERR_ARG; }
	if(!identity && (!tree || !tree->parent || !tree->blen || tree->n_nodes < 1 || (n_otu > 0 && !otu_node))) { hu_set_error("%s: the method needs a tree and the node of every OTU", fn); return HU_ERR_ARG; }
	const size_t M = (size_t) n_otu, S = (size_t) n_sample;
	/* the cells and the column totals */
	std::vector<double> tot(S, 0.0);
	for(size_t i = 0; i < M; ++i) for(size_t j = 0; j < S; ++j) {
		const double v = counts[i * S + j];
		if(!(v >= 0) || !std::isfinite(v)) { hu_set_error("%s: the cell of OTU %zu and sample %zu is negative or not finite", fn, i, j); return HU_ERR_ARG; }
		tot[j] += v;
	}
	for(size_t j = 0; j < S; ++j) if(!(tot[j] > 0)) {
		hu_set_error("%s: sample %zu has no reads: hmmufotu-amd-subset drops such samples", fn, j); return HU_ERR_ARG; }
	pl.M = n_otu; pl.S = n_sample; pl.host = o.host != 0; pl.budget = o.mem_budget; pl.alpha = o.alpha;
	pl.method = o.method == HU_UF_BRAY_CURTIS ? HU_UF_WEIGHTED : o.method == HU_UF_JACCARD ? HU_UF_UNWEIGHTED : o.method;
	if(pl.method == HU_UF_GENERALIZED && o.alpha == 1.0) pl.method = HU_UF_WEIGHTED;   /* s^1 |x - y| / s: the same terms */
	pl.perm.resize(M); pl.lo.clear(); pl.hi.clear(); pl.node.clear(); pl.b.clear();
	std::iota(pl.perm.begin(), pl.perm.end(), (int64_t) 0);
	pl.permIsIdentity = true;
	if(identity) {
		pl.B = n_otu;
		pl.lo.resize(M); pl.hi.resize(M); pl.node.resize(M); pl.b.assign(M, 1.0);
		for(size_t i = 0; i < M; ++i) { pl.lo[i] = (int32_t) i; pl.hi[i] = (int32_t) i + 1; pl.node[i] = (int32_t) i; }
	}
	else {
		const int32_t N = tree->n_nodes;
		const int32_t* par = tree->parent;
		int32_t root = -1;
		for(int32_t v = 0; v < N; ++v) {
			if(par[v] == -1) { if(root >= 0) { hu_set_error("%s: nodes %d and %d both have no parent", fn, root, v); return HU_ERR_ARG; } root = v; }
			else if(par[v] < 0 || par[v] >= N || par[v] == v) { hu_set_error("%s: node %d has the parent %d", fn, v, par[v]); return HU_ERR_ARG; }
		}
		if(root < 0) { hu_set_error("%s: the tree has no root", fn); return HU_ERR_ARG; }
		for(size_t i = 0; i < M; ++i) if(otu_node[i] < 0 || otu_node[i] >= N) {
			hu_set_error("%s: OTU %zu names node %d, the tree has %d", fn, i, otu_node[i], N); return HU_ERR_ARG; }
		/* the kept nodes: every node on a path from a row's node to the root; a walk stops at the first node another walk has kept */
		std::vector<uint8_t> kept((size_t) N, 0);
		int64_t nKept = 0;
		for(size_t i = 0; i < M; ++i) {
			int64_t steps = 0;
			for(int32_t v = otu_node[i]; v >= 0 && !kept[(size_t) v]; v = par[v]) {
				kept[(size_t) v] = 1; ++nKept;
				if(++steps > N) break;
			}
		}
		if(M > 0 && !kept[(size_t) root]) { hu_set_error("%s: the parents of the tree form a cycle", fn); return HU_ERR_ARG; }
		/* every kept node but the root hangs on a kept parent: a cycle among kept nodes would have left the root out */
		std::vector<int32_t> childOff((size_t) N + 1, 0), childIdx;
		for(int32_t v = 0; v < N; ++v) if(kept[(size_t) v] && v != root) ++childOff[(size_t) par[v] + 1];
		for(int32_t v = 0; v < N; ++v) childOff[(size_t) v + 1] += childOff[(size_t) v];
		childIdx.resize((size_t) childOff[(size_t) N]);
		{
			std::vector<int32_t> fill(childOff.begin(), childOff.end() - 1);
			for(int32_t v = 0; v < N; ++v) if(kept[(size_t) v] && v != root) childIdx[(size_t) fill[(size_t) par[v]]++] = v;   /* ascending node number */
		}
		std::vector<int32_t> pre((size_t) N, -1), end((size_t) N, -1), order;
		order.reserve((size_t) nKept);
		if(M > 0) {
			std::vector<std::pair<int32_t, int32_t>> st;                   /* node, its next child */
			st.emplace_back(root, childOff[(size_t) root]);
			pre[(size_t) root] = 0; order.push_back(root);
			while(!st.empty()) {
				const int32_t v = st.back().first;
				if(st.back().second < childOff[(size_t) v + 1]) {
					const int32_t c = childIdx[(size_t) st.back().second++];
					pre[(size_t) c] = (int32_t) order.size(); order.push_back(c);
					st.emplace_back(c, childOff[(size_t) c]);
				}
				else { end[(size_t) v] = (int32_t) order.size(); st.pop_back(); }
			}
			if((int64_t) order.size() != nKept) { hu_set_error("%s: the parents of the tree form a cycle", fn); return HU_ERR_ARG; }
		}
		const size_t B = order.empty() ? 0 : order.size() - 1;
		pl.B = (int64_t) B;
		std::stable_sort(pl.perm.begin(), pl.perm.end(), [&](int64_t a, int64_t c) { return pre[(size_t) otu_node[a]] < pre[(size_t) otu_node[c]]; });
		for(size_t q = 0; q < M; ++q) if(pl.perm[q] != (int64_t) q) { pl.permIsIdentity = false; break; }
		std::vector<int32_t> pos(M);
		for(size_t q = 0; q < M; ++q) pos[q] = pre[(size_t) otu_node[pl.perm[q]]];
		pl.lo.resize(B); pl.hi.resize(B); pl.node.resize(B); pl.b.resize(B);
		for(size_t k = 0; k < B; ++k) {
			const int32_t v = order[k + 1];
			const double len = tree->blen[v];
			if(!(len >= 0) || !std::isfinite(len)) { hu_set_error("%s: the branch above node %d has the length %g", fn, v, len); return HU_ERR_ARG; }
			pl.node[k] = v; pl.b[k] = len;
			pl.lo[k] = (int32_t)(std::lower_bound(pos.begin(), pos.end(), pre[(size_t) v]) - pos.begin());
			pl.hi[k] = (int32_t)(std::lower_bound(pos.begin(), pos.end(), end[(size_t) v]) - pos.begin());
		}
	}
	pl.L = o.slab > 0 ? o.slab : hu_unifrac_default_slab(n_sample, pl.B);
	pl.nSlab = pl.B > 0 ? (pl.B + pl.L - 1) / pl.L : 0;
	if(pl.nSlab > 65535) { hu_set_error("%s: %lld slabs of %lld branches: more than a grid holds, raise the slab", fn, (long long) pl.nSlab, (long long) pl.L); return HU_ERR_ARG; }
	return HU_OK;
}

void hu_uf_host_embed(const HuUfPlan& pl, const double* counts, double* P) {
	const size_t M = (size_t) pl.M, S = (size_t) pl.S, B = (size_t) pl.B;
	/* C [M + 1][S]: row q + 1 = the sum of the first q + 1 rows in depth-first order, as the scan kernels add them */
	std::vector<double> C((M + 1) * S, 0.0);
	const size_t nBlk = (M + HU_UF_SCAN_ROWS - 1) / HU_UF_SCAN_ROWS;
	std::vector<double> off(S, 0.0), sum(S);
	for(size_t blk = 0; blk < nBlk; ++blk) {
		const size_t q0 = blk * HU_UF_SCAN_ROWS, q1 = std::min(M, q0 + HU_UF_SCAN_ROWS);
		std::fill(sum.begin(), sum.end(), 0.0);
		for(size_t q = q0; q < q1; ++q) { const double* row = counts + (size_t) pl.perm[q] * S; for(size_t j = 0; j < S; ++j) sum[j] += row[j]; }
		std::vector<double> run(off);
		for(size_t q = q0; q < q1; ++q) {
			const double* row = counts + (size_t) pl.perm[q] * S;
			for(size_t j = 0; j < S; ++j) { run[j] += row[j]; C[(q + 1) * S + j] = run[j]; }
		}
		for(size_t j = 0; j < S; ++j) off[j] += sum[j];
	}
	const double* T = C.data() + M * S;
	for(size_t k = 0; k < B; ++k) {
		const double *a = C.data() + (size_t) pl.hi[k] * S, *c = C.data() + (size_t) pl.lo[k] * S;
		for(size_t j = 0; j < S; ++j) P[k * S + j] = (a[j] - c[j]) / T[j];
	}
}

template<int METHOD> static inline void uf_term(double b, double x, double y, double alpha, double& num, double& den) {
	if(METHOD == HU_UF_UNWEIGHTED) {
		const double xi = x > 0 ? 1.0 : 0.0, yi = y > 0 ? 1.0 : 0.0;
		num = std::fma(b, std::fabs(xi - yi), num); den = std::fma(b, std::fmax(xi, yi), den);
	}
	else if(METHOD == HU_UF_WEIGHTED) { num = std::fma(b, std::fabs(x - y), num); den = std::fma(b, x + y, den); }
	else if(METHOD == HU_UF_WEIGHTED_RAW) num = std::fma(b, std::fabs(x - y), num);
	else {
		const double s = x + y;
		if(s > 0) {
			const double pw = alpha == 0.5 ? std::sqrt(s) : std::pow(s, alpha);
			num = std::fma(b * pw, std::fabs(x - y) / s, num); den = std::fma(b, pw, den);
		}
	}
}

template<int METHOD> static void uf_pairs(const HuUfPlan& pl, const double* P, double* dist) {
	const size_t S = (size_t) pl.S, B = (size_t) pl.B, L = (size_t) pl.L;
	for(size_t i = 0; i < S; ++i) {
		dist[i * S + i] = 0.0;
		for(size_t j = i + 1; j < S; ++j) {
			double N = 0.0, D = 0.0;
			for(size_t k0 = 0; k0 < B; k0 += L) {
				double num = 0.0, den = 0.0;
				const size_t k1 = std::min(B, k0 + L);
				for(size_t k = k0; k < k1; ++k) uf_term<METHOD>(pl.b[k], P[k * S + i], P[k * S + j], pl.alpha, num, den);
				N += num; D += den;
			}
			const double d = METHOD == HU_UF_WEIGHTED_RAW ? N : D > 0 ? N / D : 0.0;
			dist[i * S + j] = d; dist[j * S + i] = d;
		}
	}
}

void hu_uf_host_pairs(const HuUfPlan& pl, const double* P, double* dist, double* pd) {
	switch(pl.method) {
	case HU_UF_UNWEIGHTED: uf_pairs<HU_UF_UNWEIGHTED>(pl, P, dist); break;
	case HU_UF_WEIGHTED: uf_pairs<HU_UF_WEIGHTED>(pl, P, dist); break;
	case HU_UF_WEIGHTED_RAW: uf_pairs<HU_UF_WEIGHTED_RAW>(pl, P, dist); break;
	default: uf_pairs<HU_UF_GENERALIZED>(pl, P, dist); break;
	}
	if(!pd) return;
	const size_t S = (size_t) pl.S, B = (size_t) pl.B, L = (size_t) pl.L;
	for(size_t j = 0; j < S; ++j) {
		double tot = 0.0;
		for(size_t k0 = 0; k0 < B; k0 += L) {
			double acc = 0.0;
			const size_t k1 = std::min(B, k0 + L);
			for(size_t k = k0; k < k1; ++k) acc += P[k * S + j] > 0 ? pl.b[k] : 0.0;
			tot += acc;
		}
		pd[j] = tot;
	}
}
