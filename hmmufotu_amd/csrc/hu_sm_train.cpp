// hmmufotu-train-sm without its counting loops, host only: which leaf rows are compared
// (PTUnrooted::getModelTraningSetGojobori / Goldman, src/PhyloTreeUnrooted.cpp:449-486), the trainers of the six models
// (trainParams of src/GTR.cpp:92-122, src/TN93.cpp:88-102, src/HKY85.cpp:86-98, src/F81.cpp:84-89, src/K80.cpp:81-89, src/JC69.h:79-80)
// and the text of DNASubModel::write.  The counts between the first and the second come from the device (hu_sm_counts, hu_kern_sm.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "hu_common.h"

static const double SM_MAX_PDIST = 0.15;     /* DNASubModel::MAX_PDIST, src/DNASubModel.cpp:39 */

extern "C" int hu_sm_training_set(int32_t n_nodes, const int32_t* parent, const int32_t* child_off, const int32_t* child_idx, const int32_t* row_of,
		int method, int32_t* items, int64_t* n_items) try {
	const char* fn = "hu_sm_training_set";
	if(n_nodes < 1 || !parent || !child_off || !child_idx || !row_of || !items || !n_items || (method != HU_SM_GOJOBORI && method != HU_SM_GOLDMAN)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	const int32_t n = n_nodes;
	*n_items = 0;
	if(child_off[0] != 0 || child_off[n] != n - 1) { hu_set_error("%s: the child lists name %d children, the tree has %d", fn, child_off[n] - child_off[0], n - 1); return HU_ERR_ARG; }
	for(int32_t u = 0; u < n; ++u) {
		if(child_off[u + 1] < child_off[u] || parent[u] >= n) { hu_set_error("%s: node %d: bad child list or parent", fn, u); return HU_ERR_ARG; }
		for(int32_t c = child_off[u]; c < child_off[u + 1]; ++c) if(child_idx[c] < 0 || child_idx[c] >= n || parent[child_idx[c]] != u) { hu_set_error("%s: child list entry %d is not a child of node %d", fn, c, u); return HU_ERR_ARG; }
	}
	/* PTUNode's predicates (src/PhyloTreeUnrooted.h:199-267) on the neighbour list "parent, then children in file order" */
	auto nChild = [&](int32_t u) { return child_off[u + 1] - child_off[u]; };
	auto nNeighbour = [&](int32_t u) { return nChild(u) + (parent[u] >= 0 ? 1 : 0); };
	auto isLeaf = [&](int32_t u) { return nNeighbour(u) == 1; };
	auto isTip = [&](int32_t u) {
		if(isLeaf(u)) return false;
		for(int32_t c = child_off[u]; c < child_off[u + 1]; ++c) if(!isLeaf(child_idx[c])) return false;
		return true;
	};
	auto first = [&](int32_t u) { return child_idx[child_off[u]]; };
	auto last = [&](int32_t u) { return child_idx[child_off[u + 1] - 1]; };
	int64_t k = 0;
	auto put = [&](int32_t node0, int32_t node1, int32_t node2) -> bool {
		const int32_t r0 = node0 < 0 ? -1 : row_of[node0], r1 = row_of[node1], r2 = row_of[node2];
		if((node0 >= 0 && r0 < 0) || r1 < 0 || r2 < 0) { hu_set_error("%s: a leaf among nodes %d, %d, %d has no MSA row", fn, node0, node1, node2); return false; }
		items[3 * k] = r0; items[3 * k + 1] = r1; items[3 * k + 2] = r2; ++k;
		return true;
	};
	for(int32_t u = 0; u < n; ++u) {
		if(method == HU_SM_GOJOBORI) { /* :464-486 */
			if(nChild(u) != 2) continue;
			int32_t tip = first(u), outer = last(u);
			if(!isTip(tip) && !isTip(outer)) continue;
			if(!isTip(tip)) std::swap(tip, outer);
			/* randomLeaf (src/PhyloTreeUnrooted.h:1480-1486): the C library's rand(), never seeded here, drawn whether or not the item is used later */
			int32_t node = outer;
			while(!isLeaf(node)) node = child_idx[child_off[node] + rand() % nChild(node)];
			if(!put(node, first(tip), last(tip))) return HU_ERR_ARG;
		}
		else { /* :449-462: a tip with more than two neighbours; the distance tested is that of the first child's row with ITSELF, as the reference has it */
			if(!isTip(u) || nNeighbour(u) <= 2) continue;
			if(!put(-1, first(u), last(u))) return HU_ERR_ARG;
		}
	}
	*n_items = k;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_sm_training_set"); }

/* SeqUtils::pDist(...) <= MAX_PDIST on the integers hu_sm_counts returns: (double) d / N, NaN (N == 0) fails */
extern "C" int hu_sm_item_pass(int64_t n_items, const int32_t* items, const int32_t* dn, int32_t* pass) {
	if(n_items < 0 || (n_items > 0 && (!items || !dn || !pass))) { hu_set_error("hu_sm_item_pass: bad argument"); return HU_ERR_ARG; }
	for(int64_t i = 0; i < n_items; ++i) {
		const double p1 = static_cast<double>(dn[4 * i]) / dn[4 * i + 1], p2 = static_cast<double>(dn[4 * i + 2]) / dn[4 * i + 3];
		pass[i] = items[3 * i] < 0 ? p1 <= SM_MAX_PDIST : (p1 <= SM_MAX_PDIST && p2 <= SM_MAX_PDIST);
	}
	return HU_OK;
}

extern "C" int hu_sm_train(int type, int64_t n_items, const double* mats, const int32_t* pass, const int64_t* base, hu_model_desc* out, int64_t* n_used) try {
	const char* fn = "hu_sm_train";
	if(type < HU_GTR || type > HU_JC69 || n_items < 0 || (n_items > 0 && (!mats || !pass)) || !base || !out) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	static const char* names[] = {"GTR", "TN93", "HKY85", "F81", "K80", "JC69"};
	enum { A = 0, C = 1, G = 2, T = 3 };
	hu_model_desc m;
	memset(&m, 0, sizeof(m));
	m.type = type;
	for(int i = 0; i < 4; ++i) m.pi[i] = 0.25;
	int64_t used = 0, handed = 0;
	for(int64_t i = 0; i < n_items; ++i) handed += pass[i] != 0;
	if(type <= HU_F81) { /* pi = f / f.sum() */
		if(base[0] < 0 || base[1] < 0 || base[2] < 0 || base[3] < 0) { hu_set_error("%s: negative base count", fn); return HU_ERR_ARG; }
		const double f[4] = {(double) base[0], (double) base[1], (double) base[2], (double) base[3]};
		const double s = ((f[0] + f[1]) + f[2]) + f[3];
		if(s == 0) { hu_set_error("%s: the leaf rows hold no residue: pi of a %s model would be NaN (the reference prints it)", fn, names[type]); return HU_ERR_ARG; }
		for(int i = 0; i < 4; ++i) m.pi[i] = f[i] / s;
	}
	const double* pi = m.pi;
	if(type == HU_GTR) {
		double Q[16] = {0};
		for(int64_t it = 0; it < n_items; ++it) if(pass[it]) {
			const double* P0 = mats + 16 * it;
			/* constrainedQfromP (src/DNASubModel.cpp:147-164) */
			double P[16], Z[4], Qv[16] = {0};
			for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) P[4 * i + j] = (P0[4 * i + j] + P0[4 * j + i]) / 2.0;
			for(int i = 0; i < 4; ++i) Z[i] = ((P[4 * i] + P[4 * i + 1]) + P[4 * i + 2]) + P[4 * i + 3];
			for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) if(i != j) { Qv[4 * i + j] = P[4 * i + j] / Z[i]; Qv[5 * i] -= Qv[4 * i + j]; }
			/* isValidRate (src/DNASubModel.h:200-206): not all zero, every off-diagonal >= 0 (a NaN fails) */
			bool allZero = true, ok = true;
			for(int i = 0; i < 16; ++i) if(!(Qv[i] == 0)) allZero = false;
			for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) if(i != j && !(Qv[4 * i + j] >= 0)) ok = false;
			if(allZero || !ok) continue;
			++used;
			/* scale(Qv) with its default pi = Ones: by minus the TRACE (src/DNASubModel.cpp:123-126) */
			const double beta = ((Qv[0] + Qv[5]) + Qv[10]) + Qv[15];
			for(int i = 0; i < 16; ++i) Q[i] += Qv[i] / -beta * 1.0;
		}
		if(used == 0) { hu_set_error("%s: none of the %lld matrices handed in gives a valid rate matrix: the GTR average would be NaN (the reference prints it)", fn, (long long) handed); return HU_ERR_ARG; }
		for(int i = 0; i < 16; ++i) Q[i] /= (double) used;
		double R[16];
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) R[4 * i + j] = i == j ? 0.0 : Q[4 * i + j] / pi[j];
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) m.par[4 * i + j] = (R[4 * i + j] + R[4 * j + i]) / 2.0;
	}
	else if(type == HU_TN93 || type == HU_HKY85 || type == HU_K80) {
		double Tr = 0, Ty = 0, Ti = 0, Tv = 0;
		for(int64_t it = 0; it < n_items; ++it) if(pass[it]) {
			const double* P = mats + 16 * it;
			++used;
			Tr += P[4 * A + G] + P[4 * G + A];
			Ty += P[4 * C + T] + P[4 * T + C];
			Ti += P[4 * A + G] + P[4 * G + A] + P[4 * C + T] + P[4 * T + C];
			Tv += P[4 * A + C] + P[4 * A + T] + P[4 * C + A] + P[4 * C + G] + P[4 * G + C] + P[4 * G + T] + P[4 * T + A] + P[4 * T + G];
		}
		if(Tv == 0) { hu_set_error("%s: Tv == 0: the %lld matrices handed in hold no transversion, so the rate ratios of %s would be NaN or infinite (the reference prints them)", fn, (long long) handed, names[type]); return HU_ERR_ARG; }
		if(type == HU_TN93) { /* setBeta: src/TN93.h:100-103 */
			const double kr = Tr / Tv, ky = Ty / Tv;
			m.par[0] = kr; m.par[1] = ky;
			m.par[2] = 1 / (2 * (pi[A] * pi[C] + pi[A] * pi[T] + pi[C] * pi[G] + pi[G] * pi[T] + kr * (pi[A] * pi[G]) + ky * (pi[C] * pi[T])));
		}
		else if(type == HU_HKY85) { /* src/HKY85.h:100-102 */
			const double kappa = Ti / Tv;
			m.par[0] = kappa;
			m.par[1] = 1 / (2 * (pi[A] + pi[G]) * (pi[C] + pi[T]) + 2 * kappa * (pi[A] * pi[G] + pi[C] * pi[T]));
		}
		else m.par[0] = Ti / Tv;
	}
	else if(type == HU_F81) { used = handed; m.par[0] = 1 / (1 - (((pi[0] * pi[0] + pi[1] * pi[1]) + pi[2] * pi[2]) + pi[3] * pi[3])); }
	else used = handed;     /* JC69 has nothing to train */
	*out = m;
	if(n_used) *n_used = used;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_sm_train"); }

/* DNASubModel::write (src/GTR.cpp:83-90, src/TN93.cpp:79-86, ...) in the layout of the .ptu's generated model block: one blank between
 * numbers, every number as %.17g.  GTR's Q: lines ("for human read only", skipped by both readers) are GTR::setQfromParams' matrix,
 * scaled by minus its trace as the reference computes it. */
extern "C" int64_t hu_sm_write_text(const hu_model_desc* model, char* buf, int64_t cap) try {
	if(!model || model->type < HU_GTR || model->type > HU_JC69 || cap < 0 || (cap > 0 && !buf)) { hu_set_error("hu_sm_write_text: bad argument"); return HU_ERR_ARG; }
	static const char* names[] = {"GTR", "TN93", "HKY85", "F81", "K80", "JC69"};
	const hu_model_desc& m = *model;
	char t[64];
	auto num = [&](double v) { snprintf(t, sizeof(t), "%.17g", v); return std::string(t); };
	auto row = [&](const double* v) { return num(v[0]) + " " + num(v[1]) + " " + num(v[2]) + " " + num(v[3]) + "\n"; };
	std::string o = std::string("# DNA Substitution Model\nType: ") + names[m.type] + "\n";
	if(m.type <= HU_F81) o += "pi: " + row(m.pi);
	if(m.type == HU_GTR) {
		o += "R:\n";
		for(int i = 0; i < 4; ++i) o += row(m.par + 4 * i);
		double Q[16], tr = 0;
		for(int i = 0; i < 4; ++i) {
			double rs = 0;
			for(int j = 0; j < 4; ++j) { Q[4 * i + j] = i == j ? 0 : m.par[4 * i + j] * m.pi[j]; rs += Q[4 * i + j]; }
			Q[5 * i] = -rs; tr += Q[5 * i];
		}
		for(int i = 0; i < 16; ++i) Q[i] = Q[i] / -tr * 1.0;
		o += "Q:\n";
		for(int i = 0; i < 4; ++i) o += row(Q + 4 * i);
	}
	else if(m.type == HU_TN93) o += "kr: " + num(m.par[0]) + " ky: " + num(m.par[1]) + " beta: " + num(m.par[2]) + "\n";
	else if(m.type == HU_HKY85) o += "kappa: " + num(m.par[0]) + " beta: " + num(m.par[1]) + "\n";
	else if(m.type == HU_F81) o += "beta: " + num(m.par[0]) + "\n";
	else if(m.type == HU_K80) o += "kappa: " + num(m.par[0]) + "\n";
	if(cap > 0) { const size_t k = std::min<size_t>(o.size(), (size_t) cap - 1); memcpy(buf, o.data(), k); buf[k] = 0; }
	return (int64_t) o.size();
} catch(...) { return hu_catch_all("hu_sm_write_text"); }
