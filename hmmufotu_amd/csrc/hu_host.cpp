// Host-side preparation: substitution-model spectral forms, profile post-load chain,
// readers of the reference's on-disk formats.  No device code in this file.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <strings.h>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <sstream>
#include <memory>
#include <algorithm>
#include <new>
#include <stdexcept>
#include <sched.h>
#include <atomic>
#include <thread>
#include "hu_common.h"
#include "hu_gamma_fn.h"

static thread_local char g_err[512] = "";

void hu_set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
}
extern "C" const char* hu_last_error(void) { return g_err; }

/* ---- CPU budget (hu_common.h) */
static int cpu_budget_compute() {
	if(const char* e = getenv("HU_CPU_BUDGET")) { const int v = atoi(e); if(v >= 1) return v; }
	long best = (long) std::thread::hardware_concurrency();
	if(best < 1) best = 1;
	{ cpu_set_t set; CPU_ZERO(&set); if(sched_getaffinity(0, sizeof(set), &set) == 0) { const long c = CPU_COUNT(&set); if(c >= 1 && c < best) best = c; } }
	{ /* cgroup v2: "<quota> <period>" or "max <period>" */
		FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r");
		if(f) { char q[64]; long per = 0; if(fscanf(f, "%63s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) { const long c = (atol(q) + per - 1) / per; if(c >= 1 && c < best) best = c; } fclose(f); }
	}
	{ /* cgroup v1 */
		FILE* fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"); FILE* fp = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
		long q = -1, per = 0;
		if(fq && fp && fscanf(fq, "%ld", &q) == 1 && fscanf(fp, "%ld", &per) == 1 && q > 0 && per > 0) { const long c = (q + per - 1) / per; if(c >= 1 && c < best) best = c; }
		if(fq) fclose(fq);
		if(fp) fclose(fp);
	}
	/* one process per GPU under a launcher (torch.distributed.run sets LOCAL_WORLD_SIZE): the ranks of a node share its CPUs */
	if(const char* e = getenv("LOCAL_WORLD_SIZE")) { const int w = atoi(e); if(w > 1) best = std::max<long>(1, best / w); }
	return (int) best;
}
int hu_cpu_budget() { static const int b = cpu_budget_compute(); return b; }
/* helpers of ALL pools together: the budget less one, because every caller of a pool works itself (the other callers — one thread per batch in
 * flight — sleep on their stream while a batch's host stage runs: hipDeviceScheduleBlockingSync, hu_engine.hip) */
static std::atomic<int>& helper_tokens() { static std::atomic<int> t{std::max(0, hu_cpu_budget() - 1)}; return t; }
int hu_helpers_acquire(int want) {
	if(want <= 0) return 0;
	std::atomic<int>& t = helper_tokens();
	int have = t.load();
	for(;;) {
		const int take = std::min(want, std::max(have, 0));
		if(take == 0) return 0;
		if(t.compare_exchange_weak(have, have - take)) return take;
	}
}
void hu_helpers_release(int n) { if(n > 0) helper_tokens().fetch_add(n); }

int hu_catch_all(const char* fn) noexcept {
	try { throw; }
	catch(const std::bad_alloc&) { hu_set_error("%s: out of host memory (std::bad_alloc)", fn); return HU_ERR_NOMEM; }
	catch(const std::length_error& e) { hu_set_error("%s: a size the host cannot hold (%s)", fn, e.what()); return HU_ERR_NOMEM; }
	catch(const std::exception& e) { hu_set_error("%s: %s", fn, e.what()); return HU_ERR_STATE; }
	catch(...) { hu_set_error("%s: unknown exception", fn); return HU_ERR_STATE; }
}

/* ------------------------------------------------------------------------------------------------
 * The first k places of std::sort, for HU_SEED_ORDER_LIBSTDCXX.
 *
 * The reference keeps the first maxNSeed elements of std::sort(locs.begin(), locs.end()) with operator< on dist alone
 * (src/HmmUFOtu_main.cpp:139, src/hmmufotu.cpp:646-647; operator< src/PhyloTreeUnrooted.h:1623-1625): which of the nodes tying at the
 * cut-off distance are kept, and the order of equal distances inside the list, is the permutation libstdc++'s introsort leaves — a
 * deterministic function of the sequence of comparison results, hence of the keys in node order.  Restated here from the published
 * algorithm of libstdc++'s <bits/stl_algo.h> (std::__sort, GCC 4.9 - 13; the reference's distribution builds with the system's g++):
 *   introsort loop on [first, last) while it holds more than 16 elements: depth limit 2 floor(lg n), decremented per partition — at 0 the
 *   range is heap-sorted (make_heap + sort_heap); pivot = median of first + 1, first + (last - first) / 2, last - 1 swapped into *first;
 *   unguarded Hoare partition of [first + 1, last) against *first (both scans stop on elements EQUAL to the pivot, which are swapped);
 *   recursion into [cut, last), loop on [first, cut); then ONE insertion sort over everything (strict comparisons: stable on what the
 *   partitions left).
 * Only what can reach the first k places is executed: a range that starts at or beyond place k is never partitioned (its elements are
 * >= everything left of it and the strict insertion sort cannot carry them across its start), so the cost is ~2n element visits
 * instead of n lg n.  tests/test_seed_order.py checks it against the literal std::sort of the oracle on tie-heavy inputs of every size.
 * Elements are (key << 24 | index) with key an order-isomorphic integer image of dist; comparisons look at the key alone. */
namespace {
struct PrefixSort {
	uint64_t* a; size_t k;
	static bool less(uint64_t x, uint64_t y) { return (x >> 24) < (y >> 24); }
	void median_to_first(uint64_t* result, uint64_t* x, uint64_t* y, uint64_t* z) {
		if(less(*x, *y)) { if(less(*y, *z)) std::swap(*result, *y); else if(less(*x, *z)) std::swap(*result, *z); else std::swap(*result, *x); }
		else if(less(*x, *z)) std::swap(*result, *x);
		else if(less(*y, *z)) std::swap(*result, *z);
		else std::swap(*result, *y);
	}
	uint64_t* partition(uint64_t* first, uint64_t* last, const uint64_t* pivot) {
		for(;;) {
			while(less(*first, *pivot)) ++first;
			--last;
			while(less(*pivot, *last)) --last;
			if(!(first < last)) return first;
			std::swap(*first, *last);
			++first;
		}
	}
	void loop(uint64_t* first, uint64_t* last, long depth) {
		while(last - first > 16) {
			if(depth == 0) { std::make_heap(first, last, less); std::sort_heap(first, last, less); return; }    /* __partial_sort(first, last, last) */
			--depth;
			uint64_t* mid = first + (last - first) / 2;
			median_to_first(first, first + 1, mid, last - 1);
			uint64_t* cut = partition(first + 1, last, first);
			if(cut < a + k) loop(cut, last, depth);       /* a range beyond the first k places cannot change them */
			last = cut;
		}
	}
	void run(size_t n) {
		if(n == 0) return;
		long lg = 0; for(size_t m = n; m > 1; m >>= 1) ++lg;
		loop(a, a + n, 2 * lg);
		/* __final_insertion_sort over the part whose blocks are final: everything up to the end of the block that holds place k - 1.
		 * The first unpartitioned range starts at or beyond k; blocks of <= 16 elements lie before it.  Sorting a few elements more
		 * than needed is harmless, fewer would not be: take [0, min(n, k + 16)) — a block reaching across k ends within 16 of it...
		 * unless it is a heap-sorted or skipped range, whose elements an insertion sort leaves where they are relative to [0, k). */
		const size_t e = std::min(n, k + 16);
		for(size_t i = 1; i < e; ++i) {
			const uint64_t v = a[i]; size_t j = i;
			while(j > 0 && less(v, a[j - 1])) { a[j] = a[j - 1]; --j; }
			a[j] = v;
		}
	}
};
}
/* a [n] packed (key << 24 | index); on return a[0 .. min(k, n)) are the first places of std::sort on the keys */
void hu_sort_prefix_packed(uint64_t* a, size_t n, size_t k) { PrefixSort s{a, k}; s.run(n); }

extern "C" int hu_sort_prefix_libstdcxx(const double* dist, int64_t n, int64_t k, int32_t* out_idx) try {
	if(n < 0 || k < 0 || (n > 0 && (!dist || !out_idx)) || n >= (1ll << 24)) { hu_set_error("hu_sort_prefix_libstdcxx: bad argument"); return HU_ERR_ARG; }
	/* order-isomorphic integer keys: the rank of each distinct value (40 bits are plenty for < 2^24 elements) */
	std::vector<double> vals(dist, dist + n);
	for(int64_t i = 0; i < n; ++i) if(std::isnan(vals[i])) { hu_set_error("hu_sort_prefix_libstdcxx: NaN distance (std::sort is undefined on it)"); return HU_ERR_ARG; }
	std::sort(vals.begin(), vals.end());
	vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
	std::vector<uint64_t> a((size_t) n);
	for(int64_t i = 0; i < n; ++i) a[i] = ((uint64_t)(std::lower_bound(vals.begin(), vals.end(), dist[i]) - vals.begin()) << 24) | (uint64_t) i;
	hu_sort_prefix_packed(a.data(), (size_t) n, (size_t) k);
	for(int64_t i = 0; i < std::min(n, k); ++i) out_idx[i] = (int32_t)(a[i] & 0xffffffu);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_sort_prefix_libstdcxx"); }

extern "C" void hu_default_opts(hu_opts* o) {
	o->align_mode = HU_MODE_GLOBAL;
	o->max_nseed = 50;
	o->max_diff = std::numeric_limits<double>::infinity();
	o->max_height = std::numeric_limits<double>::infinity();
	o->max_error = 20;
	o->weighted = 0;
	o->only_ml = 0;
	o->prior = HU_PRIOR_UNIFORM;
	o->fix_root_loglik = 0;
	o->seed_order = HU_SEED_ORDER_LIBSTDCXX;      /* the reference's own std::sort order (src/HmmUFOtu_main.cpp:139) */
	o->ignore_orient = 0;
}

/* ------------------------------------------------------------------ substitution models */
static void sym_eig4(double A[16], double V[16], double w[4]) {
	for(int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
	for(int sweep = 0; sweep < 64; ++sweep) {
		double off = 0;
		for(int p = 0; p < 4; ++p) for(int q = p + 1; q < 4; ++q) off += A[p*4+q] * A[p*4+q];
		if(off < 1e-300) break;
		for(int p = 0; p < 4; ++p) for(int q = p + 1; q < 4; ++q) {
			double apq = A[p*4+q];
			if(apq == 0) continue;
			double theta = (A[q*4+q] - A[p*4+p]) / (2 * apq);
			double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
			double c = 1 / std::sqrt(t * t + 1), s = t * c;
			for(int k = 0; k < 4; ++k) { double a = A[k*4+p], b = A[k*4+q]; A[k*4+p] = c * a - s * b; A[k*4+q] = s * a + c * b; }
			for(int k = 0; k < 4; ++k) { double a = A[p*4+k], b = A[q*4+k]; A[p*4+k] = c * a - s * b; A[q*4+k] = s * a + c * b; }
			for(int k = 0; k < 4; ++k) { double a = V[k*4+p], b = V[k*4+q]; V[k*4+p] = c * a - s * b; V[k*4+q] = s * a + c * b; }
		}
	}
	for(int i = 0; i < 4; ++i) w[i] = A[i*4+i];
}

/* Rate matrix of each model type as implied by the reference's Pr(t):
 *   GTR   Q = R*diag(pi), diagonal = -rowsum, divided by -trace(Q)   (src/GTR.cpp:124-131; note
 *         DNASubModel::scale is called with its default pi = Ones(), src/DNASubModel.h:154)
 *   TN93  Q(i,j) = beta pi(j) k(i,j), k = kr for A<->G, ky for C<->T, 1 otherwise (src/TN93.h:113-154)
 *   HKY85 kr = ky = kappa (src/HKY85.h:111-153); F81 k = 1 (src/F81.h:110-118)
 *   K80   pi = 1/4, transitions kappa*beta, transversions beta, beta = 1/(2 kappa) (src/K80.h:98-118)
 *   JC69  pi = 1/4, every rate 1/3 (src/JC69.h:97-101) */
int hu_model_prepare(const hu_model_desc* d, HuModelDev* out) {
	memset(out, 0, sizeof(*out));
	out->type = d->type;
	double pi[4], Q[16];
	for(int i = 0; i < 4; ++i) pi[i] = (d->type == HU_K80 || d->type == HU_JC69) ? 0.25 : d->pi[i];
	for(int i = 0; i < 4; ++i) if(!(pi[i] > 0)) { hu_set_error("model: base frequency %d is not positive", i); return HU_ERR_ARG; }
	auto ti = [](int i, int j) { return (i ^ j) == 2; }; /* A(0)<->G(2), C(1)<->T(3) */
	switch(d->type) {
	case HU_GTR: {
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) Q[i*4+j] = i == j ? 0.0 : d->par[i*4+j] * pi[j];
		double tr = 0;
		for(int i = 0; i < 4; ++i) { double s = 0; for(int j = 0; j < 4; ++j) if(j != i) s += Q[i*4+j]; Q[i*4+i] = -s; tr += -s; }
		for(int i = 0; i < 16; ++i) Q[i] = Q[i] / -tr;
		break;
	}
	case HU_TN93: case HU_HKY85: case HU_F81: {
		double kr = 1, ky = 1, beta;
		if(d->type == HU_TN93) { kr = d->par[0]; ky = d->par[1]; beta = d->par[2]; }
		else if(d->type == HU_HKY85) { kr = ky = d->par[0]; beta = d->par[1]; }
		else beta = d->par[0];
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j)
			Q[i*4+j] = i == j ? 0.0 : beta * pi[j] * (ti(i, j) ? ((i == 0 || i == 2) ? kr : ky) : 1.0);
		break;
	}
	case HU_K80: {
		double kappa = d->par[0], beta = 1 / (2 * kappa);
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) Q[i*4+j] = i == j ? 0.0 : (ti(i, j) ? kappa * beta : beta);
		break;
	}
	case HU_JC69:
		for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) Q[i*4+j] = i == j ? 0.0 : 1.0 / 3;
		break;
	default:
		hu_set_error("model: unknown type %d", d->type);
		return HU_ERR_ARG;
	}
	if(d->type != HU_GTR)
		for(int i = 0; i < 4; ++i) { double s = 0; for(int j = 0; j < 4; ++j) if(j != i) s += Q[i*4+j]; Q[i*4+i] = -s; }
	double S[16], V[16], sq[4], isq[4];
	for(int i = 0; i < 4; ++i) { sq[i] = std::sqrt(pi[i]); isq[i] = 1 / sq[i]; }
	for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) S[i*4+j] = sq[i] * Q[i*4+j] * isq[j];
	for(int i = 0; i < 4; ++i) for(int j = i + 1; j < 4; ++j) { double a = 0.5 * (S[i*4+j] + S[j*4+i]); S[i*4+j] = S[j*4+i] = a; }
	sym_eig4(S, V, out->lam);
	/* the zero eigenvalue and its eigenvector sqrt(pi) are exact in theory: moved to index 0 and snapped, so that
	 * P(t) rows keep summing to 1 for huge t, U(i,0) = 1, U1(0,i) = pi(i): component 0 of a message in the
	 * eigenbasis is pi . e (k_place_blk normalises messages by it and keeps the other three components) */
	int z = 0;
	for(int k = 1; k < 4; ++k) if(std::fabs(out->lam[k]) < std::fabs(out->lam[z])) z = k;
	if(z != 0) { std::swap(out->lam[0], out->lam[z]); for(int i = 0; i < 4; ++i) std::swap(V[i*4+0], V[i*4+z]); }
	out->lam[0] = 0.0;
	for(int i = 0; i < 4; ++i) V[i*4+0] = sq[i];
	for(int i = 0; i < 4; ++i) for(int k = 0; k < 4; ++k) { out->U[i*4+k] = isq[i] * V[i*4+k]; out->U1[k*4+i] = V[i*4+k] * sq[i]; }
	for(int i = 0; i < 4; ++i) { out->U[i*4+0] = 1.0; out->U1[0*4+i] = pi[i]; }
	for(int i = 0; i < 4; ++i) { out->pi[i] = pi[i]; out->logpi[i] = std::log(pi[i]); }
	out->dgK = d->dg_k;
	if(d->dg_k < 0 || d->dg_k > HU_MAX_DGK) { hu_set_error("model: dg_k %d out of range", d->dg_k); return HU_ERR_ARG; }
	out->rate[0] = 1.0;
	for(int k = 0; k < d->dg_k; ++k) out->rate[k] = d->dg_rate[k];
	return HU_OK;
}

/* constants of k_place_blk: with messages in the eigenbasis (a = U^-1 e) every per-site quantity of the joint
 * branch-length optimisation is a bilinear form a_U^T M a_V; the model-dependent factors of those 4x4 tables: */
void hu_place_consts(const HuModelDev& m, double* pc) {
	for(int i = 0; i < 4; ++i) pc[HU_PC_LAM + i] = m.lam[i];
	for(int i = 0; i < HU_MAX_DGK; ++i) pc[HU_PC_RATE + i] = m.rate[i];
	double pi2 = 0;
	for(int i = 0; i < 4; ++i) pi2 += m.pi[i] * m.pi[i];
	for(int a = 0; a < 4; ++a) for(int c = 0; c < 4; ++c) {
		for(int b = 0; b < 4; ++b) pc[HU_PC_W + b * 16 + a * 4 + c] = m.U[b*4+a] * m.U[b*4+c];
		double g = 0;
		for(int i = 0; i < 4; ++i) g += m.pi[i] * m.pi[i] * m.U[i*4+a] * m.U[i*4+c];
		pc[HU_PC_W + 4 * 16 + a * 4 + c] = g / pi2;
		for(int k = 0; k < 4; ++k) {
			double t = 0;
			for(int i = 0; i < 4; ++i) t += m.pi[i] * m.U[i*4+a] * m.U[i*4+c] * m.U[i*4+k];
			pc[HU_PC_C + (a * 4 + c) * 4 + k] = t;
		}
	}
	for(int k = 0; k < 4; ++k) {
		for(int b = 0; b < 4; ++b) pc[HU_PC_CB + b * 4 + k] = m.U1[k*4+b];
		double a = 0, s = 0;
		for(int i = 0; i < 4; ++i) { a += m.U1[k*4+i] * m.pi[i]; s += m.pi[i] * m.U[i*4+k]; }
		pc[HU_PC_CB + 4 * 4 + k] = a;
		pc[HU_PC_S + k] = s;
	}
}

/* host-only export for CPU tests of the spectral forms */
extern "C" int hu_model_spectral(const hu_model_desc* d, double* U, double* lam, double* U1) try {
	HuModelDev m;
	int rc = hu_model_prepare(d, &m);
	if(rc != HU_OK) return rc;
	memcpy(U, m.U, sizeof(m.U)); memcpy(lam, m.lam, sizeof(m.lam)); memcpy(U1, m.U1, sizeof(m.U1));
	return HU_OK;
} catch(...) { return hu_catch_all("hu_model_spectral"); }

/* ------------------------------------------------------------------ profile (BandedHMMP7) */
/* post-load chain of operator>> (src/BandedHMMP7.cpp:104-109): extend_index,
 * adjustProfileLocalMode (:721-733), wingRetract (:1083-1120) */
int HuProfileHost::init(const hu_profile_desc* d) {
	if(d->K < 1 || d->L < d->K || d->L > 65535) { hu_set_error("profile: bad sizes K=%d L=%d", d->K, d->L); return HU_ERR_ARG; }
	K = d->K; L = d->L;
	EM.assign(d->EM, d->EM + 4 * (K + 1));
	EI.assign(d->EI, d->EI + 4 * (K + 1));
	T7.assign(d->T, d->T + 7 * (K + 1));
	p2cs.assign(d->p2cs, d->p2cs + K + 1);
	p2cs[0] = 0;
	for(int k = 1; k <= K; ++k)
		if(p2cs[k] < 1 || p2cs[k] > L || (k > 1 && p2cs[k] <= p2cs[k - 1])) { hu_set_error("profile: MAP of column %d invalid", k); return HU_ERR_ARG; }
	cs2p.assign(L + 2, 0);
	for(int k = 1; k <= K; ++k) cs2p[p2cs[k]] = k;
	for(int i = p2cs[K] + 1; i <= L; ++i) cs2p[i] = K;
	const double* Tc = T7.data();
	std::vector<double> entry(K + 1, 0.0), exitp(K + 1, 0.0);
	double t0 = std::exp(-Tc[0]), tK = std::exp(-Tc[(size_t) K * 7]);
	for(int k = 1; k <= K; ++k) { entry[k] = t0; exitp[k] = tK; }
	{ /* B->D1->...->Dj-1->Mj folded into B->Mj; the partial sums are shared between consecutive j */
		double chain = Tc[2]; /* Tmat_cost[0](M,D) */
		for(int j = 2; j <= K; ++j) {
			if(j > 2) chain += Tc[(size_t)(j - 2) * 7 + 6];
			double cost = chain + Tc[(size_t)(j - 1) * 7 + 5];
			entry[j] += std::exp(-cost);
			if(entry[j] > 1) entry[j] = 1;
		}
	}
	for(int i = 1; i <= K - 1; ++i) { /* Mi->Di+1->...->DK->E folded into Mi->E */
		double cost = Tc[(size_t) i * 7 + 2];
		for(int j = i + 1; j < K; ++j) cost += Tc[(size_t) j * 7 + 6];
		cost += Tc[(size_t) K * 7 + 5];
		exitp[i] += std::exp(-cost);
		if(exitp[i] > 1) exitp[i] = 1;
	}
	entryC.resize(K + 1); exitC.resize(K + 1);
	for(int k = 0; k <= K; ++k) { entryC[k] = -std::log(entry[k]); exitC[k] = -std::log(exitp[k]); }
	return HU_OK;
}

/* setSequenceMode (src/BandedHMMP7.cpp:561-583) with p1 of src/BandedHMMP7Bg.cpp:33-35 */
void hu_mode_costs(int K, int mode, double* tNN, double* tNB, double* tEC, double* tCC) {
	double p1 = K >= 350 ? K / (K + 1.0) : 350 / (350 + 1.0);
	double term = 1 - p1, nn = 0, cc = 0;
	switch(mode) {
	case HU_MODE_LOCAL: nn = cc = term; break;
	case HU_MODE_NGCL: cc = term; break;
	case HU_MODE_CGNL: nn = term; break;
	default: break;
	}
	*tNN = -std::log(nn); *tNB = -std::log(1.0 - nn); *tEC = -std::log(1.0); *tCC = -std::log(cc);
}

/* ------------------------------------------------------------------ .hmm reader */
static double hmm_value(const std::string& s) { return s != "*" ? atof(s.c_str()) : std::numeric_limits<double>::infinity(); }

/* HMMER3/f-style text as BandedHMMP7's operator>> accepts it (src/BandedHMMP7.cpp:100-246) */
int hu_read_hmm(const char* path, HuProfileHost& prof, std::vector<double>& EM, std::vector<double>& EI,
		std::vector<double>& T, std::vector<int32_t>& p2cs, int& K, int& L) {
	std::ifstream in(path);
	if(!in) { hu_set_error("cannot open HMM file '%s'", path); return HU_ERR_IO; }
	return hu_read_hmm_stream(in, path, prof, EM, EI, T, p2cs, K, L);
}
int hu_read_hmm_stream(std::istream& in, const char* path, HuProfileHost& prof, std::vector<double>& EM, std::vector<double>& EI,
		std::vector<double>& T, std::vector<int32_t>& p2cs, int& K, int& L) {
	std::string line;
	K = 0; L = 0;
	int k = 0;
	bool mapYes = false, done = false;
	std::map<std::string, std::string> tags;
	while(std::getline(in, line)) {
		if(line == "//") { done = true; break; }
		if(line.empty()) continue;
		std::istringstream iss(line);
		std::string tag;
		if(!isspace((unsigned char) line[0])) {
			iss >> tag;
			if(tag.substr(0, 6) == "HMMER3") {
				if(tag.length() < 8 || tag[7] < 'f') { hu_set_error("obsolete HMM file version %s", tag.c_str()); return HU_ERR_IO; }
			}
			else if(tag == "LENG") {
				iss >> K;
				if(K < 1 || K > 65535) { hu_set_error("HMM LENG %d out of range", K); return HU_ERR_IO; }
				EM.assign((size_t) 4 * (K + 1), std::numeric_limits<double>::infinity());
				EI = EM;
				T.assign((size_t) 7 * (K + 1), std::numeric_limits<double>::infinity());
				p2cs.assign(K + 1, 0);
			}
			else if(tag == "ALPH") { std::string a; iss >> a; if(a != "DNA") { hu_set_error("HMM alphabet must be DNA"); return HU_ERR_IO; } }
			else if(tag == "MAXL") iss >> L;
			else if(tag == "HMM") { std::string skip; std::getline(in, skip); }
			else { std::string val; iss >> val; tags[tag] = val; if(tag == "MAP") mapYes = (val == "yes"); }
		}
		else {
			if(K == 0) { hu_set_error("HMM body before LENG"); return HU_ERR_IO; }
			iss >> tag;
			std::string tmp;
			bool compo = tag == "COMPO";
			int idx = 0;
			bool isInt = sscanf(tag.c_str(), "%d", &idx) == 1;
			if(k > K) { hu_set_error("HMM has more than LENG states"); return HU_ERR_IO; }
			if(compo || isInt) {
				if((compo && k != 0) || (!compo && idx != k)) { hu_set_error("HMM state line %s out of order", tag.c_str()); return HU_ERR_IO; }
				for(int i = 0; i < 4; ++i) { iss >> tmp; EM[(size_t) k * 4 + i] = hmm_value(tmp); }
				if(!compo) {
					if(!mapYes) { hu_set_error("HMM file must have the MAP flag set to 'yes'"); return HU_ERR_IO; }
					iss >> tmp; p2cs[k] = atoi(tmp.c_str());
				}
				for(int i = 0; i < 4; ++i) { in >> tmp; EI[(size_t) k * 4 + i] = hmm_value(tmp); }
				for(int i = 0; i < 7; ++i) { in >> tmp; T[(size_t) k * 7 + i] = hmm_value(tmp); }
			}
			else { /* non-COMPO begin-state line: tag is the first insert emission */
				if(k != 0) { hu_set_error("unexpected HMM line"); return HU_ERR_IO; }
				EI[0] = hmm_value(tag);
				for(int i = 1; i < 4; ++i) { iss >> tmp; EI[i] = hmm_value(tmp); }
				for(int i = 0; i < 7; ++i) { in >> tmp; T[i] = hmm_value(tmp); }
			}
			std::getline(in, tmp); /* rest of the transition line */
			k++;
		}
	}
	if(!done || k != K + 1) { hu_set_error("HMM file '%s' truncated (read %d of %d states)", path, k, K + 1); return HU_ERR_IO; }
	if(L == 0) L = p2cs[K];
	hu_profile_desc d{K, L, EM.data(), EI.data(), T.data(), p2cs.data()};
	return prof.init(&d);
}

/* ------------------------------------------------------------------ .ptu reader */
namespace {
struct Rd {
	std::ifstream in;
	bool ok = true;
	uint64_t size = 0;          /* of the file: no length field read from it may ask for more memory than that */
	void measure() { in.seekg(0, std::ios::end); const std::streamoff e = in.tellg(); size = e > 0 ? (uint64_t) e : 0; in.seekg(0, std::ios::beg); }
	template<class X> X get() { X v{}; in.read((char*) &v, sizeof(X)); if(!in) ok = false; return v; }
	std::string str() {
		uint64_t n = get<uint64_t>();
		if(!ok || n > size) { ok = false; return std::string(); }
		std::string s(n, '\0');
		if(n) in.read(&s[0], n);
		if(!in) ok = false;
		return s;
	}
};
}

/* model text block embedded in the .ptu (readers: src/GTR.cpp:43-81, TN93.cpp:40-77,
 * HKY85.cpp:40-75, F81.cpp:40-73, K80.cpp:41-71, JC69.cpp:39-65); consumes exactly the bytes
 * the reference consumes so that the binary dG block that follows stays aligned */
int hu_read_model_text(std::istream& in, hu_model_desc& m) {
	memset(&m, 0, sizeof(m));
	std::string type, tag, line, value;
	in >> type;
	in.ignore();
	static const char* names[] = {"GTR", "TN93", "HKY85", "F81", "K80", "JC69"};
	m.type = -1;
	for(int i = 0; i < 6; ++i) if(type == names[i]) m.type = i;
	if(m.type < 0) { hu_set_error("ptu: unknown model type '%s'", type.c_str()); return HU_ERR_IO; }
	for(int i = 0; i < 4; ++i) m.pi[i] = 0.25;
	while(in >> tag) {
		if(tag[0] == '#') { std::getline(in, line); continue; }
		if(tag == "Type:") {
			in >> value;
			if(value != type) { hu_set_error("ptu: model block type mismatch"); return HU_ERR_IO; }
			if(m.type == HU_JC69) { std::getline(in, line); break; }
		}
		else if(tag == "pi:") { for(int i = 0; i < 4; ++i) in >> m.pi[i]; }
		else if(tag == "R:" && m.type == HU_GTR) { for(int i = 0; i < 16; ++i) in >> m.par[i]; }
		else if(tag == "Q:" && m.type == HU_GTR) { for(int i = 0; i <= 4; ++i) std::getline(in, line); break; }
		else if(tag == "kr:" && m.type == HU_TN93) in >> m.par[0];
		else if(tag == "ky:" && m.type == HU_TN93) in >> m.par[1];
		else if(tag == "kappa:" && m.type == HU_HKY85) in >> m.par[0];
		else if(tag == "kappa:" && m.type == HU_K80) { in >> m.par[0]; std::getline(in, line); break; }
		else if(tag == "beta:" && (m.type == HU_TN93 || m.type == HU_HKY85 || m.type == HU_F81)) {
			in >> m.par[m.type == HU_TN93 ? 2 : m.type == HU_HKY85 ? 1 : 0];
			std::getline(in, line);
			break;
		}
		else { hu_set_error("ptu: unrecognised model tag '%s'", tag.c_str()); return HU_ERR_IO; }
	}
	return in ? HU_OK : HU_ERR_IO;
}

/* PTUnrooted::load (src/PhyloTreeUnrooted.cpp:496-535 and :99-114, :605-621, :632-697,
 * :1068-1083; src/DigitalSeq.cpp:105-121; src/util/ProgEnv.cpp:24-64) */
int hu_read_ptu(const char* path, HuTreeHost& t) { return hu_read_ptu_sink(path, t, nullptr); }

/* sink != NULL: the 4 x csLen messages are handed to it one directed edge at a time (is_down, node, data, root flag) instead of
 * being kept in t.up / t.down: a gg_97-scale file holds 98 GB of them, which hu_db_load sends straight on to the device */
int hu_read_ptu_sink(const char* path, HuTreeHost& t, const std::function<int(bool, int64_t, const double*)>* sink) {
	Rd r;
	r.in.open(path, std::ios::binary);
	if(!r.in) { hu_set_error("cannot open PTU file '%s'", path); return HU_ERR_IO; }
	r.measure();
	char magic[8];
	r.in.read(magic, 8);
	if(!r.in || memcmp(magic, "HmmUFOtu", 8) != 0) { hu_set_error("'%s' is not a HmmUFOtu database file", path); return HU_ERR_IO; }
	for(int i = 0; i < 3; ++i) r.get<int32_t>();
	uint64_t n = r.get<uint64_t>();
	int32_t csLen = r.get<int32_t>();
	if(!r.ok || n == 0 || n > (1u << 24) || csLen < 1 || csLen > 65535) { hu_set_error("ptu: bad header"); return HU_ERR_IO; }
	/* the file carries 2 (n - 1) messages of 4 x csLen doubles: a header that promises more than the file holds is refused before anything is sized by it */
	if((n - 1) * 2 * 32 * (uint64_t) csLen > r.size) { hu_set_error("ptu: the header names %llu nodes x %d columns, the file has %llu bytes", (unsigned long long) n, (int) csLen, (unsigned long long) r.size); return HU_ERR_IO; }
	t.n = (int32_t) n; t.csLen = csLen;
	t.parent.assign(n, -1); t.blen.assign(n, 0.0); t.height.assign(n, 0.0); t.annoDist.assign(n, 0.0);
	t.seq.assign((size_t) n * csLen, (int8_t) -2);
	t.names.resize(n); t.annos.resize(n);
	for(uint64_t i = 0; i < n; ++i) {
		int64_t id = r.get<int64_t>();
		if(!r.ok || id != (int64_t) i) { hu_set_error("ptu: node %llu has id %lld", (unsigned long long) i, (long long) id); return HU_ERR_IO; }
		t.names[i] = r.str();
		bool withAbc = r.get<uint8_t>() != 0;
		if(withAbc) r.str();
		r.str(); /* seq name */
		std::string s = r.str();
		if(!r.ok) break;
		if(!s.empty()) {
			if((int) s.size() != csLen) { hu_set_error("ptu: node %llu sequence length %zu != csLen", (unsigned long long) i, s.size()); return HU_ERR_IO; }
			memcpy(&t.seq[(size_t) i * csLen], s.data(), csLen);
		}
		t.annos[i] = r.str();
		t.annoDist[i] = r.get<double>();
	}
	uint64_t nEdges = r.get<uint64_t>();
	if(!r.ok || nEdges != 2 * (n - 1)) { hu_set_error("ptu: edge count %llu does not match %llu nodes", (unsigned long long) nEdges, (unsigned long long) n); return HU_ERR_IO; }
	std::vector<double> one;
	if(sink) one.resize((size_t) csLen * 4);
	else { t.up.assign((size_t) n * csLen * 4, 0.0); t.down.assign((size_t) n * csLen * 4, 0.0); }
	/* first pass cannot know parents before all isParent flags are seen, so keep the edge list */
	struct Edge { int64_t a, b; bool aParent; double len; std::streampos pos; };
	std::vector<Edge> edges(nEdges);
	for(uint64_t e = 0; e < nEdges; ++e) {
		Edge& E = edges[e];
		E.a = r.get<int64_t>(); E.b = r.get<int64_t>(); E.aParent = r.get<uint8_t>() != 0;
		E.len = r.get<double>();
		uint64_t N = r.get<uint64_t>();
		if(!r.ok || N != (uint64_t) 4 * csLen || E.a < 0 || E.b < 0 || E.a >= (int64_t) n || E.b >= (int64_t) n) { hu_set_error("ptu: bad edge %llu", (unsigned long long) e); return HU_ERR_IO; }
		E.pos = r.in.tellg();
		/* message of a->b: if a is the parent it is down[b], else up[a] */
		double* dst = sink ? one.data() : E.aParent ? &t.down[(size_t) E.b * csLen * 4] : &t.up[(size_t) E.a * csLen * 4];
		r.in.read((char*) dst, sizeof(double) * N);
		if(!r.in) { r.ok = false; break; }
		if(sink) { int rc = (*sink)(E.aParent, E.aParent ? E.b : E.a, dst); if(rc != HU_OK) return rc; }
		if(E.aParent) { t.parent[E.b] = (int32_t) E.a; t.blen[E.b] = E.len; }
	}
	int64_t rootId = r.get<int64_t>();
	if(!r.ok || rootId < 0 || rootId >= (int64_t) n) { hu_set_error("ptu: bad root"); return HU_ERR_IO; }
	t.root = (int32_t) rootId;
	r.in.read((char*) (sink ? one.data() : &t.up[(size_t) rootId * csLen * 4]), sizeof(double) * 4 * csLen);
	if(sink && r.in) { int rc = (*sink)(false, rootId, one.data()); if(rc != HU_OK) return rc; }
	for(uint64_t i = 0; i < n; ++i) {
		int64_t id = r.get<int64_t>(); double h = r.get<double>();
		if(!r.ok || id < 0 || id >= (int64_t) n) { hu_set_error("ptu: bad height record"); return HU_ERR_IO; }
		t.height[id] = h;
	}
	uint32_t nIdx = r.get<uint32_t>();
	for(uint32_t i = 0; i < nIdx && r.ok; ++i) { r.get<uint32_t>(); r.get<int64_t>(); }
	if(!r.ok) { hu_set_error("ptu: truncated file"); return HU_ERR_IO; }
	int rc = hu_read_model_text(r.in, t.model);
	if(rc != HU_OK) return rc;
	bool hasDG = r.get<uint8_t>() != 0;
	if(hasDG) {
		int32_t K = r.get<int32_t>();
		r.get<double>(); /* alpha */
		if(!r.ok || K < 1 || K > HU_MAX_DGK) { hu_set_error("ptu: bad discrete-Gamma block"); return HU_ERR_IO; }
		for(int i = 0; i <= K; ++i) r.get<double>();
		for(int i = 0; i < K; ++i) t.model.dg_rate[i] = r.get<double>();
		t.model.dg_k = K;
	}
	if(!r.ok) { hu_set_error("ptu: truncated file"); return HU_ERR_IO; }
	int roots = 0;
	for(uint64_t i = 0; i < n; ++i) if(t.parent[i] < 0) roots++;
	if(roots != 1 || t.parent[t.root] >= 0) { hu_set_error("ptu: tree is not rooted at a single node"); return HU_ERR_IO; }
	/* annotation classes: equal strings share an id (calcQValues groups by getTaxonName()) */
	std::map<std::string, int32_t> cls;
	t.annoId.resize(n);
	for(uint64_t i = 0; i < n; ++i) {
		auto it = cls.find(t.annos[i]);
		if(it == cls.end()) it = cls.insert({t.annos[i], (int32_t) cls.size()}).first;
		t.annoId[i] = it->second;
	}
	return HU_OK;
}

/* ---- hu_tree_info: the tree of a .ptu without its messages (include/hmmufotu_amd.h) ---- */
struct hu_tree_info { HuTreeHost t; std::vector<std::vector<int32_t>> children; };
extern "C" int hu_tree_info_load(const char* ptu_path, hu_tree_info** out) try {
	if(!ptu_path || !out) { hu_set_error("hu_tree_info_load: null argument"); return HU_ERR_ARG; }
	*out = nullptr;
	std::unique_ptr<hu_tree_info> ti(new hu_tree_info);
	std::vector<int32_t> order;           /* children in the order their parent -> child edges stand in the file */
	const std::function<int(bool, int64_t, const double*)> sink = [&](bool isDown, int64_t node, const double*) -> int { if(isDown) order.push_back((int32_t) node); return HU_OK; };
	int rc = hu_read_ptu_sink(ptu_path, ti->t, &sink);
	if(rc != HU_OK) return rc;
	ti->children.assign((size_t) ti->t.n, std::vector<int32_t>());
	for(int32_t c : order) { const int32_t p = c >= 0 && c < ti->t.n ? ti->t.parent[c] : -1; if(p >= 0 && p < ti->t.n) ti->children[p].push_back(c); }
	*out = ti.release();
	return HU_OK;
} catch(...) { return hu_catch_all("hu_tree_info_load"); }
extern "C" void hu_tree_info_free(hu_tree_info* t) { delete t; }
extern "C" int hu_tree_info_get(const hu_tree_info* t, int32_t* n_nodes, int32_t* cs_len, int32_t* root, hu_model_desc* model) {
	if(!t) return HU_ERR_ARG;
	if(n_nodes) *n_nodes = t->t.n; if(cs_len) *cs_len = t->t.csLen; if(root) *root = t->t.root; if(model) *model = t->t.model;
	return HU_OK;
}
extern "C" int hu_tree_info_node(const hu_tree_info* t, int32_t i, int32_t* parent, double* blen, double* anno_dist, int32_t* is_leaf,
		const char** name, const char** anno) {
	if(!t || i < 0 || i >= t->t.n) return HU_ERR_ARG;
	if(parent) *parent = t->t.parent[i]; if(blen) *blen = t->t.blen[i]; if(anno_dist) *anno_dist = t->t.annoDist[i];
	if(is_leaf) *is_leaf = t->children[i].empty();
	if(name) *name = t->t.names[i].c_str(); if(anno) *anno = t->t.annos[i].c_str();
	return HU_OK;
}
extern "C" int hu_tree_info_children(const hu_tree_info* t, int32_t i, const int32_t** children) {
	if(!t || i < 0 || i >= t->t.n) return 0;
	if(children) *children = t->children[i].data();
	return (int) t->children[i].size();
}

/* ---- discrete Gamma model of the build (src/DiscreteGammaModel.cpp:40-55, 92-98), without Boost ------------------ */
extern "C" int hu_dg_model(int32_t K, double alpha, double* breaks, double* rates) try {
	if(K < 1 || K > HU_MAX_DGK || !(alpha > 0) || std::isinf(alpha) || !breaks || !rates) { hu_set_error("hu_dg_model: bad argument"); return HU_ERR_ARG; }
	/* boost::math::gamma_distribution<double>(alpha, alpha) is (shape, scale): b(i) = alpha * P^-1(alpha, i / K) */
	for(int i = 0; i < K; ++i) breaks[i] = alpha * dg_gamma_quantile(alpha, i / static_cast<double>(K));
	breaks[K] = std::numeric_limits<double>::infinity();
	for(int i = 0; i < K; ++i) {
		const double lbd = breaks[i], ubd = breaks[i + 1];
		rates[i] = !std::isinf(ubd) ? dg_gamma_p(alpha + 1, ubd * alpha) - dg_gamma_p(alpha + 1, lbd * alpha) : 1 - dg_gamma_p(alpha + 1, lbd * alpha);
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dg_model"); }

extern "C" double hu_dg_estimate_shape(int64_t n, const double* X) {
	#pragma clang fp contract(off)
	if(n < 2 || !X) return std::numeric_limits<double>::infinity();
	double s = 0;
	for(int64_t i = 0; i < n; ++i) s += X[i];
	const double m = s / n;
	double q = 0;
	for(int64_t i = 0; i < n; ++i) q += (X[i] - m) * (X[i] - m);
	q /= (n - 1);
	return m * m / (q - m);
}

/* ---- the description of an OTU consensus record (src/hmmufotu-sum.cpp:448-452) ------------------------------------ */
extern "C" int64_t hu_otucs_description(const char* db_name, const char* taxonomy, double anno_dist, int64_t read_count, int64_t sample_hits, char* out, int64_t cap) try {
	if(!db_name || !taxonomy || (cap > 0 && !out)) { hu_set_error("hu_otucs_description: null argument"); return HU_ERR_ARG; }
	/* boost::lexical_cast<std::string>(double) sets the stream's precision to 17 (lcast_precision: 2 + digits * 30103 / 100000) and
	 * writes in the default floating format: printf's %.17g.  Taken from Boost's documented behaviour, not checked against a build. */
	char num[64];
	snprintf(num, sizeof num, "%.17g", anno_dist);
	const std::string d = std::string("DBName=") + db_name + ";Taxonomy=\"" + taxonomy + "\";AnnoDist=" + num + ";ReadCount=" + std::to_string(read_count)
		+ ";SampleHits=" + std::to_string(sample_hits);
	if(cap > 0) { const size_t k = std::min<size_t>(d.size(), (size_t) cap - 1); memcpy(out, d.data(), k); out[k] = 0; }
	return (int64_t) d.size();
} catch(...) { return hu_catch_all("hu_otucs_description"); }

/* ---- Newick reader (src/NewickTree.h:186-215, src/NewickTree.cpp:37-59) and the node numbering of PTUnrooted(const NewickTree&)
 * (src/PhyloTreeUnrooted.cpp:131-182).  Iterative: a ladder-shaped tree of 200,000 leaves nests as deep as it is long. */
struct hu_newick {
	std::vector<int32_t> parent, childOff, childIdx;
	std::vector<double> blen;
	std::vector<std::string> names;
};
namespace {
struct NwNode { std::string name; double len = 0; std::vector<int32_t> kids; };
inline bool nw_space(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
inline bool nw_unquoted(unsigned char c) { return c > 0x20 && c < 0x7f && !strchr("()[]':;,", c); }
}
extern "C" int hu_newick_parse(const char* text, int64_t len, hu_newick** out) try {
	if(!text || len < 0 || !out) { hu_set_error("hu_newick_parse: bad argument"); return HU_ERR_ARG; }
	*out = nullptr;
	const std::string s(text, (size_t) len);           /* NUL-terminated for strtod */
	size_t pos = 0;
	auto skip = [&] { while(pos < s.size() && nw_space((unsigned char) s[pos])) ++pos; };
	auto fail = [&](const char* what) { hu_set_error("Newick: %s at byte %zu", what, pos); return HU_ERR_IO; };
	skip();
	if(pos == s.size()) return fail("empty tree");
	std::vector<NwNode> nd(1);
	std::vector<int32_t> open;                         /* nodes whose descendant list is being read */
	int32_t cur = 0;
	bool starting = true;                               /* cur may still open a descendant list */
	for(;;) {
		skip();
		if(starting && pos < s.size() && s[pos] == '(') {
			++pos; open.push_back(cur);
			nd[cur].kids.push_back((int32_t) nd.size()); cur = (int32_t) nd.size(); nd.emplace_back();
			continue;
		}
		/* label, then branch length, both optional */
		if(pos < s.size() && nw_unquoted((unsigned char) s[pos])) {
			const size_t a = pos;
			while(pos < s.size() && nw_unquoted((unsigned char) s[pos])) ++pos;
			nd[cur].name = s.substr(a, pos - a);
		}
		else if(pos < s.size() && s[pos] == '\'') {
			const size_t a = ++pos;
			while(pos < s.size() && s[pos] != '\'' && (unsigned char) s[pos] >= 0x20 && (unsigned char) s[pos] < 0x7f) ++pos;
			if(pos == a) return fail("empty quoted label");
			if(pos == s.size() || s[pos] != '\'') return fail("unterminated quoted label");
			nd[cur].name = s.substr(a, pos - a);
			++pos;
		}
		skip();
		if(pos < s.size() && s[pos] == ':') {
			++pos; skip();
			size_t q = pos;
			if(q < s.size() && (s[q] == '+' || s[q] == '-')) ++q;
			const bool numeric = q < s.size() && (isdigit((unsigned char) s[q]) || (s[q] == '.' && q + 1 < s.size() && isdigit((unsigned char) s[q + 1])));
			const bool word = q < s.size() && (!strncasecmp(s.c_str() + q, "inf", 3) || !strncasecmp(s.c_str() + q, "nan", 3));
			if(!numeric && !word) return fail("branch length expected");
			if(numeric && s[q] == '0' && q + 1 < s.size() && (s[q + 1] == 'x' || s[q + 1] == 'X')) { nd[cur].len = 0; pos = q + 1; }   /* no hexadecimal: the 0 is the number */
			else if(word) {
				const bool isInf = !strncasecmp(s.c_str() + q, "inf", 3), neg = s[pos] == '-';
				pos = q + (isInf && !strncasecmp(s.c_str() + q, "infinity", 8) ? 8 : 3);
				const double v = isInf ? std::numeric_limits<double>::infinity() : std::numeric_limits<double>::quiet_NaN();
				nd[cur].len = neg ? -v : v;
			}
			else { char* e = nullptr; nd[cur].len = strtod(s.c_str() + pos, &e); pos = (size_t)(e - s.c_str()); }
			skip();
		}
		/* the subtree of cur is complete */
		if(open.empty()) break;
		if(pos < s.size() && s[pos] == ',') {
			++pos;
			nd[open.back()].kids.push_back((int32_t) nd.size()); cur = (int32_t) nd.size(); nd.emplace_back();
			starting = true;
			continue;
		}
		if(pos < s.size() && s[pos] == ')') { ++pos; cur = open.back(); open.pop_back(); starting = false; continue; }
		return fail(pos == s.size() || s[pos] == ';' ? "unbalanced brackets: ')' expected" : "',' or ')' expected");
	}
	if(pos == s.size() || s[pos] != ';') return fail(pos < s.size() && s[pos] == ')' ? "unbalanced brackets: ')' without '('" : "';' expected");
	++pos; skip();
	if(pos != s.size()) return fail("text after the closing ';'");
	if(nd.size() >= (size_t) 1 << 24) { hu_set_error("Newick: %zu nodes, at most %d are supported", nd.size(), (1 << 24) - 1); return HU_ERR_ARG; }
	/* ids: depth-first with an explicit stack, children pushed in file order */
	std::unique_ptr<hu_newick> t(new hu_newick);
	const size_t n = nd.size();
	std::vector<int32_t> idOf(n, -1), st{0}, parOf(n, -1);
	for(size_t i = 0; i < n; ++i) for(int32_t k : nd[i].kids) parOf[k] = (int32_t) i;
	t->parent.resize(n); t->blen.resize(n); t->names.resize(n);
	int32_t id = 0;
	while(!st.empty()) {
		const int32_t v = st.back(); st.pop_back();
		idOf[v] = id;
		t->parent[id] = parOf[v] < 0 ? -1 : idOf[parOf[v]];
		t->blen[id] = parOf[v] < 0 ? 0.0 : nd[v].len;
		t->names[id].swap(nd[v].name);
		++id;
		for(int32_t k : nd[v].kids) st.push_back(k);
	}
	t->childOff.assign(n + 1, 0);
	for(size_t v = 0; v < n; ++v) t->childOff[idOf[v] + 1] = (int32_t) nd[v].kids.size();
	for(size_t i = 0; i < n; ++i) t->childOff[i + 1] += t->childOff[i];
	t->childIdx.resize(n - 1);
	for(size_t v = 0; v < n; ++v) { int32_t o = t->childOff[idOf[v]]; for(int32_t k : nd[v].kids) t->childIdx[o++] = idOf[k]; }
	*out = t.release();
	return HU_OK;
} catch(...) { return hu_catch_all("hu_newick_parse"); }
extern "C" void hu_newick_free(hu_newick* t) { delete t; }
extern "C" int hu_newick_size(const hu_newick* t, int32_t* n_nodes) { if(!t || !n_nodes) return HU_ERR_ARG; *n_nodes = (int32_t) t->parent.size(); return HU_OK; }
extern "C" int hu_newick_get(const hu_newick* t, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx) {
	if(!t) return HU_ERR_ARG;
	if(parent) memcpy(parent, t->parent.data(), t->parent.size() * 4);
	if(blen) memcpy(blen, t->blen.data(), t->blen.size() * 8);
	if(child_off) memcpy(child_off, t->childOff.data(), t->childOff.size() * 4);
	if(child_idx && !t->childIdx.empty()) memcpy(child_idx, t->childIdx.data(), t->childIdx.size() * 4);
	return HU_OK;
}
extern "C" const char* hu_newick_name(const hu_newick* t, int32_t node) { return t && node >= 0 && node < (int32_t) t->names.size() ? t->names[node].c_str() : ""; }
/* the tree written back with other lengths (hmmufotu-amd-tree --ml-lengths): children in file order, iterative like the reader */
extern "C" int64_t hu_newick_write(const hu_newick* t, const double* blen, char* buf, int64_t cap) try {
	if(!t || !blen || cap < 0 || (cap > 0 && !buf)) { hu_set_error("hu_newick_write: bad argument"); return HU_ERR_ARG; }
	const size_t n = t->parent.size();
	std::string out;
	char num[40];
	auto close_node = [&](int32_t v) {
		const std::string& s = t->names[v];
		bool plain = true;
		for(unsigned char c : s) if(!nw_unquoted(c)) plain = false;
		if(plain) out += s; else { out += '\''; out += s; out += '\''; }
		if(t->parent[v] >= 0) { snprintf(num, sizeof(num), ":%.17g", blen[v]); out += num; }
	};
	std::vector<std::pair<int32_t, int32_t>> st;       /* node, next child */
	st.push_back({0, t->childOff[0]});
	if(n > 1) out += '(';
	while(!st.empty()) {
		auto& f = st.back();
		const int32_t v = f.first;
		if(f.second < t->childOff[v + 1]) {
			if(f.second > t->childOff[v]) out += ',';
			const int32_t c = t->childIdx[f.second++];
			if(t->childOff[c] != t->childOff[c + 1]) out += '(';
			st.push_back({c, t->childOff[c]});
			continue;
		}
		if(t->childOff[v] != t->childOff[v + 1]) out += ')';
		close_node(v);
		st.pop_back();
	}
	out += ";\n";
	if(cap > 0) { const size_t k = std::min<size_t>(out.size(), (size_t) cap - 1); memcpy(buf, out.data(), k); buf[k] = 0; }
	return (int64_t) out.size();
} catch(...) { return hu_catch_all("hu_newick_write"); }

/* ---- loadAnnotation, formatName, annotate (src/PhyloTreeUnrooted.cpp:223-240, :956-1006; src/PhyloTreeUnrooted.h:1531-1578) ---- */
struct hu_tree_anno { std::vector<std::string> names, annos; std::vector<double> dist; };
namespace {
/* boost::split(fields, s, is_any_of(";: "), token_compress_on): a run of separators ends a field; a separator at either end leaves an empty field there */
std::vector<std::string> taxon_fields(const std::string& s) {
	std::vector<std::string> f(1);
	bool inSep = false;
	for(char c : s) {
		if(c == ';' || c == ':' || c == ' ') { if(!inSep) f.emplace_back(); inSep = true; }
		else { f.back() += c; inSep = false; }
	}
	return f;
}
bool taxon_canonical(const std::string& x) { return x.size() > 3 && x[1] == '_' && x[2] == '_' && strchr("dkpcofgs", x[0]) != nullptr; }
bool taxon_full(const std::string& s) {
	static const char level[] = "kpcofgs";
	const std::vector<std::string> f = taxon_fields(s);
	for(size_t i = 0; i < f.size(); ++i) if(i < 7 && !(f[i].size() >= 3 && f[i][0] == level[i] && f[i][1] == '_' && f[i][2] == '_')) return false;   /* past Species the prefix is "" */
	return true;
}
bool taxon_partial(const std::string& s) { for(const std::string& x : taxon_fields(s)) if(!taxon_canonical(x)) return false; return true; }
std::string taxon_format(const std::string& s) {
	if(s.empty()) return s;
	std::string o;
	for(const std::string& x : taxon_fields(s)) if(taxon_canonical(x)) { if(!o.empty()) o += ';'; o += x; }
	return o;
}
}
extern "C" int hu_tree_annotate(int32_t n, const int32_t* parent, const double* blen, const char* const* names, const char* anno_text,
		int64_t anno_len, const char* root_name, hu_tree_anno** out) try {
	if(n < 1 || !parent || !blen || !names || !out || (anno_text && anno_len < 0)) { hu_set_error("hu_tree_annotate: bad argument"); return HU_ERR_ARG; }
	*out = nullptr;
	for(int32_t i = 0; i < n; ++i) if(parent[i] >= n || parent[i] == i) { hu_set_error("hu_tree_annotate: parent of node %d out of range", i); return HU_ERR_ARG; }
	std::unique_ptr<hu_tree_anno> a(new hu_tree_anno);
	a->names.resize(n); a->annos.resize(n); a->dist.assign(n, 0.0);
	for(int32_t i = 0; i < n; ++i) a->names[i] = names[i] ? names[i] : "";
	if(anno_text) {
		std::map<std::string, std::string> name2anno;
		std::string anno;                                   /* kept from line to line: see the header */
		const char* p = anno_text; const char* end = anno_text + anno_len;
		while(p < end) {
			const char* e = (const char*) memchr(p, '\n', (size_t)(end - p));
			const char* le = e ? e : end;
			const char* tab = (const char*) memchr(p, '\t', (size_t)(le - p));
			const std::string name(p, tab ? tab : le);
			if(tab) { const char* t2 = (const char*) memchr(tab + 1, '\t', (size_t)(le - tab - 1)); anno.assign(tab + 1, t2 ? t2 : le); }
			name2anno[name] = anno;
			p = le + 1;
		}
		for(int32_t i = 0; i < n; ++i) { auto it = name2anno.find(a->names[i]); if(it != name2anno.end()) a->names[i] = it->second; }
	}
	for(int32_t i = 0; i < n; ++i) a->names[i] = taxon_format(a->names[i]);
	std::vector<uint8_t> full(n), partial(n);
	for(int32_t i = 0; i < n; ++i) { full[i] = taxon_full(a->names[i]); partial[i] = taxon_partial(a->names[i]); }
	const std::string rootName = root_name ? root_name : "cellular_organisms";
	std::vector<int32_t> path;
	for(int32_t i = 0; i < n; ++i) {
		path.clear();
		int32_t p = i, steps = 0;
		while(!full[p] && parent[p] >= 0) {
			if(++steps > n) { hu_set_error("hu_tree_annotate: the parents of node %d form a cycle", i); return HU_ERR_ARG; }
			a->dist[i] += blen[p];
			if(partial[p]) path.push_back(p);
			p = parent[p];
		}
		if(full[p]) path.push_back(p);
		std::string s;
		for(size_t k = path.size(); k-- > 0;) { if(!s.empty()) s += ';'; s += a->names[path[k]]; }
		a->annos[i] = path.empty() ? rootName : s;
	}
	*out = a.release();
	return HU_OK;
} catch(...) { return hu_catch_all("hu_tree_annotate"); }
extern "C" void hu_tree_anno_free(hu_tree_anno* a) { delete a; }
extern "C" const char* hu_tree_anno_name(const hu_tree_anno* a, int32_t node) { return a && node >= 0 && node < (int32_t) a->names.size() ? a->names[node].c_str() : ""; }
extern "C" const char* hu_tree_anno_anno(const hu_tree_anno* a, int32_t node) { return a && node >= 0 && node < (int32_t) a->annos.size() ? a->annos[node].c_str() : ""; }
extern "C" int hu_tree_anno_dist(const hu_tree_anno* a, double* anno_dist) { if(!a || !anno_dist) return HU_ERR_ARG; memcpy(anno_dist, a->dist.data(), a->dist.size() * 8); return HU_OK; }
