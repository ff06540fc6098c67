// hu_msa_pair_counts, hu_msa_distances, hu_nj and hu_msa_tree: the entries and the device path of hmmufotu-amd-tree.
// The checks, the host path and the Newick writer are hu_nj_host.cpp's; the kernels are those of hu_kern_dist.h and hu_kern_nj.h.
// One work area holds everything a call needs on the device, and its size is held against the free memory before it is allocated.
#include <algorithm>
#include <cstring>
#include <vector>
#include "hu_tree_dev.h"
#include "hu_kern_dist.h"
#include "hu_kern_nj.h"

static thread_local double g_njTiming[4] = {0, 0, 0, 0};

extern "C" int hu_nj_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_njTiming, sizeof(g_njTiming));
	return HU_OK;
}

namespace {
struct TreeWork {
	int8_t* rows = nullptr; uint64_t* plane = nullptr; double* D = nullptr; int32_t* counts = nullptr;
	double* R = nullptr; int32_t* id = nullptr; HuNjCand* cand = nullptr; HuNjCand* win = nullptr; int32_t* join = nullptr; double* len = nullptr;
	double* blkMax = nullptr; unsigned long long* blkInf = nullptr;
	~TreeWork() {
		(void) hipFree(rows); (void) hipFree(plane); (void) hipFree(D); (void) hipFree(counts); (void) hipFree(R); (void) hipFree(id); (void) hipFree(cand);
		(void) hipFree(win); (void) hipFree(join); (void) hipFree(len); (void) hipFree(blkMax); (void) hipFree(blkInf);
	}
};
struct TreeSizes { int64_t np, Wp; size_t rows, plane, D, counts, vec, need; };
}

/* what a call needs on the device: dist (the rows and the planes), counts, nj (the vectors); the matrix unless counts alone */
static TreeSizes tree_sizes(int64_t n, int64_t cs_len, bool dist, bool counts, bool nj) {
	TreeSizes s; memset(&s, 0, sizeof(s));
	s.np = (n + HU_DIST_TILE - 1) / HU_DIST_TILE * HU_DIST_TILE;
	s.Wp = ((cs_len + 63) / 64 + HU_DIST_CHUNK - 1) / HU_DIST_CHUNK * HU_DIST_CHUNK;
	if(dist || counts) { s.rows = (size_t) n * (size_t) cs_len; s.plane = (size_t) 3 * (size_t) s.np * (size_t) s.Wp * 8; }
	if(counts) s.counts = (size_t) n * (size_t) n * 16;
	else s.D = (size_t) n * (size_t) n * 8;
	if(dist) s.vec += HU_NJ_PICK_WG * 16;
	if(nj) s.vec += (size_t) n * 12 + (HU_NJ_PICK_WG + 1) * sizeof(HuNjCand) + (size_t)(2 * n) * 12;
	s.need = s.rows + s.plane + s.D + s.counts + s.vec + (1 << 20);
	return s;
}

static int tree_reserve(const char* fn, int device, int64_t n, int64_t cs_len, const TreeSizes& s, int64_t budget) {
	if(hu_device_count() <= 0) { hu_set_error("%s: no gfx950 device visible: the host path needs none", fn); return HU_ERR_DEVICE; }
	TCHK(hipSetDevice(device));
	size_t freeB = 0, totB = 0;
	TCHK(hipMemGetInfo(&freeB, &totB));
	if(budget > 0 && (size_t) budget < freeB) freeB = (size_t) budget;
	if(s.need > freeB) {
		hu_set_error("%s: %lld rows of %lld columns need %zu bytes of device memory (the matrix %zu, the rows and their bit-planes %zu, the vectors %zu), %zu bytes are free",
			fn, (long long) n, (long long) cs_len, s.need, s.D + s.counts, s.rows + s.plane, s.vec, freeB);
		return HU_ERR_NOMEM;
	}
	return HU_OK;
}

/* rows up, planes made */
static int tree_encode(const char* fn, TreeWork& w, const TreeSizes& s, int64_t n, int64_t cs_len, const int8_t* rows) {
	TCHK(hipMalloc((void**) &w.rows, s.rows)); TCHK(hipMalloc((void**) &w.plane, s.plane));
	TCHK(hipMemcpy(w.rows, rows, s.rows, hipMemcpyHostToDevice));
	for(int64_t r0 = 0; r0 < s.np; r0 += 65535) {                        /* grid.y holds 65535 */
		const int64_t nr = std::min<int64_t>(65535, s.np - r0);
		/* the kernel takes its row from blockIdx.y: the pointers of a later slice start at its first row */
		k_dist_encode<<<dim3((unsigned)((s.Wp + 255) / 256), (unsigned) nr), 256>>>(w.rows + r0 * cs_len, w.plane + r0 * s.Wp, n - r0, cs_len, s.np, s.Wp);
		TCHK(hipGetLastError());
	}
	return HU_OK;
}

static HuDistArgs dist_args(const TreeWork& w, const TreeSizes& s, int64_t n, int type, const double* pi) {
	HuDistArgs a; memset(&a, 0, sizeof(a));
	a.plane = w.plane; a.np = s.np; a.Wp = s.Wp; a.n = n; a.type = type; a.D = w.D; a.counts = w.counts;
	for(int b = 0; b < 4; ++b) a.pi[b] = pi ? pi[b] : 0.25;
	return a;
}

static int64_t dist_tiles(const TreeSizes& s) { const int64_t nt = s.np / HU_DIST_TILE; return nt * (nt + 1) / 2; }

/* D on the device from the planes; the saturated pairs counted and given `sat`, or with sat == 0 twice the largest finite distance */
static int tree_distances(const char* fn, TreeWork& w, const TreeSizes& s, int64_t n, int type, const double* pi, double sat, int64_t* n_sat) {
	const int64_t tiles = dist_tiles(s);
	if(tiles > 0x7fffffffll) { hu_set_error("%s: %lld tiles: more than a grid holds", fn, (long long) tiles); return HU_ERR_ARG; }
	k_dist_pairs<false><<<(unsigned) tiles, HU_DIST_WG>>>(dist_args(w, s, n, type, pi));
	TCHK(hipGetLastError());
	if(n_sat) *n_sat = 0;
	if(type == HU_DIST_PDIST) return HU_OK;                               /* no logarithm: never saturated */
	const int G = (int) std::min<int64_t>(n, HU_NJ_PICK_WG);
	TCHK(hipMalloc((void**) &w.blkMax, (size_t) G * 8)); TCHK(hipMalloc((void**) &w.blkInf, (size_t) G * 8));
	k_dist_scan<<<G, 256>>>(w.D, n, w.blkMax, w.blkInf);
	TCHK(hipGetLastError());
	std::vector<double> mx((size_t) G); std::vector<unsigned long long> ni((size_t) G);
	TCHK(hipMemcpy(mx.data(), w.blkMax, (size_t) G * 8, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(ni.data(), w.blkInf, (size_t) G * 8, hipMemcpyDeviceToHost));
	double m = -1.0; unsigned long long c = 0;
	for(int g = 0; g < G; ++g) { if(mx[(size_t) g] > m) m = mx[(size_t) g]; c += ni[(size_t) g]; }
	if(n_sat) *n_sat = (int64_t) c;
	if(c == 0) return HU_OK;
	if(!(sat > 0) && m < 0) { hu_set_error("%s: every pair of rows is saturated: no finite distance to scale from, give one", fn); return HU_ERR_ARG; }
	const int64_t total = n * n;
	k_dist_fix<<<(unsigned) std::min<int64_t>((total + 255) / 256, 65536), 256>>>(w.D, total, sat > 0 ? sat : 2 * m);
	TCHK(hipGetLastError());
	return HU_OK;
}

/* the joins on w.D, which is used up; the records come back in one copy each */
static int tree_nj(const char* fn, TreeWork& w, int64_t n, int32_t* join, double* len, int32_t* last3, double* last_len3) {
	const size_t nRec = (size_t)(2 * (n - 3) + 3);
	TCHK(hipMalloc((void**) &w.R, (size_t) n * 8)); TCHK(hipMalloc((void**) &w.id, (size_t) n * 4));
	TCHK(hipMalloc((void**) &w.cand, HU_NJ_PICK_WG * sizeof(HuNjCand))); TCHK(hipMalloc((void**) &w.win, sizeof(HuNjCand)));
	TCHK(hipMalloc((void**) &w.join, nRec * 4)); TCHK(hipMalloc((void**) &w.len, nRec * 8));
	{
		std::vector<int32_t> id((size_t) n);
		for(int64_t i = 0; i < n; ++i) id[(size_t) i] = (int32_t) i;
		TCHK(hipMemcpy(w.id, id.data(), (size_t) n * 4, hipMemcpyHostToDevice));
	}
	HuNjDev a; a.D = w.D; a.R = w.R; a.id = w.id; a.n = n; a.cand = w.cand; a.win = w.win; a.join = w.join; a.len = w.len;
	k_nj_rowsum<<<(unsigned) n, 256>>>(a, n, 0);
	TCHK(hipGetLastError());
	int64_t r = n;
	for(int64_t t = 0; t < n - 3; ++t, --r) {
		const int G = (int) std::min<int64_t>(r - 1, HU_NJ_PICK_WG);
		k_nj_pick<<<G, 256>>>(a, r);
		k_nj_winner<<<1, 256>>>(a, r, t, G);
		k_nj_update<<<(unsigned)((r + 255) / 256), 256>>>(a, r);
		k_nj_move<<<(unsigned)((r - 1 + 255) / 256), 256>>>(a, r);
		k_nj_rowsum<<<1, 256>>>(a, r - 1, 1);
		if((t & 1023) == 1023) TCHK(hipGetLastError());
	}
	k_nj_end<<<1, 64>>>(a);
	TCHK(hipGetLastError());
	TCHK(hipDeviceSynchronize());
	std::vector<int32_t> hj(nRec); std::vector<double> hl(nRec);
	TCHK(hipMemcpy(hj.data(), w.join, nRec * 4, hipMemcpyDeviceToHost)); TCHK(hipMemcpy(hl.data(), w.len, nRec * 8, hipMemcpyDeviceToHost));
	const size_t m = (size_t)(2 * (n - 3));
	if(m) { memcpy(join, hj.data(), m * 4); memcpy(len, hl.data(), m * 8); }
	memcpy(last3, hj.data() + m, 12); memcpy(last_len3, hl.data() + m, 24);
	return HU_OK;
}

extern "C" int hu_msa_pair_counts(int device, int64_t n, int64_t cs_len, const int8_t* rows, int32_t* counts) try {
	const char* fn = "hu_msa_pair_counts";
	if(!counts) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	const int rc = hu_dist_check(fn, n, cs_len, rows, HU_DIST_PDIST, nullptr, 0.0);
	if(rc != HU_OK) return rc;
	if(device < 0) { hu_dist_host_counts(n, cs_len, rows, counts); return HU_OK; }
	const TreeSizes s = tree_sizes(n, cs_len, false, true, false);
	const int rr = tree_reserve(fn, device, n, cs_len, s, 0);
	if(rr != HU_OK) return rr;
	TreeWork w;
	const int re = tree_encode(fn, w, s, n, cs_len, rows);
	if(re != HU_OK) return re;
	TCHK(hipMalloc((void**) &w.counts, s.counts));
	k_dist_pairs<true><<<(unsigned) dist_tiles(s), HU_DIST_WG>>>(dist_args(w, s, n, HU_DIST_PDIST, nullptr));
	TCHK(hipGetLastError());
	TCHK(hipMemcpy(counts, w.counts, s.counts, hipMemcpyDeviceToHost));
	return HU_OK;
} catch(...) { return hu_catch_all("hu_msa_pair_counts"); }

/* the three entries that fill or use the matrix: rows == NULL: D_in is the matrix; join == NULL: the distances alone */
static int tree_run(const char* fn, int device, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, const hu_nj_opts* opts,
		const double* D_in, double* D_out, int64_t* n_sat, int32_t* join, double* len, int32_t* last3, double* last_len3) {
	hu_nj_opts o;
	hu_nj_default_opts(&o);
	if(opts) o = *opts;
	const bool dist = rows != nullptr, nj = last3 != nullptr, host = o.host != 0 || device < 0;
	if(nj && (!last_len3 || (n > 3 && (!join || !len)))) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	if(o.mem_budget < 0) { hu_set_error("%s: a memory budget below 0", fn); return HU_ERR_ARG; }
	if(dist) { const int rc = hu_dist_check(fn, n, cs_len, rows, dist_type, pi, sat); if(rc != HU_OK) return rc; }
	if(nj && n < 3) { hu_set_error("%s: %lld rows: a tree needs 3", fn, (long long) n); return HU_ERR_ARG; }
	if(!dist) { const int rc = hu_nj_check(fn, n, D_in); if(rc != HU_OK) return rc; }
	g_njTiming[0] = g_njTiming[1] = g_njTiming[2] = g_njTiming[3] = 0;
	if(host) {
		std::vector<double> own;
		double* D = D_out;
		if(!D) { own.resize((size_t) n * (size_t) n); D = own.data(); }
		if(dist) { const int rc = hu_dist_host(fn, n, cs_len, rows, dist_type, pi, sat, D, n_sat); if(rc != HU_OK) return rc; }
		if(!nj) return HU_OK;
		std::vector<double> work(dist ? D : D_in, (dist ? D : D_in) + (size_t) n * (size_t) n);     /* the joins use their matrix up */
		hu_nj_host_run(n, work.data(), join, len, last3, last_len3);
		return HU_OK;
	}
	const TreeSizes s = tree_sizes(n, cs_len, dist, false, nj);
	const int rr = tree_reserve(fn, device, n, cs_len, s, o.mem_budget);
	if(rr != HU_OK) return rr;
	TreeWork w;
	double t0 = hu_now_s();
	TCHK(hipMalloc((void**) &w.D, s.D));
	if(dist) {
		const int re = tree_encode(fn, w, s, n, cs_len, rows);
		if(re != HU_OK) return re;
	}
	else TCHK(hipMemcpy(w.D, D_in, s.D, hipMemcpyHostToDevice));
	TCHK(hipDeviceSynchronize());
	g_njTiming[0] = hu_now_s() - t0; t0 = hu_now_s();
	if(dist) {
		const int rd = tree_distances(fn, w, s, n, dist_type, pi, sat, n_sat);
		if(rd != HU_OK) return rd;
		TCHK(hipDeviceSynchronize());
		g_njTiming[1] = hu_now_s() - t0; t0 = hu_now_s();
		if(D_out) TCHK(hipMemcpy(D_out, w.D, s.D, hipMemcpyDeviceToHost));
		g_njTiming[3] = hu_now_s() - t0; t0 = hu_now_s();
	}
	if(nj) {
		const int rn = tree_nj(fn, w, n, join, len, last3, last_len3);
		if(rn != HU_OK) return rn;
		g_njTiming[2] = hu_now_s() - t0;
	}
	return HU_OK;
}

extern "C" int hu_msa_distances(int device, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, double* D,
		int64_t* n_saturated) try {
	const char* fn = "hu_msa_distances";
	if(!D || !rows) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	return tree_run(fn, device, n, cs_len, rows, dist_type, pi, sat, nullptr, nullptr, D, n_saturated, nullptr, nullptr, nullptr, nullptr);
} catch(...) { return hu_catch_all("hu_msa_distances"); }

extern "C" int hu_nj(int device, int64_t n, const double* D, const hu_nj_opts* opts, int32_t* join, double* len, int32_t* last3, double* last_len3) try {
	const char* fn = "hu_nj";
	if(!last3) { hu_set_error("%s: null output", fn); return HU_ERR_ARG; }
	return tree_run(fn, device, n, 0, nullptr, 0, nullptr, 0.0, opts, D, nullptr, nullptr, join, len, last3, last_len3);
} catch(...) { return hu_catch_all("hu_nj"); }

extern "C" int hu_msa_tree(int device, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, const hu_nj_opts* opts,
		double* D_out, int64_t* n_saturated, int32_t* join, double* len, int32_t* last3, double* last_len3) try {
	const char* fn = "hu_msa_tree";
	if(!rows || !last3) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	return tree_run(fn, device, n, cs_len, rows, dist_type, pi, sat, opts, nullptr, D_out, n_saturated, join, len, last3, last_len3);
} catch(...) { return hu_catch_all("hu_msa_tree"); }
