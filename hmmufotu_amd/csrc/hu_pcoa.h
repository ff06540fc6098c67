// What the host half (hu_pcoa_host.cpp, a plain C++ compiler) and the device half (hu_pcoa.cpp, hu_kern_pcoa.h) of hu_pcoa share
// (DESIGN.md §28): the checked arguments of a call, the constants that fix the layout and the order of the sums, the start block, and
// the block iteration itself, which is written once against the six operations of HuPcOps and runs on either half.
#pragma once
#include <stdint.h>
#include <vector>
#include "hu_sim_rng.h"
#include "../../include/hmmufotu_amd.h"

#define HU_PCOA_TILE 64            /* rows of the matrix per workgroup of the product kernel */
#define HU_PCOA_KT 32              /* columns of the matrix per staged tile of the product kernel; a slab is a whole number of them */
#define HU_PCOA_MAX_MP 64          /* the block's padded width at the most: four accumulator tiles per wave */
#define HU_PCOA_MAX_SLABS 8        /* K slabs of the product at the most */
#define HU_PCOA_SLAB_MIN 128       /* columns of the matrix per slab at the least: S = min(8, ceil(n / 128)) */
#define HU_PCOA_CHUNK 256          /* rows per partial of the column sums and of the Gram matrices */
#define HU_PCOA_KEEP 1e-7          /* a Ritz vector with |theta| <= this * max |theta| is kept, not multiplied, in the power step */
#define HU_PCOA_GROW_AFTER 3       /* iterations of a block before too few positive Ritz values widen it */

/* the block's width padded to whole accumulator tiles */
inline int64_t hu_pc_pad(int64_t m) { return (m + 15) / 16 * 16; }
/* the K slabs of the product: a function of n alone */
inline int64_t hu_pc_slabs(int64_t n) { const int64_t s = (n + HU_PCOA_SLAB_MIN - 1) / HU_PCOA_SLAB_MIN; return s < 1 ? 1 : s > HU_PCOA_MAX_SLABS ? HU_PCOA_MAX_SLABS : s; }
/* the columns of a slab: ceil(n / S) rounded up to whole staged tiles; slab s is [s L, min(n, (s + 1) L)), empty where s L >= n */
inline int64_t hu_pc_slab_len(int64_t n) { const int64_t s = hu_pc_slabs(n), l = (n + s - 1) / s; return (l + HU_PCOA_KT - 1) / HU_PCOA_KT * HU_PCOA_KT; }
inline int64_t hu_pc_chunks(int64_t n) { return (n + HU_PCOA_CHUNK - 1) / HU_PCOA_CHUNK; }
/* the bytes on the device for a block of m columns */
inline int64_t hu_pc_need_m(int64_t n, int64_t m) {
	const int64_t mp = hu_pc_pad(m), c = hu_pc_chunks(n);
	return 8 * n * n + 8 * (hu_pc_slabs(n) + 4) * n * mp + 8 * (c + 3) * mp * mp + 8 * c * mp + (1 << 20);
}

/* entry (row, col) of the start block: a uniform of [-1/2, 1/2) named by (seed, row, col) alone */
inline double hu_pc_start(uint64_t seed, uint64_t row, uint64_t col) {
	const uint32_t c[4] = {(uint32_t) row, (uint32_t)(row >> 32), (uint32_t) col, (uint32_t)(col >> 32)}, k[2] = {(uint32_t) seed, (uint32_t)(seed >> 32)};
	uint32_t w[4];
	hu_philox4x32_10(c, k, w);
	return hu_sim_u01(w[1], w[0]) - 0.5;
}

struct HuPcPlan {
	int64_t n = 0, k = 0, oversample = 0, max_it = 0, budget = 0;
	double tol = 0;
	uint64_t seed = 1;
	bool host = false;
};

/* a block is n x mp doubles, row-major, the columns from m on zero; the operations name the four blocks they own by 0 .. 3 */
struct HuPcOps {
	virtual ~HuPcOps() {}
	/* room for blocks of m columns (mp = hu_pc_pad(m)); block `dst` = start [n][mp] from the host */
	virtual int setup(int64_t m, const double* start, int dst) = 0;
	/* dst = -1/2 J D2 src (the product, the column means and the scaling); src != dst */
	virtual int bv(int src, int dst) = 0;
	/* dst = J src; src != dst */
	virtual int centre(int src, int dst) = 0;
	/* G [mp][mp] (host) = x' y */
	virtual int gram(int x, int y, double* G) = 0;
	/* dst = x M1 + y M2 with M1, M2 [mp][mp] on the host; y < 0: dst = x M1; dst is neither x nor y */
	virtual int apply(int x, const double* M1, int y, const double* M2, int dst) = 0;
	/* out [n][mp] (host) = src */
	virtual int fetch(int src, double* out) = 0;
};

/* the arguments of hu_pcoa, checked (the matrix by hu_pm_check_matrix), and the plan */
int hu_pc_plan(const char* fn, int64_t n, const double* dist, const hu_pcoa_opts* opts, HuPcPlan& pl);
/* the iteration of DESIGN.md §28 on `ops`; trace = hu_pm_ss_total of the matrix */
int hu_pc_run(const char* fn, HuPcOps& ops, const HuPcPlan& pl, double trace, hu_pcoa_result* out, double* coords, double* eigval, double* resid);
/* the host's operations on dist [n][n] */
HuPcOps* hu_pc_host_ops(int64_t n, const double* dist);
/* seconds [6] of this thread's last call: the device half adds to slots 0 .. 3 and 5, hu_pc_run to slot 4 */
double* hu_pc_timing_slots();
/* the m x m work of the host, for the sanitizer driver: the lower Cholesky factor L of G in place (false: pivot j is not positive), the
 * eigenvalues and eigenvectors (columns of Q) of the symmetric H by cyclic Jacobi */
bool hu_pc_cholesky(int64_t m, int64_t ld, double* G, int64_t* fail);
void hu_pc_jacobi(int64_t m, int64_t ld, double* H, double* theta, double* Q);
