// The distances averaged over rarefied draws on the device (hmmufotu-amd-unifrac --rarefy).
//
// A chunk of n repeats is resident at a time.  Unit a = z * S' + jj is kept sample jj of resident draw z; the select / ties / take
// kernels of hu_kern_draw.h leave its integer counters in out[], one per nonzero cell of the sample, in depth-first row order.
//   k_ur_reset     before a chunk's select: the keys of the groups (seed + repeat, a group per (sample, repeat) that is drawn) and the
//                  selection state of the units, so that the host builds the lists once and only launches afterwards.
//   k_ur_embed     one workgroup per unit: the counters become their inclusive prefix W (a workgroup scan, as k_al_pd's over presence),
//                  and a branch entry (k, lo, hi) of the sample gives P_z[k][jj] = (double)(W[hi-1] - W[lo-1]) / (double) depth into the
//                  zero-filled P_z [B][Sp].  Integers below 2^32 and one rounded division: the bits of hu_unifrac_embed on the draw's table.
//   k_ur_pairs     hu_kern_unifrac.h's workgroup of a (tile, slab), with the resident draw as the grid's third dimension.
//   k_ur_finish    a thread per pair of a tile: for the chunk's draws in ascending order it adds the draw's slabs in ascending order and
//                  divides, as k_unifrac_finish does, then takes one step of the recurrence (hu_ur_step) on mean and M2, which it
//                  holds in registers across the chunk; it stores the pair and its mirrored copy, and D_z when asked.
// No atomics in the floating-point path: every double is written by one thread, and added in an order that (table, tree, L) fix.
// Bounds: unit a < n * S' by the grid; cell0, br0, lo, hi, k come from the host's lists (hu_unifrac_rarefied_host.cpp), hi <= nnz, k < B.
#pragma once
#include "hu_common.h"
#include "hu_kern_alpha.h"
#include "hu_kern_unifrac.h"
#include "hu_unifrac_rarefied.h"

static __global__ __launch_bounds__(HU_AL_WG) void k_ur_reset(const HuAlSample* smp, const HuAlDraw* draw, HuAlSel* sel, HuAlGroup* grp,
		uint32_t nUnit, uint32_t nGrp, uint32_t grpPerDraw, uint64_t seed0) {
	const uint32_t a = blockIdx.x * HU_AL_WG + threadIdx.x;
	if(a < nUnit) {
		const HuAlDraw d = draw[a];
		if(d.m != 0) { HuAlSel s; s.prefix = 0; s.rank = d.m; s.eq = smp[d.smp].T; sel[a] = s; }
	}
	if(a < nGrp) {
		const uint64_t sd = seed0 + (uint64_t)(a / grpPerDraw);
		grp[a].k0 = (uint32_t)(sd & 0xffffffffu); grp[a].k1 = (uint32_t)(sd >> 32);
	}
}

static __global__ __launch_bounds__(HU_AL_WG) void k_ur_embed(const HuAlSample* smp, const HuAlBranch* br, const uint32_t* brK, const HuAlDraw* draw,
		uint32_t* out, double* P, uint32_t Sk, int64_t Sp, int64_t B, double depth) {
	__shared__ uint32_t ws[HU_AL_WAVES];
	const uint32_t a = blockIdx.x, z = a / Sk, jj = a - z * Sk;
	const HuAlDraw d = draw[a];
	const HuAlSample s = smp[d.smp];
	uint32_t* o = out + d.cell0;
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t carry = 0;
	for(uint32_t c0 = 0; c0 < s.nnz; c0 += HU_AL_WG) {
		const uint32_t c = c0 + threadIdx.x;
		const uint32_t v = c < s.nnz ? o[c] : 0u, incl = hu_draw_wave_scan(v, lane);
		if(lane == 63) ws[w] = incl;
		__syncthreads();
		uint32_t off = 0, tot = 0;
		#pragma unroll
		for(int x = 0; x < HU_AL_WAVES; ++x) { if(x < w) off += ws[x]; tot += ws[x]; }
		if(c < s.nnz) o[c] = carry + off + incl;
		carry += tot;
		__syncthreads();
	}
	const HuAlBranch* E = br + s.br0;
	const uint32_t* K = brK + s.br0;
	double* Pz = P + (int64_t) z * B * Sp + jj;
	for(uint32_t e = threadIdx.x; e < s.nBr; e += HU_AL_WG) {
		const HuAlBranch x = E[e];
		const uint32_t hi = o[x.hi - 1], lo = x.lo ? o[x.lo - 1] : 0u;
		Pz[(int64_t) K[e] * Sp] = (double)(hi - lo) / depth;
	}
}

/* grid (tiles, slabs, resident draws); P [draw][B][Sp], part [draw][slab][tile][2][64][64] */
template<int METHOD> __global__ void __launch_bounds__(HU_UF_WG) k_ur_pairs(const double* __restrict__ P, const double* __restrict__ blen,
		double* __restrict__ part, int64_t Sp, int64_t B, int64_t L, double alpha) {
	const int64_t z = blockIdx.z;
	hu_uf_pairs_wg<METHOD>(P + z * B * Sp, blen, part + z * (int64_t) gridDim.y * gridDim.x * (2 * HU_UF_TILE * HU_UF_TILE), Sp, B, L, alpha,
		(int) blockIdx.x, (int) blockIdx.y, (int) gridDim.x);
}

/* grid (tiles, 16): a thread per pair of the tile; r0 is the number of draws taken before this chunk */
static __global__ void __launch_bounds__(256) k_ur_finish(const double* __restrict__ part, double* __restrict__ mean, double* __restrict__ m2,
		double* __restrict__ D, int64_t S, int64_t Sp, int64_t nSlab, int raw, int64_t nDraw, int64_t r0) {
	const int nt = (int)(Sp / HU_UF_TILE);
	int t = blockIdx.x, iblk = 0;
	while(t >= nt - iblk) { t -= nt - iblk; ++iblk; }
	const int jblk = iblk + t;
	const int e = blockIdx.y * 256 + threadIdx.x, row = e >> 6, col = e & 63;
	const int64_t i = (int64_t) iblk * HU_UF_TILE + row, j = (int64_t) jblk * HU_UF_TILE + col;
	if(i >= S || j >= S || i > j) return;
	if(i == j) {
		mean[i * S + i] = 0.0; m2[i * S + i] = 0.0;
		if(D) for(int64_t z = 0; z < nDraw; ++z) D[z * S * S + i * S + i] = 0.0;
		return;
	}
	double mu = r0 ? mean[i * S + j] : 0.0, q = r0 ? m2[i * S + j] : 0.0;
	const int64_t perDraw = nSlab * gridDim.x * (2 * HU_UF_TILE * HU_UF_TILE);
	for(int64_t z = 0; z < nDraw; ++z) {
		double N = 0.0, Dn = 0.0;
		for(int64_t s = 0; s < nSlab; ++s) {
			const double* p = part + z * perDraw + (s * gridDim.x + blockIdx.x) * (2 * HU_UF_TILE * HU_UF_TILE) + e;
			N += p[0];
			if(!raw) Dn += p[HU_UF_TILE * HU_UF_TILE];
		}
		const double d = raw ? N : Dn > 0 ? N / Dn : 0.0;
		if(D) { D[z * S * S + i * S + j] = d; D[z * S * S + j * S + i] = d; }
		hu_ur_step(d, (double)(r0 + z + 1), mu, q);
	}
	mean[i * S + j] = mu; mean[j * S + i] = mu;
	m2[i * S + j] = q; m2[j * S + i] = q;
}
