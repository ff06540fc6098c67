// Simulated reads from the database's own messages (hmmufotu-sim, src/hmmufotu-sim.cpp:382-423).
//
// A read is a point on the branch above node c: p = parent[c], v = blen[c], the point lies v * rc above c.  At column j the reference
// forms  dot_product_scaled(Pr(v rc), msg(c -> p, j)) + dot_product_scaled(Pr(v (1 - rc)), msg(p -> c, j))  in log space, takes
// exp(. - max) and draws the base from those four weights (:401-407).  The messages lie in HBM in linear space and in the eigenbasis of
// the model (HuDbDev::up / down: a = U^-1 e), where Pr(t) is the diagonal exp(lam t), so per site this is
//     x = U (D1 o up[c][j]),  y = U (D2 o down[c][j]),  q_i = max(x_i y_i, 0),     D1 = exp(lam v rc),  D2 = exp(lam v (1 - rc)):
// two 4 x 4 mat-vecs and no transcendental; the eight exponentials belong to the read.  The power-of-two exponents of the packed
// messages (upK / downK) are common to the four q_i and cancel in the draw: they are not read.  The plain model's Pr is meant: the
// reference does not apply the database's discrete-Gamma rates here either.
//
// One workgroup of 256 lanes per read, lanes on consecutive columns: the two 32-byte loads of a site coalesce along [node][column][4].
// Per tile of 256 columns every lane decides its column (gap, or a base), writes the aligned row's byte, and the residues are
// compacted into the ungapped sequence: a ballot and a population count inside the wave, the four wave totals through LDS, the running
// offset carried from tile to tile.  The mate, when asked for, is the reverse complement of that sequence, written once its length
// is known.  Every index formed here (node, columns, the offsets of the outputs) is checked by hu_sim_reads before the launch.
#pragma once
#include "hu_common.h"
#include "hu_sim_rng.h"

#define HU_SIM_BLOCK 256

struct HuSimArgs {
	const double* up;          /* HuDbDev::up / down of a database that holds ALL columns: [n][csLen][4] */
	const double* down;
	const double* blen;        /* [n] */
	int64_t csLen;
	const double* gapFrac;     /* [csLen] */
	const int32_t* node;       /* [R] never the root */
	const double* rc;          /* [R] in [0, 1] */
	const int32_t* start;      /* [R] 0 <= start <= end < csLen */
	const int32_t* end;
	const int64_t* off;        /* [R] first byte of the read in the three outputs: the columns of the reads before it */
	uint32_t key0, key1;       /* seed & 0xffffffff, seed >> 32 */
	uint64_t read0;            /* global index of read 0 */
	char* aligned;             /* [sum of columns] ACGT- */
	char* seq;                 /* the same room: the read's residues, seqLen[r] of them */
	char* mate;                /* nullptr: no mates */
	int32_t* seqLen;           /* [R] */
};

__device__ __forceinline__ double sim_row(const double* U, const double* s) { return (U[0] * s[0] + U[1] * s[1]) + (U[2] * s[2] + U[3] * s[3]); }

__global__ __launch_bounds__(HU_SIM_BLOCK) void k_sim_reads(HuModelDev mdl, HuSimArgs a) {
	__shared__ double sD[8];
	__shared__ int32_t sCnt[2][HU_SIM_BLOCK / 64];
	const int64_t r = blockIdx.x;
	const int lane = threadIdx.x, wave = lane >> 6, wl = lane & 63;
	const int32_t c = a.node[r], s = a.start[r], cols = a.end[r] - s + 1;
	if(lane < 8) { /* the read's eight exponentials, one per lane */
		const double v = a.blen[c], rc = a.rc[r];
		const int k = lane & 3;
		const double lam = k == 0 ? mdl.lam[0] : k == 1 ? mdl.lam[1] : k == 2 ? mdl.lam[2] : mdl.lam[3];
		sD[lane] = exp(lam * (lane < 4 ? v * rc : v * (1 - rc)));
	}
	__syncthreads();
	const double D1[4] = {sD[0], sD[1], sD[2], sD[3]}, D2[4] = {sD[4], sD[5], sD[6], sD[7]};
	const uint64_t g = a.read0 + (uint64_t) r;
	const uint32_t key[2] = {a.key0, a.key1};
	const int64_t o = a.off[r];
	const double* mu = a.up + (int64_t) c * a.csLen * 4;
	const double* md = a.down + (int64_t) c * a.csLen * 4;
	int32_t filled = 0;                                   /* residues of the tiles before this one */
	int par = 0;
	for(int32_t j0 = 0; j0 < cols; j0 += HU_SIM_BLOCK, par ^= 1) {
		const int32_t jj = j0 + lane;
		const bool have = jj < cols;
		char ch = '-';
		if(have) {
			const int32_t j = s + jj;
			const uint32_t ctr[4] = {(uint32_t) j, (uint32_t) g, (uint32_t)(g >> 32), 0u};
			uint32_t w[4];
			hu_philox4x32_10(ctr, key, w);
			if(!(hu_sim_u01(w[0], w[1]) <= a.gapFrac[j])) {
				const double2 u0 = *reinterpret_cast<const double2*>(mu + (int64_t) j * 4), u1 = *reinterpret_cast<const double2*>(mu + (int64_t) j * 4 + 2);
				const double2 d0 = *reinterpret_cast<const double2*>(md + (int64_t) j * 4), d1 = *reinterpret_cast<const double2*>(md + (int64_t) j * 4 + 2);
				const double su[4] = {D1[0] * u0.x, D1[1] * u0.y, D1[2] * u1.x, D1[3] * u1.y};
				const double sd[4] = {D2[0] * d0.x, D2[1] * d0.y, D2[2] * d1.x, D2[3] * d1.y};
				const double q0 = fmax(sim_row(mdl.U, su) * sim_row(mdl.U, sd), 0.0), q1 = fmax(sim_row(mdl.U + 4, su) * sim_row(mdl.U + 4, sd), 0.0);
				const double q2 = fmax(sim_row(mdl.U + 8, su) * sim_row(mdl.U + 8, sd), 0.0), q3 = fmax(sim_row(mdl.U + 12, su) * sim_row(mdl.U + 12, sd), 0.0);
				const double c1 = q0 + q1, c2 = c1 + q2, S = c2 + q3;
				const double t = hu_sim_u01(w[2], w[3]) * S;
				ch = t < q0 ? 'A' : t < c1 ? 'C' : t < c2 ? 'G' : 'T';
			}
			a.aligned[o + jj] = ch;
		}
		const bool keep = have && ch != '-';
		const unsigned long long m = __ballot(keep);
		if(wl == 0) sCnt[par][wave] = __popcll(m);
		__syncthreads();                                  /* the totals of tile t + 1 go to the other half of sCnt: one barrier per tile */
		int32_t before = 0, total = 0;
		#pragma unroll
		for(int w2 = 0; w2 < HU_SIM_BLOCK / 64; ++w2) { const int32_t n = sCnt[par][w2]; before += w2 < wave ? n : 0; total += n; }
		if(keep) a.seq[o + filled + before + __popcll(m & ((1ull << wl) - 1ull))] = ch;
		filled += total;
	}
	if(lane == 0) a.seqLen[r] = filled;
	if(a.mate) { /* PrimarySeq::revcom of the whole insert (src/hmmufotu-sim.cpp:422) */
		__syncthreads();                                  /* the workgroup's own stores to seq are visible to it behind the barrier */
		for(int32_t k = lane; k < filled; k += HU_SIM_BLOCK) {
			const char b = a.seq[o + filled - 1 - k];
			a.mate[o + k] = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
		}
	}
}
