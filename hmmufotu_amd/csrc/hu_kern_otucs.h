// HIP kernels of the OTU consensus sequences of hmmufotu-sum -c (gfx950, wave64).  Included by hu_engine.hip.
//
//   k_otucs_count   per-OTU column counts of a batch of alignment rows: the loop of src/hmmufotu-sum.cpp:391-397
//                   (b = encode(toupper(aln[j])); b >= 0 ? freq(b, j)++ : gap(j)++) for every accepted read
//   k_otucs_infer   PTUnrooted::inferPostCS (src/PhyloTreeUnrooted.cpp:1111-1125): the Dirichlet prior from the node's message, the
//                   posterior with the counts, the first maximum or a gap, one symbol per (OTU, column)
//
// The counts live in one resident table of uint32, tab[slot][5][L]: planes 0..3 = freq of A C G T, plane 4 = gap (gap symbols and
// every invalid byte alike).  A slot is an OTU (a node) in the order the handle first saw it.  Integer sums: any order is exact.
#pragma once
#include "hu_common.h"

#ifndef HU_OTUCS_CPL
#define HU_OTUCS_CPL 16        /* columns per lane: one 16-byte load per row, a wave reads 1 KB of a row at a stretch */
#endif
#define HU_OTUCS_THREADS 256
#define HU_OTUCS_BLOCK_COLS (HU_OTUCS_CPL * HU_OTUCS_THREADS)
#define HU_OTUCS_CHUNK 64      /* rows of one OTU per workgroup: a heavy OTU is spread over many workgroups, which meet in the table's atomics */

/* one staged row: the bytes of its columns [c0, c1) stand at stage + off; every other column of the row is '-' (hu_otucs_add cuts a
 * row down to the span that holds anything else).  c0 and off are multiples of 16; c1 is one, or the row's length. */
struct HuOtucsRow { int32_t off16, c0, c1, pad; };
/* one workgroup's share: rows order[begin .. end) of the batch, all of OTU `slot` */
struct HuOtucsWork { int32_t slot, begin, end, pad; };

/* Grid (work items, column blocks).  A lane owns HU_OTUCS_CPL consecutive columns and keeps their 5 x CPL counters in registers over
 * the rows of its work item; the row index is wave-uniform, so a row's descriptor comes in through the scalar cache and the rows
 * themselves stay where the copy put them.  A row that does not reach the lane's columns is one more gap in each of them: counted
 * once per lane (`outside`), no load.  cls [256]: byte -> plane (0..3 residue, 4 otherwise), from hu_msa_encode_table. */
__global__ __launch_bounds__(HU_OTUCS_THREADS) void k_otucs_count(const unsigned char* __restrict__ stage, const HuOtucsRow* __restrict__ rows,
		const int32_t* __restrict__ order, const HuOtucsWork* __restrict__ work, const unsigned char* __restrict__ cls, int L,
		uint32_t* __restrict__ tab) {
	constexpr int CPL = HU_OTUCS_CPL;
	__shared__ unsigned char sCls[256];
	const int tid = threadIdx.x;
	sCls[tid] = cls[tid];
	__syncthreads();
	const HuOtucsWork w = work[blockIdx.x];
	const int col = blockIdx.y * HU_OTUCS_BLOCK_COLS + tid * CPL;
	if(col >= L) return;
	uint32_t cnt[5][CPL];
#pragma unroll
	for(int p = 0; p < 5; ++p)
#pragma unroll
		for(int k = 0; k < CPL; ++k) cnt[p][k] = 0;
	uint32_t outside = 0;
	for(int i = w.begin; i < w.end; ++i) {
		const HuOtucsRow r = rows[order[i]];
		if(col < r.c0 || col >= r.c1) { ++outside; continue; }
		uint32_t word[CPL / 4];
		const unsigned char* src = stage + (size_t) r.off16 * 16 + (col - r.c0);
		if constexpr(CPL == 16) { const uint4 v = *reinterpret_cast<const uint4*>(src); word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w; }
		else if constexpr(CPL == 8) { const uint2 v = *reinterpret_cast<const uint2*>(src); word[0] = v.x; word[1] = v.y; }
		else word[0] = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
		for(int k = 0; k < CPL; ++k) {
			const uint32_t c = sCls[(word[k >> 2] >> ((k & 3) * 8)) & 0xffu];
#pragma unroll
			for(int p = 0; p < 5; ++p) cnt[p][k] += c == (uint32_t) p;
		}
	}
	uint32_t* __restrict__ t = tab + (size_t) w.slot * 5 * L;
#pragma unroll
	for(int k = 0; k < CPL; ++k) {
		cnt[4][k] += outside;
#pragma unroll
		for(int p = 0; p < 5; ++p) if(col + k < L && cnt[p][k]) atomicAdd(&t[(size_t) p * L + col + k], cnt[p][k]);   /* past the row's end: staged padding, never counted */
	}
}

/* One lane per (OTU, column): grid (ceil(L / 256), n).  The prior is pri_i = e_i / sum e of the node's packed message: HuDbDev::up
 * holds it in linear space as eigen-coordinates a = U^-1 e (k_pack_msgs), so e = U a clamped at 0 (from_eig), and the site's common
 * factor 2^-k cancels in the quotient: no exp(), no upK.  The reference takes exp(M - max M) / sum (inferWeight,
 * src/PhyloTreeUnrooted.h:1590-1593): the same numbers in exact arithmetic.  Then, in the reference's order,
 * post = effN * pri + freq, post /= sum(post) — the division BEFORE the arg-max: it can round a strict order into a tie — and the
 * symbol is '-' when sum(freq) < gap, else ACGT[first maximum] (Eigen's maxCoeff keeps the lowest index of equal values).
 * The round trip through the eigenbasis leaves a few ulp on each e_i, so weights that are EQUAL in the log message (a subtree of gaps
 * under JC69: four equal weights; any symmetric pair) come back unequal, and the first-maximum rule would follow the noise.  Weights
 * closer than HU_OTUCS_SAME x the largest are therefore taken as the same number (the one of the lower index), well above the round
 * trip's error and far below any difference a model makes.
 * A message with no mass (every e_i = 0; the reference's 0 / 0) counts as no prior.  slot < 0: an OTU without counts. */
#define HU_OTUCS_SAME 0x1p-44
__global__ __launch_bounds__(256) void k_otucs_infer(HuDbDev db, HuModelDev mdl, const int32_t* __restrict__ nodes, const int32_t* __restrict__ slots,
		const uint32_t* __restrict__ tab, double effN, char* __restrict__ out) {
	const int j = blockIdx.x * 256 + threadIdx.x, o = blockIdx.y, L = db.csLen;
	if(j >= L) return;
	const int node = nodes[o], slot = slots[o];
	double a[4], e[4];
	load4(db.up + ((size_t) node * L + j) * 4, a);
	from_eig(mdl, a, e);
	const double same = fmax(fmax(e[0], e[1]), fmax(e[2], e[3])) * HU_OTUCS_SAME;
#pragma unroll
	for(int i = 1; i < 4; ++i)
#pragma unroll
		for(int k = i - 1; k >= 0; --k) if(fabs(e[i] - e[k]) <= same) e[i] = e[k];      /* ends on the lowest such index */
	uint32_t f[5] = {0, 0, 0, 0, 0};
	if(slot >= 0) {
		const uint32_t* __restrict__ t = tab + (size_t) slot * 5 * L + j;
#pragma unroll
		for(int p = 0; p < 5; ++p) f[p] = t[(size_t) p * L];
	}
	const double s = (e[0] + e[1]) + (e[2] + e[3]);
	double post[4];
#pragma unroll
	for(int i = 0; i < 4; ++i) post[i] = (s > 0 ? effN * (e[i] / s) : 0.0) + (double) f[i];
	const double tot = (post[0] + post[1]) + (post[2] + post[3]);
#pragma unroll
	for(int i = 0; i < 4; ++i) post[i] /= tot;
	int best = 0;
	double top = post[0];
#pragma unroll
	for(int i = 1; i < 4; ++i) if(post[i] > top) { top = post[i]; best = i; }
	const uint64_t nf = (uint64_t) f[0] + f[1] + f[2] + f[3];
	out[(size_t) o * L + j] = nf < (uint64_t) f[4] ? '-' : "ACGT"[best];
}
