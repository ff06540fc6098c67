// Build statistics on the device (two of the wide loops of hmmufotu-build around the tree sweep):
// the MSA column counts and sequence weights of MSA::prune / updateRawCounts / updateSeqWeight /
// updateWeightedCounts (src/MSA.cpp:87-138, 226-293), and the per-site mutation counts of
// PhyloTreeUnrooted::estimateNumMutations (src/PhyloTreeUnrooted.cpp:1008-1016) that the Gamma shape is
// estimated from.  The MSA is the loaded text, row-major [nSeq][csLen]; every residue is classified through
// one 256-entry table: encode(toupper(c)) of the MSA's alphabet, IUPACNucl (src/IUPACNucl.cpp:34-50,
// src/DegenAlphabet.cpp:51-63): A C G T -> 0..3, a degenerate letter -> the first base of its expansion,
// '-' '.' '_' -> -2 (gap), everything else -> -1.
#pragma once
#include "hu_common.h"

struct HuMsaDev {
	const char* msa;            /* [nSeq][csLen] */
	int64_t nSeq, csLen;
	const int8_t* enc;          /* [256] */
};

/* raw per-column residue / gap counts (MSA::updateRawCounts): integers, so the atomics' order is exact.
 * grid (csLen / 256, row chunks of rowsPer); res [4][csLen], gap [csLen] zeroed by the caller */
__global__ __launch_bounds__(256) void k_msa_col_counts(HuMsaDev m, int64_t rowsPer, int32_t* __restrict__ res, int32_t* __restrict__ gap) {
	__shared__ int8_t enc[256];
	enc[threadIdx.x] = m.enc[threadIdx.x];
	__syncthreads();
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= m.csLen) return;
	const int64_t i0 = (int64_t) blockIdx.y * rowsPer, i1 = min(m.nSeq, i0 + rowsPer);
	int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, cg = 0;     /* named, not an indexed array: no scratch */
	for(int64_t i = i0; i < i1; ++i) {
		const int8_t b = enc[(unsigned char) m.msa[i * m.csLen + j]];
		c0 += b == 0; c1 += b == 1; c2 += b == 2; c3 += b == 3; cg += b == -2;
	}
	if(c0) atomicAdd(&res[j], c0);
	if(c1) atomicAdd(&res[m.csLen + j], c1);
	if(c2) atomicAdd(&res[2 * m.csLen + j], c2);
	if(c3) atomicAdd(&res[3 * m.csLen + j], c3);
	if(cg) atomicAdd(&gap[j], cg);
}

/* per sequence (one lane each): first / last residue column, residue count, and the position-specific weight
 * sum_j 1 / pssw(b, j) in the reference's serial j order (MSA::updateSeqWeight, src/MSA.cpp:256-278), divided by
 * the residue count when it is not 0.  inv [4][csLen] = 1.0 / pssw, made on the host from the column counts. */
__global__ __launch_bounds__(64) void k_msa_seq_weight(HuMsaDev m, const double* __restrict__ inv, int32_t* __restrict__ start,
		int32_t* __restrict__ end, int32_t* __restrict__ len, double* __restrict__ w) {
	__shared__ int8_t enc[256];
	for(int c = threadIdx.x; c < 256; c += 64) enc[c] = m.enc[c];
	__syncthreads();
	const int64_t i = (int64_t) blockIdx.x * 64 + threadIdx.x;
	if(i >= m.nSeq) return;
	const char* row = m.msa + i * m.csLen;
	int32_t s = -1, e = -1, n = 0;
	double acc = 0;
	for(int64_t j = 0; j < m.csLen; ++j) {
		const int8_t b = enc[(unsigned char) row[j]];
		if(b >= 0) {
			if(s == -1) s = (int32_t) j;
			e = (int32_t) j;
			++n;
			acc += inv[b * m.csLen + j];
		}
	}
	if(n > 0) acc /= n;
	start[i] = s; end[i] = e; len[i] = n; w[i] = acc;
}

/* weighted counts (MSA::updateWeightedCounts, src/MSA.cpp:280-293): one lane per column, sequences added in i
 * order; 8 rows are loaded ahead of the serial additions to hide the load latency. */
__global__ __launch_bounds__(256) void k_msa_wcounts(HuMsaDev m, const double* __restrict__ w, double* __restrict__ res, double* __restrict__ gap) {
	__shared__ int8_t enc[256];
	enc[threadIdx.x] = m.enc[threadIdx.x];
	__syncthreads();
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= m.csLen) return;
	double c0 = 0, c1 = 0, c2 = 0, c3 = 0, cg = 0;
	constexpr int AHEAD = 8;
	for(int64_t i0 = 0; i0 < m.nSeq; i0 += AHEAD) {
		const int k = (int) min<int64_t>(AHEAD, m.nSeq - i0);
		unsigned char ch[AHEAD];
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) ch[t] = t < k ? (unsigned char) m.msa[(i0 + t) * m.csLen + j] : (unsigned char) 0;
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) if(t < k) {
			const int8_t b = enc[ch[t]];
			const double x = w[i0 + t];
			if(b == 0) c0 += x; else if(b == 1) c1 += x; else if(b == 2) c2 += x; else if(b == 3) c3 += x; else if(b == -2) cg += x;
		}
	}
	res[j] = c0; res[m.csLen + j] = c1; res[2 * m.csLen + j] = c2; res[3 * m.csLen + j] = c3;
	gap[j] = cg;
}

/* PTUnrooted::inferState of every node's own message (the branch node -> parent; the root's is its root message):
 * the first maximum of the 4 log-likelihoods, Eigen's maxCoeff.  up [n][csLen][4] as hu_tree_evaluate leaves it; a gap
 * leaf's message is log pi (src/PhyloTreeUnrooted.h:1431-1437), so its state is the first maximum of pi.  grid (csLen / 256, nodes) */
__global__ __launch_bounds__(256) void k_mut_state(const double* __restrict__ up, int64_t csLen, int8_t* __restrict__ st) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	const int64_t o = (int64_t) blockIdx.y * csLen + j;
	const double2* p = reinterpret_cast<const double2*>(up + o * 4);
	const double2 a = p[0], b = p[1];
	const double v[4] = {a.x, a.y, b.x, b.y};
	int s = 0;
	for(int k = 1; k < 4; ++k) if(v[k] > v[s]) s = k;
	st[o] = (int8_t) s;
}

/* per column: the non-root nodes whose state differs from their parent's (estimateNumMutations).
 * grid (csLen / 256, node chunks of nodesPer from node base); cnt [csLen] zeroed by the caller */
__global__ __launch_bounds__(256) void k_mut_count(const int8_t* __restrict__ st, const int32_t* __restrict__ parent, int32_t n, int64_t csLen,
		int32_t nodesPer, int32_t base, int32_t* __restrict__ cnt) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	const int32_t u0 = base + (int32_t) blockIdx.y * nodesPer, u1 = min(n, u0 + nodesPer);
	int32_t c = 0;
	for(int32_t u = u0; u < u1; ++u) {
		const int32_t p = parent[u];
		if(p >= 0 && st[(int64_t) u * csLen + j] != st[(int64_t) p * csLen + j]) ++c;
	}
	if(c) atomicAdd(&cnt[j], c);
}

/* PTUnrooted::treeLoglik(pi, X, j) = dot_product_scaled(pi, X.col(j)) (src/PhyloTreeUnrooted.h:1341-1343, :1505-1510) of the root
 * message: log(pi . exp(v + s)) - s, s = MIN_LOGLIK_EXP - max(v) when max(v) is finite and below MIN_LOGLIK_EXP, else 0.  One lane
 * per column, two 16-byte loads; the dot product in Eigen's association for a Vector4d, (p0 e0 + p2 e2) + (p1 e1 + p3 e3).
 * msg [csLen][4]: up[root] as hu_tree_evaluate leaves it.  The host adds the columns up in serial order. */
__global__ __launch_bounds__(256) void k_tree_loglik(const double* __restrict__ msg, int64_t csLen, double p0, double p1, double p2, double p3,
		double* __restrict__ out) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	const double2* p = reinterpret_cast<const double2*>(msg + j * 4);
	const double2 a = p[0], b = p[1];
	const double mx = fmax(fmax(a.x, a.y), fmax(b.x, b.y));
	const double sc = (mx != -INFINITY && mx < HU_MIN_LOGLIK_EXP) ? HU_MIN_LOGLIK_EXP - mx : 0.0;
	const double e0 = exp(a.x + sc), e1 = exp(a.y + sc), e2 = exp(b.x + sc), e3 = exp(b.y + sc);
	out[j] = log((p0 * e0 + p2 * e2) + (p1 * e1 + p3 * e3)) - sc;
}

/* The payloads of a run of consecutive directed edges of a .ptu, packed in file order (hu_ptu_write_stream): item e of the run is
 * the message down[c] (code = c << 1 | 1: the edge parent -> c) or up[c] (code = c << 1: the edge c -> parent, and the root row that
 * ends the file).  A message is `pieces` = 2 csLen pieces of 16 bytes; lane = one piece, one 16-byte load and one 16-byte store.
 * grid (pieces / 256, min(items, 65535)): a workgroup row walks the items with the grid's stride.
 * dst [items][pieces].  The host has checked every code against the node count. */
__global__ __launch_bounds__(256) void k_ptu_gather(const uint4* __restrict__ up, const uint4* __restrict__ down, const uint32_t* __restrict__ code,
		int64_t items, int64_t pieces, uint4* __restrict__ dst) {
	const int64_t q = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(q >= pieces) return;
	for(int64_t e = blockIdx.y; e < items; e += gridDim.y) {
		const uint32_t c = code[e];
		const uint4* src = (c & 1u) ? down : up;
		dst[e * pieces + q] = src[(int64_t)(c >> 1) * pieces + q];
	}
}
