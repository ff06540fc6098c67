// Training the Dirichlet prior file on the device (hmmufotu-train-dm, src/hmmufotu-train-dm.cpp:253-370).
// The training data: k_hmm_states of hu_kern_hmm.h gives every cell its own state and the state of the nearest non-P cell to its
// right; k_dm_wcounts sums the scaled weights per column (MSA::updateWeightedCounts, src/MSA.cpp:280-293), k_dm_drop finds per row the
// one cell whose transition the reference's search loop drops, k_dm_counts adds the weights up per column as k_hmm_counts does.
// The optimiser: k_dm_train, one workgroup per problem (a Dirichlet density, L = 1, or a mixture of L components), gradient ascent on
// w = log alpha with the mixture's EM update of q (src/math/DirichletDensity.cpp:29-77, src/math/DirichletMixture.cpp:63-195), at
// most `chunk` iterations per launch.  FP64 throughout; every sum over the data columns is a serial chain per lane followed by a fixed
// tree in LDS, so a result depends on the inputs and HU_DM_WG alone.
#pragma once
#include "hu_common.h"
#include "hu_kern_hmm.h"

#define HU_DM_WG 256           /* lanes of a training workgroup: part of the result (the shape of the sums) */
#define HU_DM_MAXK 4
#define HU_DM_MAXL 10          /* MAX_NUM_COMPO, src/hmmufotu-train-dm.cpp:51 */
#define HU_DM_MAXP (HU_DM_MAXK * HU_DM_MAXL)

/* ------------------------------------------------------------------------------ the training data */
/* one lane per column, rows added in i order: res [4][csLen] and gap [csLen] of the weights w (k_msa_wcounts on the plain text) */
__global__ __launch_bounds__(256) void k_dm_wcounts(const char* __restrict__ msa, int64_t nSeq, int64_t csLen, const int8_t* __restrict__ encTab,
		const double* __restrict__ w, double* __restrict__ res, double* __restrict__ gap) {
	__shared__ int8_t enc[256];
	enc[threadIdx.x] = encTab[threadIdx.x];
	__syncthreads();
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	double c0 = 0, c1 = 0, c2 = 0, c3 = 0, cg = 0;
	for(int64_t i = 0; i < nSeq; ++i) {
		const int8_t b = enc[(unsigned char) msa[i * csLen + j]];
		const double x = w[i];
		if(b == 0) c0 += x; else if(b == 1) c1 += x; else if(b == 2) c2 += x; else if(b == 3) c3 += x; else if(b == -2) cg += x;
	}
	res[j] = c0; res[csLen + j] = c1; res[2 * csLen + j] = c2; res[3 * csLen + j] = c3;
	gap[j] = cg;
}

/* The reference's search for the next non-phantom cell (src/hmmufotu-train-dm.cpp:287-294) steps k past the cell it found before it
 * tests k >= L, so a next cell found in the last column is dropped like "none found".  One lane per row: drop[i] is the column of the
 * last non-P cell before column csLen - 1 when the last column's cell is not P, else -1 (that cell's next state is NONE already). */
__global__ __launch_bounds__(64) void k_dm_drop(const uint8_t* __restrict__ plane, int64_t nSeq, int64_t csLen, int32_t* __restrict__ drop) {
	const int64_t i = (int64_t) blockIdx.x * 64 + threadIdx.x;
	if(i >= nSeq) return;
	const uint8_t* row = plane + i * csLen;
	int32_t d = -1;
	if((row[csLen - 1] & 3u) != HU_HMM_NONE)
		for(int64_t j = csLen - 2; j >= 0; --j) if((row[j] & 3u) != HU_HMM_NONE) { d = (int32_t) j; break; }
	drop[i] = d;
}

/* k_hmm_counts with the rule above: out [csLen][9], 4 emissions, then M->M M->I M->D D->M D->D (match column) or I->M I->I (other
 * column).  Every sum is a serial chain over the rows in ascending i: the reference's sums bit for bit.  Named accumulators, plain
 * loads, adds and stores: no atomics, nothing across lanes. */
__global__ __launch_bounds__(256) void k_dm_counts(const uint8_t* __restrict__ plane, int64_t nSeq, int64_t csLen, const uint8_t* __restrict__ mask,
		const double* __restrict__ w, const int32_t* __restrict__ drop, double* __restrict__ out) {
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(j >= csLen) return;
	const unsigned emit = mask[j] != 0 ? HU_HMM_M : HU_HMM_I;
	double e0 = 0, e1 = 0, e2 = 0, e3 = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
	constexpr int AHEAD = 8;
	for(int64_t i0 = 0; i0 < nSeq; i0 += AHEAD) {
		const int k = (int) min<int64_t>(AHEAD, nSeq - i0);
		uint8_t c[AHEAD];
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) c[t] = t < k ? plane[(i0 + t) * csLen + j] : (uint8_t) HU_HMM_NONE;
		#pragma unroll
		for(int t = 0; t < AHEAD; ++t) if(t < k) {
			const unsigned own = c[t] & 3u, b = c[t] >> 4;
			if(own == HU_HMM_NONE) continue;
			const unsigned nxt = drop[i0 + t] == (int32_t) j ? (unsigned) HU_HMM_NONE : (c[t] >> 2) & 3u;
			const double x = w[i0 + t];
			if(own == emit) {
				if(b == 0) e0 += x; else if(b == 1) e1 += x; else if(b == 2) e2 += x; else e3 += x;
				if(nxt == HU_HMM_M) t0 += x;
				else if(nxt == HU_HMM_I) t1 += x;
				else if(nxt == HU_HMM_D && emit == HU_HMM_M) t2 += x;
			}
			else { /* D: only in a match column */
				if(nxt == HU_HMM_M) t3 += x; else if(nxt == HU_HMM_D) t4 += x;
			}
		}
	}
	double* o = out + j * HU_HMM_COL_VALUES;
	o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3; o[4] = t0; o[5] = t1; o[6] = t2; o[7] = t3; o[8] = t4;
}

/* ------------------------------------------------------------------------------ the optimiser */
#define HU_DM_RUNNING 0        /* the other states of a problem are the ABI's (include/hmmufotu_amd.h): HU_DM_CONVERGED, HU_DM_MAXIT, HU_DM_NAN_OVERFIT (an
                                * alpha underflowed to 0, src/math/DirichletMixture.cpp:116-119), HU_DM_NAN_UNUSED (a mixture coefficient below 1 / M,
                                * :120-124), HU_DM_NOT_FINITE (the cost is NaN or infinite: the reference would loop for ever) */

struct HuDmProblem {
	int32_t K, L; int64_t M;
	const double* data;        /* [M][K] */
	double* logp;              /* [L][M]: log P(column t | component j) at the current alpha */
	double* lse;               /* [M]: log sum_j q_j exp(logp_j) */
};
/* everything an unfinished problem carries from one launch to the next */
struct HuDmState { double alpha[HU_DM_MAXP], w[HU_DM_MAXP], q[HU_DM_MAXL], cost; int64_t iter; int32_t status, pad; };     /* alpha, w: [K][L] */
struct HuDmOpts { double eta, absEpsCost, relEpsCost, absEpsParams, relEpsParams; int64_t maxIter; int32_t chunk; };

/* digamma for x > 0 (the device library has none): psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the asymptotic series to x^-14,
 * whose first dropped term is 3617 / (8160 x^16) < 5e-17.  At most 10 steps, so x down to 1e-5 and below is as good as 1 / x is. */
__device__ inline double dm_digamma(double x) {
	double r = 0;
	for(int k = 0; k < 10 && x < 10.0; ++k) { r -= 1.0 / x; x += 1.0; }
	const double f = 1.0 / (x * x);
	const double s = f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
	return r + ((log(x) - 0.5 / x) - s);
}

/* test probe: the kernels' lgamma and digamma at n points */
__global__ __launch_bounds__(256) void k_dm_special(const double* __restrict__ x, int64_t n, double* __restrict__ lg, double* __restrict__ dg) {
	const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
	if(i >= n) return;
	lg[i] = lgamma(x[i]);
	dg[i] = dm_digamma(x[i]);
}

/* the sum of a vector of K entries in Eigen's association (hu_hmm_train.cpp: sum4, sum3) */
__device__ inline double dm_sumk(int K, double a, double b, double c, double d) { return K == 4 ? (a + c) + (b + d) : K == 3 ? (a + b) + c : a + b; }

/* sums of n <= 5 values over the workgroup: v[k] holds this lane's part and comes back as the total in every lane.  A fixed tree */
__device__ inline void dm_reduce(double (*red)[HU_DM_WG], int n, double* v) {
	const int tid = threadIdx.x;
	__syncthreads();
	for(int k = 0; k < n; ++k) red[k][tid] = v[k];
	__syncthreads();
	for(int s = HU_DM_WG / 2; s > 0; s >>= 1) {
		if(tid < s) for(int k = 0; k < n; ++k) red[k][tid] += red[k][tid + s];
		__syncthreads();
	}
	for(int k = 0; k < n; ++k) v[k] = red[k][0];
}

/* One workgroup per problem; a finished problem returns at once.  Per iteration (the order of trainML):
 *   gradient at (alpha, q) -> w += eta grad, alpha = exp(w) -> the two NaN exits -> cost at (alpha_new, q_old) -> q = mean_t compPostP
 *   at (alpha_new, q_old) -> the stop test.
 * logp is filled once per alpha and the cost, compPostP and the gradient are read from it; log sum_j q_j exp(logp_j) is taken
 * max-shifted, which is the reference's unshifted sum in exact arithmetic.  A launch begins by filling logp from the carried alpha
 * with the code that filled it in the launch before, so where a launch ends changes no bit of the result. */
__global__ __launch_bounds__(HU_DM_WG) void k_dm_train(const HuDmProblem* __restrict__ prob, HuDmState* __restrict__ state, HuDmOpts o) {
	const HuDmProblem P = prob[blockIdx.x];
	HuDmState* S = state + blockIdx.x;
	if(S->status != HU_DM_RUNNING) return;
	__shared__ double red[5][HU_DM_WG];
	__shared__ double sA[HU_DM_MAXP], sAOld[HU_DM_MAXP], sW[HU_DM_MAXP], sLgA[HU_DM_MAXP], sPsiA[HU_DM_MAXP], sGrad[HU_DM_MAXP];
	__shared__ double sQ[HU_DM_MAXL], sQNew[HU_DM_MAXL], sAsum[HU_DM_MAXL], sLgAsum[HU_DM_MAXL], sPsiAsum[HU_DM_MAXL];
	__shared__ double sCost;
	__shared__ int64_t sIter;
	__shared__ int sStatus;
	const int tid = threadIdx.x, K = P.K, L = P.L, KL = K * L;
	const int64_t M = P.M;
	if(tid < KL) { sA[tid] = S->alpha[tid]; sW[tid] = S->w[tid]; }
	if(tid < L) sQ[tid] = S->q[tid];
	if(tid == 0) { sCost = S->cost; sIter = S->iter; sStatus = HU_DM_RUNNING; }
	__syncthreads();
	auto column = [&](int64_t t, double& d0, double& d1, double& d2, double& d3) {
		const double* d = P.data + t * K;
		d0 = d[0]; d1 = d[1]; d2 = K > 2 ? d[2] : 0.0; d3 = K > 3 ? d[3] : 0.0;
	};
	/* lse[t] from logp and the current q */
	auto fill_lse = [&](int64_t t) -> double {
		double mx = P.logp[t];
		for(int j = 1; j < L; ++j) mx = fmax(mx, P.logp[(int64_t) j * M + t]);
		double s = 0;
		for(int j = 0; j < L; ++j) s += sQ[j] * exp(P.logp[(int64_t) j * M + t] - mx);
		const double l = mx + log(s);
		P.lse[t] = l;
		return l;
	};
	for(int step = 0; ; ++step) {
		/* ---- logp, the cost and the new q at the current alpha and q (DirichletMixture::compPostP, pdf; DirichletDensity::lpdf) */
		if(tid < L) {
			const double as = dm_sumk(K, sA[tid], sA[L + tid], K > 2 ? sA[2 * L + tid] : 0.0, K > 3 ? sA[3 * L + tid] : 0.0);
			sAsum[tid] = as; sLgAsum[tid] = lgamma(as);
		}
		if(tid < KL) sLgA[tid] = lgamma(sA[tid]);
		__syncthreads();
		double v[5];
		v[0] = 0;
		for(int64_t t = tid; t < M; t += HU_DM_WG) {
			double d0, d1, d2, d3;
			column(t, d0, d1, d2, d3);
			const double n = dm_sumk(K, d0, d1, d2, d3);
			const double lgN = lgamma(n + 1), l0 = lgamma(d0 + 1), l1 = lgamma(d1 + 1), l2 = K > 2 ? lgamma(d2 + 1) : 0.0, l3 = K > 3 ? lgamma(d3 + 1) : 0.0;
			for(int j = 0; j < L; ++j) {
				const double c = lgN + sLgAsum[j] - lgamma(n + sAsum[j]);
				double s = 0;
				s += lgamma(d0 + sA[j]) - l0 - sLgA[j];
				s += lgamma(d1 + sA[L + j]) - l1 - sLgA[L + j];
				if(K > 2) s += lgamma(d2 + sA[2 * L + j]) - l2 - sLgA[2 * L + j];
				if(K > 3) s += lgamma(d3 + sA[3 * L + j]) - l3 - sLgA[3 * L + j];
				P.logp[(int64_t) j * M + t] = c + s;
			}
			v[0] -= fill_lse(t);
		}
		dm_reduce(red, 1, v);
		const double c = v[0];
		for(int j = 0; j < L; ++j) {
			v[0] = 0;
			for(int64_t t = tid; t < M; t += HU_DM_WG) v[0] += sQ[j] * exp(P.logp[(int64_t) j * M + t] - P.lse[t]);
			dm_reduce(red, 1, v);
			if(tid == 0) sQNew[j] = v[0] / (double) M;
		}
		__syncthreads();
		if(tid == 0) {
			if(step == 0) { if(sIter == 0) sCost = c; }     /* the cost before the first iteration; later launches carry theirs */
			else {
				const double cOld = sCost, deltaC = cOld - c;
				for(int j = 0; j < L; ++j) sQ[j] = sQNew[j];
				/* Eigen's isApprox(alphaOld, prec): |a - b|^2 <= prec^2 min(|a|^2, |b|^2) */
				double d2 = 0, na = 0, nb = 0;
				for(int k = 0; k < KL; ++k) { const double e = sA[k] - sAOld[k]; d2 += e * e; na += sA[k] * sA[k]; nb += sAOld[k] * sAOld[k]; }
				const double prec = o.absEpsParams + o.relEpsParams * sqrt(nb);
				sCost = c;
				if(d2 <= prec * prec * fmin(na, nb) && deltaC >= 0 && deltaC < o.absEpsCost + o.relEpsCost * cOld) sStatus = HU_DM_CONVERGED;
				else if(!isfinite(c)) sStatus = HU_DM_NOT_FINITE;
				else if(o.maxIter > 0 && sIter >= o.maxIter) sStatus = HU_DM_MAXIT;
			}
		}
		__syncthreads();
		if(sStatus != HU_DM_RUNNING || step == o.chunk) break;
		/* ---- the gradient at (alpha, q) (weightGradient), with compPostP under the q just set */
		for(int64_t t = tid; t < M; t += HU_DM_WG) fill_lse(t);     /* also in a launch's first step, where q has not changed: one code path */
		if(tid < L) sPsiAsum[tid] = dm_digamma(sAsum[tid]);
		if(tid < KL) { sPsiA[tid] = dm_digamma(sA[tid]); sAOld[tid] = sA[tid]; }
		for(int j = 0; j < L; ++j) {
			const double a0 = sA[j], a1 = sA[L + j], a2 = K > 2 ? sA[2 * L + j] : 0.0, a3 = K > 3 ? sA[3 * L + j] : 0.0, as = sAsum[j], qj = sQ[j];
			v[0] = v[1] = v[2] = v[3] = v[4] = 0;
			for(int64_t t = tid; t < M; t += HU_DM_WG) {
				double d0, d1, d2, d3;
				column(t, d0, d1, d2, d3);
				const double p = qj * exp(P.logp[(int64_t) j * M + t] - P.lse[t]);
				const double pn = dm_digamma(dm_sumk(K, d0, d1, d2, d3) + as);
				v[0] += p * (dm_digamma(d0 + a0) - pn);
				v[1] += p * (dm_digamma(d1 + a1) - pn);
				if(K > 2) v[2] += p * (dm_digamma(d2 + a2) - pn);
				if(K > 3) v[3] += p * (dm_digamma(d3 + a3) - pn);
				v[4] += p;
			}
			dm_reduce(red, 5, v);
			if(tid == 0) {
				sGrad[j] = a0 * (v[4] * (sPsiAsum[j] - sPsiA[j]) + v[0]);
				sGrad[L + j] = a1 * (v[4] * (sPsiAsum[j] - sPsiA[L + j]) + v[1]);
				if(K > 2) sGrad[2 * L + j] = a2 * (v[4] * (sPsiAsum[j] - sPsiA[2 * L + j]) + v[2]);
				if(K > 3) sGrad[3 * L + j] = a3 * (v[4] * (sPsiAsum[j] - sPsiA[3 * L + j]) + v[3]);
			}
		}
		__syncthreads();
		if(tid < KL) { sW[tid] += o.eta * sGrad[tid]; sA[tid] = exp(sW[tid]); }
		__syncthreads();
		if(tid == 0) {
			sIter += 1;
			bool zero = false;
			for(int k = 0; k < KL; ++k) zero |= sA[k] == 0;
			double qmin = sQ[0];
			for(int j = 1; j < L; ++j) qmin = fmin(qmin, sQ[j]);
			if(zero) sStatus = HU_DM_NAN_OVERFIT;
			else if(L > 1 && qmin < 1.0 / (double) M) sStatus = HU_DM_NAN_UNUSED;
			if(sStatus != HU_DM_RUNNING) sCost = nan("");
		}
		__syncthreads();
		if(sStatus != HU_DM_RUNNING) break;
	}
	if(tid < KL) { S->alpha[tid] = sA[tid]; S->w[tid] = sW[tid]; }
	if(tid < L) S->q[tid] = sQ[tid];
	if(tid == 0) { S->cost = sCost; S->iter = sIter; S->status = sStatus; }
}
