// hmmufotu-train-hmm without its files: the match columns (src/BandedHMMP7.cpp:405-411, :517-530) and, host only and
// to stay there, the effective sequence number and the probabilities (:479-494 with scale :248-257, estimateParams :280-315,
// meanRelativeEntropy :317-322, RelativeEntropyTargetFunc :1122-1135, src/math/RootFinder.cpp:22-76, the meanPostP of
// src/math/DirichletMixture.cpp:45-61 and src/math/DirichletDensity.cpp:25-27).  The counting loops (:424-477) run on the device
// (hu_hmm_counts launches hu_kern_hmm.h); the host adds the columns of one profile position up and the begin / end sums.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "hu_common.h"
#include "hu_kern_hmm.h"

static const int HMM_MAX_CS = 65535;         /* kMaxCS - 1, src/BandedHMMP7.h:279: index 1 .. 65,535 of the reference's arrays */
static const double HMM_CONS_THRESHOLD = 0.9; /* src/BandedHMMP7.cpp:54 */
static const double HMM_ERE = 1.0;           /* DEFAULT_ERE, src/BandedHMMP7.cpp:55 */

extern "C" int hu_hmm_match_columns(int64_t cs_len, int64_t n_seq, const double* res_wcount, const double* gap_wcount, double symfrac,
		uint8_t* mask, int32_t* K, int32_t* map, char* cons, double* identity) try {
	const char* fn = "hu_hmm_match_columns";
	if(cs_len < 1 || n_seq < 1 || !res_wcount || !gap_wcount || !mask || !K || !map || !cons || !identity) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(!(symfrac > 0 && symfrac < 1)) { hu_set_error("%s: symfrac must between 0 and 1, %g given", fn, symfrac); return HU_ERR_ARG; }
	if(cs_len > HMM_MAX_CS) { hu_set_error("%s: %lld columns: the profile's index arrays end at %d", fn, (long long) cs_len, HMM_MAX_CS); return HU_ERR_ARG; }
	const int64_t L = cs_len;
	int32_t k = 0;
	for(int64_t j = 0; j < L; ++j) {
		const double c[4] = {res_wcount[j], res_wcount[L + j], res_wcount[2 * L + j], res_wcount[3 * L + j]};
		const double numRes = (c[0] + c[2]) + (c[1] + c[3]), numGap = gap_wcount[j];
		mask[j] = numRes / (numRes + numGap) >= symfrac;     /* NaN: no */
		if(!mask[j]) continue;
		int mx = 0;
		for(int b = 1; b < 4; ++b) if(c[b] > c[mx]) mx = b;     /* maxCoeff: the first maximum */
		map[k] = (int32_t) j + 1;
		identity[k] = c[mx] / (double) n_seq;
		cons[k] = identity[k] < HMM_CONS_THRESHOLD ? "acgt"[mx] : "ACGT"[mx];
		++k;
	}
	*K = k;
	if(k == 0) { hu_set_error("%s: no column of %lld reaches the symbol fraction %g: the profile would have no position", fn, (long long) L, symfrac); return HU_ERR_ARG; }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_hmm_match_columns"); }

/* ------------------------------------------------------------------------------ the counts */
static thread_local double g_hmmTiming[4] = {0, 0, 0, 0};
static thread_local int64_t g_hmmPeak = 0;

extern "C" int hu_hmm_counts(int device, int64_t n_seq, int64_t cs_len, const char* msa, const double* weight, const int32_t* start, const int32_t* end,
		const uint8_t* mask, int32_t K, double* e_m, double* e_i, double* t) try {
	const char* fn = "hu_hmm_counts";
	if(n_seq < 1 || cs_len < 1 || n_seq > INT32_MAX || !msa || !weight || !start || !end || !mask || K < 1 || !e_m || !e_i || !t) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(cs_len > HMM_MAX_CS) { hu_set_error("%s: %lld columns: the profile's index arrays end at %d", fn, (long long) cs_len, HMM_MAX_CS); return HU_ERR_ARG; }
	const int64_t N = n_seq, L = cs_len;
	int8_t enc[256];
	hu_msa_encode_table(enc);
	std::vector<int32_t> cs2p((size_t) L);     /* cs2ProfileIdx: the match columns at or before j */
	{
		int32_t k = 0;
		for(int64_t j = 0; j < L; ++j) { k += mask[j] != 0; cs2p[(size_t) j] = k; }
		if(k != K) { hu_set_error("%s: the mask holds %d match columns, K is %d", fn, k, K); return HU_ERR_ARG; }
	}
	/* a row without a residue (start < 0; the reference would index column -1) adds nothing: its weight is taken as 0, and +0.0 changes no sum */
	std::vector<double> w((size_t) N);
	for(int64_t i = 0; i < N; ++i) {
		if(!(weight[i] >= 0) || !std::isfinite(weight[i])) { hu_set_error("%s: weight of row %lld is %g", fn, (long long) i, weight[i]); return HU_ERR_ARG; }
		const int32_t s = start[i], e = end[i];
		if(s < 0) { w[(size_t) i] = 0; continue; }
		if(s >= L || e < s || e >= L || enc[(unsigned char) msa[i * L + s]] < 0 || enc[(unsigned char) msa[i * L + e]] < 0) {
			hu_set_error("%s: row %lld: start %d and end %d are not two residues of its %lld columns", fn, (long long) i, s, e, (long long) L); return HU_ERR_ARG;
		}
		w[(size_t) i] = weight[i];
	}
	if(hu_device_count() <= 0) { hu_set_error("no gfx950 device visible: the engine has no CPU path"); return HU_ERR_DEVICE; }
	#define HCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)
	HCHK(hipSetDevice(device));
	const size_t bytes = (size_t) N * L, outBytes = (size_t) L * HU_HMM_COL_VALUES * 8;
	char* dMsa = nullptr; uint8_t *dPlane = nullptr, *dMask = nullptr; int8_t* dEnc = nullptr; double *dW = nullptr, *dOut = nullptr;
	HuScope guard([&] { (void) hipFree(dMsa); (void) hipFree(dPlane); (void) hipFree(dMask); (void) hipFree(dEnc); (void) hipFree(dW); (void) hipFree(dOut); });
	size_t freeB = 0, totB = 0;
	HCHK(hipMemGetInfo(&freeB, &totB));
	{
		const size_t need = 2 * bytes + outBytes + (size_t) N * 8 + (size_t) L + 256 + 1024;
		if(need > freeB) { hu_set_error("%s: %lld rows x %lld columns (the text and one byte of state per cell) need %.3f GB of device memory, %.3f GB are free", fn, (long long) N, (long long) L, need / 1e9, freeB / 1e9); return HU_ERR_NOMEM; }
	}
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	HCHK(hipMalloc((void**) &dMsa, bytes)); HCHK(hipMalloc((void**) &dPlane, bytes)); HCHK(hipMalloc((void**) &dMask, (size_t) L));
	HCHK(hipMalloc((void**) &dEnc, 256)); HCHK(hipMalloc((void**) &dW, (size_t) N * 8)); HCHK(hipMalloc((void**) &dOut, outBytes));
	{
		size_t nowFree = 0;
		HCHK(hipMemGetInfo(&nowFree, &totB));
		g_hmmPeak = (int64_t) freeB - (int64_t) nowFree;
	}
	HCHK(hipMemcpy(dMsa, msa, bytes, hipMemcpyHostToDevice)); HCHK(hipMemcpy(dMask, mask, (size_t) L, hipMemcpyHostToDevice));
	HCHK(hipMemcpy(dEnc, enc, 256, hipMemcpyHostToDevice)); HCHK(hipMemcpy(dW, w.data(), (size_t) N * 8, hipMemcpyHostToDevice));
	HCHK(hipDeviceSynchronize());
	g_hmmTiming[0] = since();
	(void) hipGetLastError();
	k_hmm_states<<<(unsigned)((N + 63) / 64), 64>>>(dMsa, N, L, dEnc, dMask, dPlane);
	HCHK(hipGetLastError());
	HCHK(hipDeviceSynchronize());
	g_hmmTiming[1] = since() - g_hmmTiming[0];
	k_hmm_counts<<<(unsigned)((L + 255) / 256), 256>>>(dPlane, N, L, dMask, dW, dOut);
	HCHK(hipGetLastError());
	HCHK(hipDeviceSynchronize());
	g_hmmTiming[2] = since() - g_hmmTiming[0] - g_hmmTiming[1];
	std::vector<double> col((size_t) L * HU_HMM_COL_VALUES);
	HCHK(hipMemcpy(col.data(), dOut, outBytes, hipMemcpyDeviceToHost));
	#undef HCHK
	/* the columns of one k, in ascending j.  What a match column gives (E_M(., k), T[k](M, .), T[k](D, .)) comes from that column alone */
	std::fill(e_m, e_m + (size_t)(K + 1) * 4, 0.0); std::fill(e_i, e_i + (size_t)(K + 1) * 4, 0.0); std::fill(t, t + (size_t)(K + 1) * 9, 0.0);
	for(int64_t j = 0; j < L; ++j) {
		const double* c = col.data() + (size_t) j * HU_HMM_COL_VALUES;
		const size_t k = (size_t) cs2p[(size_t) j];
		double* T = t + k * 9;
		if(mask[j]) {
			for(int b = 0; b < 4; ++b) { e_m[k * 4 + b] = c[b]; e_m[b] += c[b]; }
			T[3 * HU_HMM_M + HU_HMM_M] = c[4]; T[3 * HU_HMM_M + HU_HMM_I] = c[5]; T[3 * HU_HMM_M + HU_HMM_D] = c[6];
			T[3 * HU_HMM_D + HU_HMM_M] = c[7]; T[3 * HU_HMM_D + HU_HMM_D] = c[8];
		}
		else {
			for(int b = 0; b < 4; ++b) e_i[k * 4 + b] += c[b];
			T[3 * HU_HMM_I + HU_HMM_M] += c[4]; T[3 * HU_HMM_I + HU_HMM_I] += c[5];
		}
	}
	/* B->M1/I0 and MK/IK->E (:466-477), in ascending i */
	for(int64_t i = 0; i < N; ++i) if(start[i] >= 0) {
		const int sS = mask[start[i]] ? HU_HMM_M : HU_HMM_I, sE = mask[end[i]] ? HU_HMM_M : HU_HMM_I;
		t[3 * HU_HMM_M + sS] += w[(size_t) i];
		t[(size_t) K * 9 + 3 * sE + HU_HMM_M] += w[(size_t) i];
	}
	g_hmmTiming[3] = since() - g_hmmTiming[0] - g_hmmTiming[1] - g_hmmTiming[2];
	return HU_OK;
} catch(...) { return hu_catch_all("hu_hmm_counts"); }

extern "C" int hu_hmm_counts_timing(double* seconds, int64_t* peak_bytes) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_hmmTiming, sizeof(g_hmmTiming));
	if(peak_bytes) *peak_bytes = g_hmmPeak;
	return HU_OK;
}

/* ------------------------------------------------------------------------------ effN and the probabilities */
namespace {
inline double sum4(const double* x) { return (x[0] + x[2]) + (x[1] + x[3]); }
inline double sum3(const double* x) { return (x[0] + x[1]) + x[2]; }

/* DirichletDensity::meanPostP: (freq + alpha) / (freq.sum() + alpha.sum()) */
inline void density_post(int n, const double* alpha, double r, const double* cnt, double* out) {
	double f[4];
	for(int i = 0; i < n; ++i) f[i] = cnt[i] * r;
	const double fs = n == 4 ? sum4(f) : n == 3 ? sum3(f) : f[0] + f[1];
	const double as = n == 4 ? sum4(alpha) : n == 3 ? sum3(alpha) : alpha[0] + alpha[1];
	for(int i = 0; i < n; ++i) out[i] = (f[i] + alpha[i]) / (fs + as);
}

struct HmmEstimator {
	int32_t K; const double *em, *ei, *t; const hu_hmm_prior* pr;
	double lbAlpha[HU_HMM_MAX_MIX], alphaSum[HU_HMM_MAX_MIX];     /* lbeta(alpha.col(j)) and alpha.col(j).sum(): the same in every call */
	void init() {
		for(int j = 0; j < pr->me_L; ++j) {
			const double a[4] = {pr->me_alpha[0][j], pr->me_alpha[1][j], pr->me_alpha[2][j], pr->me_alpha[3][j]};
			alphaSum[j] = sum4(a);
			double s = 0;
			for(int i = 0; i < 4; ++i) s += lgamma(a[i]);
			lbAlpha[j] = s - lgamma(alphaSum[j]);
		}
	}
	/* DirichletMixture::meanPostP of the scaled counts */
	void mixture_post(double r, const double* cnt, double* out) const {
		const int L = pr->me_L;
		double d[4], logB[HU_HMM_MAX_MIX];
		for(int i = 0; i < 4; ++i) d[i] = cnt[i] * r;
		const double dataSum = sum4(d);
		double mx = -std::numeric_limits<double>::infinity();
		for(int j = 0; j < L; ++j) {
			double x[4], s = 0;
			for(int i = 0; i < 4; ++i) { x[i] = pr->me_alpha[i][j] + d[i]; s += lgamma(x[i]); }
			logB[j] = (s - lgamma(sum4(x))) - lbAlpha[j];
			mx = std::max(mx, logB[j]);
		}
		double X[4] = {0, 0, 0, 0};
		for(int j = 0; j < L; ++j) {
			const double wj = pr->me_q[j] * exp(logB[j] - mx);
			for(int i = 0; i < 4; ++i) X[i] += wj * (pr->me_alpha[i][j] + d[i]) / (alphaSum[j] + dataSum);
		}
		const double xs = sum4(X);
		for(int i = 0; i < 4; ++i) out[i] = X[i] / xs;
	}
	/* scale(r) and estimateParams; pm / pi / pt may be null for the entropy alone.  Returns meanRelativeEntropy against 0.25 */
	double estimate(double r, double* pm, double* pi, double* pt) const {
		const double nat2bit = 1.0 / log(2.0);
		double ent = 0;
		for(int32_t k = 0; k <= K; ++k) {
			double m[4];
			if(k > 0 || pm) mixture_post(r, em + (size_t) k * 4, m);
			if(k > 0) {
				double e = 0;
				for(int i = 0; i < 4; ++i) if(m[i] > 0) e += m[i] * log(m[i] / 0.25);
				ent += nat2bit * e;
			}
			if(!pm) continue;
			memcpy(pm + (size_t) k * 4, m, sizeof(m));
			density_post(4, pr->ie_alpha, r, ei + (size_t) k * 4, pi + (size_t) k * 4);
			const double* T = t + (size_t) k * 9;
			double* P = pt + (size_t) k * 9;
			density_post(3, pr->mt_alpha, r, T, P);
			density_post(2, pr->it_alpha, r, T + 3, P + 3);
			P[5] = T[5] * r;     /* I->D: scaled, never estimated */
			const double dt[2] = {T[6], T[8]};
			double dp[2];
			density_post(2, pr->dt_alpha, r, dt, dp);
			P[6] = dp[0]; P[7] = T[7] * r; P[8] = dp[1];
		}
		if(pt) { /* the enforced specials */
			pt[6] = 1; pt[8] = 0;
			double* P = pt + (size_t) K * 9;
			P[2] = 0; P[6] = 1; P[8] = 0;
		}
		return ent / K;
	}
};
}

extern "C" int hu_hmm_estimate(int32_t K, const double* e_m, const double* e_i, const double* t, int64_t n_seq, const hu_hmm_prior* prior,
		double* p_m, double* p_i, double* p_t, double* eff_n, int32_t* passes) try {
	const char* fn = "hu_hmm_estimate";
	if(K < 1 || !e_m || !e_i || !t || n_seq < 1 || !prior || !p_m || !p_i || !p_t || !eff_n) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(prior->me_L < 1 || prior->me_L > HU_HMM_MAX_MIX) { hu_set_error("%s: the prior's mixture has %d components", fn, prior->me_L); return HU_ERR_ARG; }
	for(size_t q = 0; q < (size_t)(K + 1) * 9; ++q) if(!(t[q] >= 0) || !std::isfinite(t[q])) { hu_set_error("%s: a transition count is %g", fn, t[q]); return HU_ERR_ARG; }
	for(size_t q = 0; q < (size_t)(K + 1) * 4; ++q) if(!(e_m[q] >= 0) || !std::isfinite(e_m[q]) || !(e_i[q] >= 0) || !std::isfinite(e_i[q])) { hu_set_error("%s: an emission count is negative or not finite", fn); return HU_ERR_ARG; }
	HmmEstimator est{K, e_m, e_i, t, prior, {0}, {0}};
	est.init();
	const double nSeq = (double) n_seq;
	auto f = [&](double x) { return est.estimate(x / nSeq, nullptr, nullptr, nullptr) - HMM_ERE; };
	/* RootFinder::rootBisection on [0, nSeq] */
	const double absEps = 1e-10, relEps = 1e-10;
	double xl = 0, xr = nSeq, x = std::numeric_limits<double>::quiet_NaN();
	double fxl = f(xl);
	const double fxr = f(xr);
	int32_t it = 0;
	if(!(fxl * fxr >= 0)) {
		for(;;) {
			++it;
			x = (xl + xr) / 2;
			const double fx = f(x);
			if(fx == 0) break;
			const double xmag = (xl < 0 && xr > 0) ? 0 : x;
			if(xr - xl < absEps + relEps * xmag) break;     /* resEps = 0: fabs(fx) < resEps never holds */
			if(fxl > 0 ? fx > 0 : fx < 0) { xl = x; fxl = fx; } else xr = x;
		}
	}
	const double effN = std::isnan(x) ? nSeq : x;
	est.estimate(effN / nSeq, p_m, p_i, p_t);
	*eff_n = effN;
	if(passes) *passes = it;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_hmm_estimate"); }
