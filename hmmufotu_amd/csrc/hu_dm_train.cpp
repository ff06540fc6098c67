// hmmufotu-train-dm on the device: the five training sets of src/hmmufotu-train-dm.cpp:253-333 (hu_dm_training_data
// launches k_dm_wcounts, k_hmm_states, k_dm_drop and k_dm_counts; the host scales the weights, decides the match columns and closes the
// non-zero columns up) and the optimiser of src/math/DirichletDensity.cpp:46-77 and src/math/DirichletMixture.cpp:92-146 for a batch
// of problems (hu_dm_train launches k_dm_train, `chunk` iterations at a time, until every problem has finished).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>
#include "hu_common.h"
namespace {     /* k_hmm_states is compiled into hu_hmm_train.cpp's object as well: this file's copies of the kernels are its own */
#include "hu_kern_dm.h"
}
static const auto unused_counts [[maybe_unused]] = &k_hmm_counts;     /* hu_hmm_train.cpp's; k_dm_counts stands in for it here */

static const int DM_MAX_CS = 65535;          /* as hu_hmm_counts: the profile these priors are for indexes its columns up to there */
static thread_local double g_dmTiming[4] = {0, 0, 0, 0};
static thread_local int64_t g_dmPeak = 0;

#define DCHK(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { hu_set_error("%s: %s failed: %s", fn, #call, hipGetErrorString(e_)); return HU_ERR_DEVICE; } } while(0)

extern "C" int hu_dm_training_data(int device, int64_t n_seq, int64_t cs_len, const char* msa, const double* weight, double pri_rate, double symfrac,
		uint8_t* mask, double* data_me, double* data_ie, double* data_mt, double* data_it, double* data_dt, int64_t* n_cols) try {
	const char* fn = "hu_dm_training_data";
	if(n_seq < 1 || cs_len < 1 || n_seq > INT32_MAX || !msa || !weight || !mask || !data_me || !data_ie || !data_mt || !data_it || !data_dt || !n_cols) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(cs_len > DM_MAX_CS) { hu_set_error("%s: %lld columns: the profile's index arrays end at %d", fn, (long long) cs_len, DM_MAX_CS); return HU_ERR_ARG; }
	if(!(pri_rate > 0 && pri_rate <= 1)) { hu_set_error("%s: pri_rate must be in (0, 1], %g given", fn, pri_rate); return HU_ERR_ARG; }
	if(!(symfrac >= 0 && symfrac <= 1)) { hu_set_error("%s: symfrac must between 0 and 1, %g given", fn, symfrac); return HU_ERR_ARG; }
	const int64_t N = n_seq, L = cs_len;
	/* MSA::sclaleWeight(effN / numSeq) with effN = 1 / priRate (src/hmmufotu-train-dm.cpp:236-237): the weights first, the counts from them */
	const double effN = 1 / pri_rate, r = effN / (double) N;
	std::vector<double> w((size_t) N);
	for(int64_t i = 0; i < N; ++i) {
		if(!(weight[i] >= 0) || !std::isfinite(weight[i])) { hu_set_error("%s: weight of row %lld is %g", fn, (long long) i, weight[i]); return HU_ERR_ARG; }
		w[(size_t) i] = weight[i] * r;
	}
	int8_t enc[256];
	hu_msa_encode_table(enc);
	if(hu_device_count() <= 0) { hu_set_error("no gfx950 device visible: the engine has no CPU path"); return HU_ERR_DEVICE; }
	DCHK(hipSetDevice(device));
	const size_t bytes = (size_t) N * L, outBytes = (size_t) L * HU_HMM_COL_VALUES * 8;
	char* dMsa = nullptr; uint8_t *dPlane = nullptr, *dMask = nullptr; int8_t* dEnc = nullptr; double *dW = nullptr, *dOut = nullptr, *dRes = nullptr, *dGap = nullptr; int32_t* dDrop = nullptr;
	HuScope guard([&] { (void) hipFree(dMsa); (void) hipFree(dPlane); (void) hipFree(dMask); (void) hipFree(dEnc); (void) hipFree(dW); (void) hipFree(dOut); (void) hipFree(dRes); (void) hipFree(dGap); (void) hipFree(dDrop); });
	size_t freeB = 0, totB = 0;
	DCHK(hipMemGetInfo(&freeB, &totB));
	{
		const size_t need = 2 * bytes + outBytes + (size_t) N * 12 + (size_t) L * 41 + 256 + 4096;
		if(need > freeB) { hu_set_error("%s: %lld rows x %lld columns (the text and one byte of state per cell) need %.3f GB of device memory, %.3f GB are free", fn, (long long) N, (long long) L, need / 1e9, freeB / 1e9); return HU_ERR_NOMEM; }
	}
	auto t0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	DCHK(hipMalloc((void**) &dMsa, bytes)); DCHK(hipMalloc((void**) &dPlane, bytes)); DCHK(hipMalloc((void**) &dMask, (size_t) L));
	DCHK(hipMalloc((void**) &dEnc, 256)); DCHK(hipMalloc((void**) &dW, (size_t) N * 8)); DCHK(hipMalloc((void**) &dOut, outBytes));
	DCHK(hipMalloc((void**) &dRes, (size_t) L * 32)); DCHK(hipMalloc((void**) &dGap, (size_t) L * 8)); DCHK(hipMalloc((void**) &dDrop, (size_t) N * 4));
	{
		size_t nowFree = 0;
		DCHK(hipMemGetInfo(&nowFree, &totB));
		g_dmPeak = (int64_t) freeB - (int64_t) nowFree;
	}
	DCHK(hipMemcpy(dMsa, msa, bytes, hipMemcpyHostToDevice)); DCHK(hipMemcpy(dEnc, enc, 256, hipMemcpyHostToDevice));
	DCHK(hipMemcpy(dW, w.data(), (size_t) N * 8, hipMemcpyHostToDevice));
	DCHK(hipDeviceSynchronize());
	g_dmTiming[0] = since();
	(void) hipGetLastError();
	/* the scaled weighted counts, and from them the match columns: symWFrac(j) >= symfrac (src/MSA.cpp:81-85; NaN: no) */
	const unsigned gx = (unsigned)((L + 255) / 256);
	k_dm_wcounts<<<gx, 256>>>(dMsa, N, L, dEnc, dW, dRes, dGap);
	DCHK(hipGetLastError());
	std::vector<double> res((size_t) L * 4), gap((size_t) L);
	DCHK(hipMemcpy(res.data(), dRes, (size_t) L * 32, hipMemcpyDeviceToHost)); DCHK(hipMemcpy(gap.data(), dGap, (size_t) L * 8, hipMemcpyDeviceToHost));
	for(int64_t j = 0; j < L; ++j) {
		const double numRes = (res[j] + res[2 * L + j]) + (res[L + j] + res[3 * L + j]);
		mask[j] = numRes / (numRes + gap[j]) >= symfrac;
	}
	DCHK(hipMemcpy(dMask, mask, (size_t) L, hipMemcpyHostToDevice));
	g_dmTiming[1] = since() - g_dmTiming[0];
	k_hmm_states<<<(unsigned)((N + 63) / 64), 64>>>(dMsa, N, L, dEnc, dMask, dPlane);
	DCHK(hipGetLastError());
	k_dm_drop<<<(unsigned)((N + 63) / 64), 64>>>(dPlane, N, L, dDrop);
	DCHK(hipGetLastError());
	DCHK(hipDeviceSynchronize());
	g_dmTiming[2] = since() - g_dmTiming[0] - g_dmTiming[1];
	k_dm_counts<<<gx, 256>>>(dPlane, N, L, dMask, dW, dDrop, dOut);
	DCHK(hipGetLastError());
	DCHK(hipDeviceSynchronize());
	g_dmTiming[3] = since() - g_dmTiming[0] - g_dmTiming[1] - g_dmTiming[2];
	std::vector<double> col((size_t) L * HU_HMM_COL_VALUES);
	DCHK(hipMemcpy(col.data(), dOut, outBytes, hipMemcpyDeviceToHost));
	/* the five sets (:265-333): the emissions of every column, the transitions of the columns j < L - 1 that have any */
	int64_t nME = 0, nIE = 0, nMT = 0, nIT = 0, nDT = 0;
	for(int64_t j = 0; j < L; ++j) {
		const double* c = col.data() + (size_t) j * HU_HMM_COL_VALUES;
		if(mask[j]) {
			memcpy(data_me + 4 * nME++, c, 32);
			if(c[4] != 0 || c[5] != 0 || c[6] != 0) { memcpy(data_mt + 3 * nMT++, c + 4, 24); }
			if(c[7] != 0 || c[8] != 0) { memcpy(data_dt + 2 * nDT++, c + 7, 16); }
		}
		else {
			memcpy(data_ie + 4 * nIE++, c, 32);
			if(c[4] != 0 || c[5] != 0) { memcpy(data_it + 2 * nIT++, c + 4, 16); }
		}
	}
	n_cols[0] = nME; n_cols[1] = nIE; n_cols[2] = nMT; n_cols[3] = nIT; n_cols[4] = nDT;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_training_data"); }

extern "C" int hu_dm_training_data_timing(double* seconds, int64_t* peak_bytes) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_dmTiming, sizeof(g_dmTiming));
	if(peak_bytes) *peak_bytes = g_dmPeak;
	return HU_OK;
}

extern "C" void hu_dm_default_opts(hu_dm_opts* o) {
	if(!o) return;
	/* eta: DirichletModel::DEFAULT_ETA (src/math/DirichletModel.cpp:15); the epsilons: BandedHMMP7Prior's (src/BandedHMMP7Prior.cpp:32-35) */
	o->eta = 0.001; o->abs_eps_cost = 0; o->rel_eps_cost = 1e-6; o->abs_eps_params = 0; o->rel_eps_params = 1e-4;
	o->max_iter = 0; o->chunk = 64;
}

extern "C" int hu_dm_train(int device, int32_t n, const hu_dm_problem* prob, const hu_dm_opts* opts, hu_dm_result* out, hu_dm_progress progress, void* user) try {
	const char* fn = "hu_dm_train";
	if(n < 1 || n > 4096 || !prob || !opts || !out) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(opts->chunk < 1 || opts->max_iter < 0 || !std::isfinite(opts->eta)) { hu_set_error("%s: chunk %d, max_iter %lld, eta %g", fn, opts->chunk, (long long) opts->max_iter, opts->eta); return HU_ERR_ARG; }
	std::vector<HuDmState> st((size_t) n);
	std::vector<int32_t> slot((size_t) n, -1);     /* the workgroup of a problem, -1: nothing to train */
	size_t dataDoubles = 0, scratchDoubles = 0;
	int32_t nDev = 0;
	for(int32_t p = 0; p < n; ++p) {
		const hu_dm_problem& P = prob[p];
		if(P.K < 2 || P.K > HU_DM_MAXK || P.L < 1 || P.L > HU_DM_MAXL || P.M < 0 || P.M > INT32_MAX || (P.M > 0 && !P.data) || !P.alpha0) { hu_set_error("%s: problem %d: K %d, L %d, M %lld", fn, p, P.K, P.L, (long long) P.M); return HU_ERR_ARG; }
		for(int64_t k = 0; k < P.M * P.K; ++k) if(!(P.data[k] >= 0) || !std::isfinite(P.data[k])) { hu_set_error("%s: problem %d: a count is %g", fn, p, P.data[k]); return HU_ERR_ARG; }
		HuDmState& s = st[(size_t) p];
		memset(&s, 0, sizeof(s));
		for(int k = 0; k < P.K * P.L; ++k) {
			if(!(P.alpha0[k] > 0)) { hu_set_error("%s: problem %d: a starting alpha is %g", fn, p, P.alpha0[k]); return HU_ERR_ARG; }
			s.alpha[k] = P.alpha0[k]; s.w[k] = log(P.alpha0[k]);     /* w = alpha.array().log() */
		}
		for(int j = 0; j < P.L; ++j) s.q[j] = P.q0 ? P.q0[j] : 1.0 / P.L;
		if(P.M == 0) { s.status = HU_DM_CONVERGED; continue; }     /* an empty set trains nothing: alpha as given, cost 0 */
		slot[(size_t) p] = nDev++;
		dataDoubles += (size_t) P.M * P.K; scratchDoubles += (size_t) P.M * (P.L + 1);
	}
	if(nDev > 0) {
		if(hu_device_count() <= 0) { hu_set_error("no gfx950 device visible: the engine has no CPU path"); return HU_ERR_DEVICE; }
		DCHK(hipSetDevice(device));
		double *dData = nullptr, *dScratch = nullptr; HuDmProblem* dProb = nullptr; HuDmState* dState = nullptr;
		HuScope guard([&] { (void) hipFree(dData); (void) hipFree(dScratch); (void) hipFree(dProb); (void) hipFree(dState); });
		DCHK(hipMalloc((void**) &dData, dataDoubles * 8)); DCHK(hipMalloc((void**) &dScratch, scratchDoubles * 8));
		DCHK(hipMalloc((void**) &dProb, (size_t) nDev * sizeof(HuDmProblem))); DCHK(hipMalloc((void**) &dState, (size_t) nDev * sizeof(HuDmState)));
		std::vector<HuDmProblem> hp((size_t) nDev); std::vector<HuDmState> hs((size_t) nDev);
		size_t atData = 0, atScratch = 0;
		for(int32_t p = 0; p < n; ++p) if(slot[(size_t) p] >= 0) {
			const hu_dm_problem& P = prob[p];
			HuDmProblem& d = hp[(size_t) slot[(size_t) p]];
			d.K = P.K; d.L = P.L; d.M = P.M; d.data = dData + atData; d.logp = dScratch + atScratch; d.lse = d.logp + (size_t) P.M * P.L;
			DCHK(hipMemcpy(dData + atData, P.data, (size_t) P.M * P.K * 8, hipMemcpyHostToDevice));
			atData += (size_t) P.M * P.K; atScratch += (size_t) P.M * (P.L + 1);
			hs[(size_t) slot[(size_t) p]] = st[(size_t) p];
		}
		DCHK(hipMemcpy(dProb, hp.data(), hp.size() * sizeof(HuDmProblem), hipMemcpyHostToDevice));
		DCHK(hipMemcpy(dState, hs.data(), hs.size() * sizeof(HuDmState), hipMemcpyHostToDevice));
		const HuDmOpts o{opts->eta, opts->abs_eps_cost, opts->rel_eps_cost, opts->abs_eps_params, opts->rel_eps_params, opts->max_iter, opts->chunk};
		(void) hipGetLastError();
		/* every launch is bounded by `chunk` iterations; the loop ends when no problem is running (max_iter 0: when all have stopped by themselves) */
		for(;;) {
			k_dm_train<<<(unsigned) nDev, HU_DM_WG>>>(dProb, dState, o);
			DCHK(hipGetLastError());
			DCHK(hipDeviceSynchronize());
			DCHK(hipMemcpy(hs.data(), dState, hs.size() * sizeof(HuDmState), hipMemcpyDeviceToHost));
			int32_t running = 0; int64_t most = 0;
			for(const HuDmState& s : hs) { running += s.status == HU_DM_RUNNING; most = std::max(most, s.iter); }
			if(progress) progress(user, most, running);
			if(running == 0) break;
		}
		for(int32_t p = 0; p < n; ++p) if(slot[(size_t) p] >= 0) st[(size_t) p] = hs[(size_t) slot[(size_t) p]];
	}
	for(int32_t p = 0; p < n; ++p) {
		const hu_dm_problem& P = prob[p];
		const HuDmState& s = st[(size_t) p];
		hu_dm_result& R = out[p];
		memset(&R, 0, sizeof(R));
		for(int i = 0; i < P.K; ++i) for(int j = 0; j < P.L; ++j) R.alpha[i][j] = s.alpha[i * P.L + j];
		for(int j = 0; j < P.L; ++j) R.q[j] = s.q[j];
		R.cost = s.cost; R.iterations = s.iter; R.status = s.status;
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_train"); }

extern "C" int hu_dm_special(int device, int64_t n, const double* x, double* lgamma_out, double* digamma_out) try {
	const char* fn = "hu_dm_special";
	if(n < 1 || n > (1 << 24) || !x || !lgamma_out || !digamma_out) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(hu_device_count() <= 0) { hu_set_error("no gfx950 device visible: the engine has no CPU path"); return HU_ERR_DEVICE; }
	DCHK(hipSetDevice(device));
	double *dX = nullptr, *dL = nullptr, *dG = nullptr;
	HuScope guard([&] { (void) hipFree(dX); (void) hipFree(dL); (void) hipFree(dG); });
	DCHK(hipMalloc((void**) &dX, (size_t) n * 8)); DCHK(hipMalloc((void**) &dL, (size_t) n * 8)); DCHK(hipMalloc((void**) &dG, (size_t) n * 8));
	DCHK(hipMemcpy(dX, x, (size_t) n * 8, hipMemcpyHostToDevice));
	(void) hipGetLastError();
	k_dm_special<<<(unsigned)((n + 255) / 256), 256>>>(dX, n, dL, dG);
	DCHK(hipGetLastError());
	DCHK(hipMemcpy(lgamma_out, dL, (size_t) n * 8, hipMemcpyDeviceToHost)); DCHK(hipMemcpy(digamma_out, dG, (size_t) n * 8, hipMemcpyDeviceToHost));
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_special"); }
