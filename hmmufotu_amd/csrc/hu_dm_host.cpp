// hmmufotu-train-dm's host steps, free of HIP headers so that a plain C++ compiler builds this file for the sanitizer
// run of tests/san/dm_train_driver.cpp: the shuffle and the moment fit that start a training (DirichletDensity::momentInit,
// src/math/DirichletDensity.cpp:105-133; DirichletMixture::momentInit, src/math/DirichletMixture.cpp:208-252) and the writer of the
// prior file (operator<< of BandedHMMP7Prior, src/BandedHMMP7Prior.cpp:62-69, with the print of DirichletMixture.cpp:197-206 and of
// DirichletDensity.cpp:96-103).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

/* std::random_shuffle of libstdc++ (bits/stl_algo.h) on 0 .. M - 1, on the C library's rand() as the reference's is */
extern "C" int hu_dm_shuffle(int64_t M, const uint32_t* seed, int32_t* idx) try {
	if(M < 0 || M > INT32_MAX || (M > 0 && !idx)) { hu_set_error("hu_dm_shuffle: bad argument"); return HU_ERR_ARG; }
	if(seed) srand(*seed);
	for(int64_t t = 0; t < M; ++t) idx[t] = (int32_t) t;
	for(int64_t i = 1; i < M; ++i) {
		const int64_t j = rand() % (i + 1);
		if(i != j) { const int32_t x = idx[i]; idx[i] = idx[j]; idx[j] = x; }
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_shuffle"); }

namespace {
/* mean and variance of rows of `cols` normalised columns, and the first i whose alphaNorm is positive; false: none (alpha untouched) */
bool moment_fit(int K, const std::vector<double>& x /* [cols][K] */, size_t from, size_t cols, double N, double* alpha, int stride) {
	double mean[4], var[4];
	for(int i = 0; i < K; ++i) {
		double s = 0;
		for(size_t t = 0; t < cols; ++t) s += x[(from + t) * K + i];
		mean[i] = s / (double) cols;
		double v = 0;
		for(size_t t = 0; t < cols; ++t) { const double e = x[(from + t) * K + i] - mean[i]; v += e * e; }
		var[i] = v / (double) cols;
	}
	double alphaNorm = 0;
	for(int i = 0; i < K; ++i) {
		alphaNorm = (var[i] - N * mean[i] + 1) / (mean[i] - 1 / N - var[i]);
		if(alphaNorm > 0) break;
	}
	if(alphaNorm <= 0) return false;     /* a NaN goes on, as in the reference */
	for(int i = 0; i < K; ++i) alpha[i * stride] = mean[i] * alphaNorm / N;
	return true;
}
inline double sum_k(int K, const double* d) { return K == 4 ? (d[0] + d[2]) + (d[1] + d[3]) : K == 3 ? (d[0] + d[1]) + d[2] : d[0] + d[1]; }
}

extern "C" int hu_dm_moment_init(int32_t K, int32_t L, int64_t M, const double* data, const int32_t* idx, double* alpha) try {
	const char* fn = "hu_dm_moment_init";
	if(K < 2 || K > 4 || L < 1 || L > 10 || M < 0 || (M > 0 && !data) || !alpha || (L > 1 && M > 0 && !idx)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	for(int k = 0; k < K * L; ++k) alpha[k] = 1;     /* DEFAULT_ALPHA: what a fit that fails leaves */
	if(L == 1 ? M < 2 : M < 2 * (int64_t) L) return HU_OK;     /* too few columns to estimate from */
	std::vector<double> x((size_t) M * K);
	for(int64_t t = 0; t < M; ++t) {
		const int64_t src = L == 1 ? t : idx[t];
		if(src < 0 || src >= M) { hu_set_error("%s: idx[%lld] is %lld of %lld", fn, (long long) t, (long long) src, (long long) M); return HU_ERR_ARG; }
		memcpy(&x[(size_t) t * K], data + src * K, (size_t) K * 8);
	}
	/* every column scaled to the largest column sum */
	double N = sum_k(K, &x[0]);
	for(int64_t t = 1; t < M; ++t) { const double s = sum_k(K, &x[(size_t) t * K]); if(s > N) N = s; }
	for(int64_t t = 0; t < M; ++t) { const double f = N / sum_k(K, &x[(size_t) t * K]); for(int i = 0; i < K; ++i) x[(size_t) t * K + i] *= f; }
	if(L == 1) { moment_fit(K, x, 0, (size_t) M, N, alpha, 1); return HU_OK; }
	for(int j = 0; j < L; ++j) moment_fit(K, x, (size_t)((int64_t) j * M / L), (size_t)(M / L), N, alpha + j, L);     /* block j: M / L columns from j M / L */
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_moment_init"); }

namespace {
/* Eigen's operator<< under IOFormat(FullPrecision): 16 significant digits, every entry right-aligned to the widest of its matrix */
std::string eigen_full(const double* a, int rows, int cols, int stride) {
	std::vector<std::string> s((size_t) rows * cols);
	size_t width = 0;
	char t[64];
	for(int i = 0; i < rows; ++i) for(int j = 0; j < cols; ++j) {
		snprintf(t, sizeof(t), "%.16g", a[i * stride + j]);
		s[(size_t) i * cols + j] = t;
		if(s[(size_t) i * cols + j].size() > width) width = s[(size_t) i * cols + j].size();
	}
	std::string o;
	for(int i = 0; i < rows; ++i) {
		for(int j = 0; j < cols; ++j) { const std::string& e = s[(size_t) i * cols + j]; if(j) o += ' '; o.append(width - e.size(), ' '); o += e; }
		o += '\n';
	}
	return o;
}
std::string cost_line(double c) { char t[64]; snprintf(t, sizeof(t), "Training cost: %g\n", c); return t; }
}

extern "C" int hu_dm_write(const char* path, const hu_hmm_prior* p, const double* cost) try {
	const char* fn = "hu_dm_write";
	if(!path || !p || !cost || p->me_L < 1 || p->me_L > HU_HMM_MAX_MIX) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	std::string o = "Match emission:\nDirichlet Mixture Model\n" + cost_line(cost[0]) + "K: 4 L: " + std::to_string(p->me_L) + "\nMixture coefficients:\n";
	o += eigen_full(p->me_q, 1, p->me_L, 0) + "alpha:\n" + eigen_full(&p->me_alpha[0][0], 4, p->me_L, HU_HMM_MAX_MIX);
	static const char* heads[4] = {"Insert emission:", "Match transition:", "Insert transition:", "Delete transition:"};
	const double* alpha[4] = {p->ie_alpha, p->mt_alpha, p->it_alpha, p->dt_alpha};
	static const int dims[4] = {4, 3, 2, 2};
	for(int b = 0; b < 4; ++b)
		o += std::string(heads[b]) + "\nDirichlet Density Model\n" + cost_line(cost[b + 1]) + "K: " + std::to_string(dims[b]) + "\nalpha:\n" + eigen_full(alpha[b], 1, dims[b], 0);
	if(strcmp(path, "-") == 0) {
		if(fwrite(o.data(), 1, o.size(), stdout) != o.size() || fflush(stdout) != 0) { hu_set_error("%s: unable to write to the standard output", fn); return HU_ERR_IO; }
		return HU_OK;
	}
	std::ofstream f(path, std::ios::binary | std::ios::trunc);
	if(!f.is_open()) { hu_set_error("%s: unable to write to '%s'", fn, path); return HU_ERR_IO; }
	f.write(o.data(), (std::streamsize) o.size());
	f.flush();
	if(!f) { hu_set_error("%s: unable to write '%s'", fn, path); return HU_ERR_IO; }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_dm_write"); }
