// Test infrastructure: the host steps of hmmufotu-amd-train-dm (hu_dm_host.cpp: no HIP headers, no device code) built for the CPU
// with AddressSanitizer + UBSan; tests/test_train_dm.py compiles this file together with that source and hu_hmm_io.cpp and runs it
// stand-alone.  The writer is run on what the reader returns from a valid .dm file (the result must be that file byte for byte) and
// on models of every size; the shuffle and the moment fit on random sets of every shape the program can meet: empty, one column,
// fewer than 2 L columns, columns that sum to 0, a constant set, M that L does not divide.  Exit code 0 = every trial returned.
//
// usage: dm_train_driver <valid .dm file> <scratch path> <trials>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

/* what hu_host.cpp gives the library: the last error of the thread, and the exception barrier */
static char g_err[1024];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }

static std::string slurp(const char* p) {
	std::ifstream in(p, std::ios::binary);
	return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
	if(argc < 4) { fprintf(stderr, "usage: dm_train_driver <file.dm> <scratch> <trials>\n"); return 2; }
	const std::string good = slurp(argv[1]);
	const char* scratch = argv[2];
	const int trials = atoi(argv[3]);
	hu_hmm_prior pr;
	if(hu_hmm_prior_read(argv[1], &pr) != HU_OK) { fprintf(stderr, "the valid file was refused: %s\n", g_err); return 3; }
	{ /* the costs as the file has them */
		double cost[5]; int k = 0;
		for(size_t at = good.find("Training cost: "); at != std::string::npos && k < 5; at = good.find("Training cost: ", at + 1)) cost[k++] = atof(good.c_str() + at + 15);
		if(k != 5 || hu_dm_write(scratch, &pr, cost) != HU_OK) { fprintf(stderr, "writer: %s\n", g_err); return 3; }
		if(slurp(scratch) != good) { fprintf(stderr, "writer: the file did not come back byte for byte\n"); return 3; }
		if(hu_dm_write("/nonexistent-directory/x.dm", &pr, cost) == HU_OK) { fprintf(stderr, "writer: wrote into a missing directory\n"); return 3; }
	}
	std::mt19937_64 rng(777);
	std::uniform_real_distribution<double> uni(0.0, 1.0);
	int fitted = 0, kept = 0;
	for(int t = 0; t < trials; ++t) {
		const int K = 2 + (int)(rng() % 3), L = t % 3 == 0 ? 1 : 2 + (int)(rng() % 9);
		static const int64_t sizes[] = {0, 1, 2, 3, 4, 19, 20, 21, 63, 100, 257};
		const int64_t M = sizes[rng() % 11];
		std::vector<double> data((size_t) M * K + 1);
		const int how = (int)(rng() % 4);
		for(auto& v : data) v = how == 0 ? 3.0 : uni(rng) * 20;
		if(how == 1 && M > 0) for(int i = 0; i < K; ++i) data[(size_t)(rng() % M) * K + i] = 0;     /* a column that sums to 0 */
		std::vector<int32_t> idx((size_t) M + 1);
		uint32_t seed = (uint32_t) t;
		if(hu_dm_shuffle(M, t % 2 ? &seed : nullptr, idx.data()) != HU_OK) { fprintf(stderr, "shuffle: %s\n", g_err); return 4; }
		std::vector<char> seen((size_t) M + 1, 0);
		for(int64_t k = 0; k < M; ++k) { if(idx[k] < 0 || idx[k] >= M || seen[idx[k]]) { fprintf(stderr, "shuffle: not a permutation\n"); return 4; } seen[idx[k]] = 1; }
		std::vector<double> alpha((size_t) K * L);
		if(hu_dm_moment_init(K, L, M, data.data(), idx.data(), alpha.data()) != HU_OK) { fprintf(stderr, "moment fit: %s\n", g_err); return 4; }
		bool all1 = true;
		for(double a : alpha) all1 &= a == 1.0;
		all1 ? ++kept : ++fitted;
		if(M < (L == 1 ? 2 : 2 * L) && !all1) { fprintf(stderr, "moment fit: a set too small was fitted\n"); return 4; }
		/* a model of this size through the writer and the reader */
		hu_hmm_prior p = pr;
		p.me_L = L;
		for(int j = 0; j < L; ++j) { p.me_q[j] = 1.0 / L; for(int i = 0; i < 4; ++i) p.me_alpha[i][j] = std::exp(20 * uni(rng) - 10); }
		const double cost[5] = {uni(rng) * 1e4, 0, 1e-9, 1e12, NAN};
		if(hu_dm_write(scratch, &p, cost) != HU_OK) { fprintf(stderr, "writer: %s\n", g_err); return 4; }
		hu_hmm_prior back;
		g_err[0] = 0;
		if(hu_hmm_prior_read(scratch, &back) != HU_OK || back.me_L != L) { fprintf(stderr, "round trip: %s\n", g_err); return 4; }
		for(int j = 0; j < L; ++j) for(int i = 0; i < 4; ++i)     /* 16 digits were printed */
			if(std::fabs(back.me_alpha[i][j] - p.me_alpha[i][j]) > 1e-15 * p.me_alpha[i][j]) { fprintf(stderr, "round trip: alpha(%d, %d) %.17g came back as %.17g\n", i, j, p.me_alpha[i][j], back.me_alpha[i][j]); return 4; }
	}
	if(hu_dm_moment_init(4, 2, 8, nullptr, nullptr, nullptr) == HU_OK) { fprintf(stderr, "moment fit: null arguments accepted\n"); return 4; }
	remove(scratch);
	printf("dm train: %d trials, %d fitted, %d kept at 1; the valid file came back byte for byte\n", trials, fitted, kept);
	return 0;
}
