// Test infrastructure: the OTU table and the host path of hu_otu_subset (hu_otu_table.cpp: no HIP headers, no device code) built for
// the CPU with AddressSanitizer + UBSan; tests/test_otu_tools.py compiles this file together with that source and runs it stand-alone.
// The writer is run on what the reader returns from a valid table (the result must be that file byte for byte); the reader on damaged
// copies of it, which it may accept or refuse; then random tables of every shape the programs can meet (no OTU, no sample, empty
// samples, repeated ids) go through write, read, merge, prune, normalise and both subsampling methods.  Exit code 0 = every trial
// returned and every invariant held.
//
// usage: otu_table_driver <valid table> <scratch path> <trials>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>
#include "../../hmmufotu_amd/csrc/hu_otu_table.h"

/* what hu_host.cpp gives the library: the last error of the thread, and the exception barrier */
static char g_err[1024];
void hu_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
int hu_catch_all(const char* fn) noexcept { snprintf(g_err, sizeof(g_err), "%s: exception", fn); return HU_ERR_STATE; }

static std::string slurp(const char* p) {
	std::ifstream in(p, std::ios::binary);
	return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
#define FAIL(code, ...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (%s)\n", g_err); return code; } while(0)

int main(int argc, char** argv) {
	if(argc < 4) { fprintf(stderr, "usage: otu_table_driver <table> <scratch> <trials>\n"); return 2; }
	const std::string good = slurp(argv[1]);
	const char* scratch = argv[2];
	const int trials = atoi(argv[3]);
	{
		hu_otu_table* t = nullptr;
		if(hu_otu_table_read(argv[1], &t) != HU_OK) FAIL(3, "the valid table was refused");
		const size_t eol = good.find('\n'), at = good.find(" OTU table");
		const std::string info = good.substr(at, eol - at);
		if(hu_otu_table_write(t, scratch, info.c_str()) != HU_OK || slurp(scratch) != good) FAIL(3, "writer: the table did not come back byte for byte");
		if(hu_otu_table_write(t, "/nonexistent-directory/x.txt", "") == HU_OK) FAIL(3, "writer: wrote into a missing directory");
		if(hu_otu_table_merge(t, t) == HU_OK) FAIL(3, "merge: a table was added to itself");
		hu_otu_table_free(t);
		if(hu_otu_table_read("/nonexistent-directory/x.txt", &t) == HU_OK) FAIL(3, "reader: read a missing file");
	}
	std::mt19937_64 rng(4242);
	int refused = 0, subsampled = 0;
	for(int k = 0; k < trials; ++k) {
		/* a damaged copy: a truncation, a flipped byte, a tab or a line break dropped in */
		std::string bad = good;
		switch(k % 4) {
			case 0: bad.resize(rng() % (good.size() + 1)); break;
			case 1: bad[rng() % bad.size()] = (char)(rng() & 0xff); break;
			case 2: bad.insert(rng() % bad.size(), 1, '\t'); break;
			default: bad.insert(rng() % bad.size(), 1, '\n'); break;
		}
		{ std::ofstream o(scratch, std::ios::binary); o << bad; }
		hu_otu_table* d = nullptr;
		if(hu_otu_table_read(scratch, &d) != HU_OK) ++refused; else hu_otu_table_free(d);
		/* a random table */
		const int64_t M = (int64_t)(rng() % 7), S = (int64_t)(rng() % 6);
		std::vector<std::string> ids, taxa, names;
		for(int64_t i = 0; i < M; ++i) { ids.push_back(std::to_string(rng() % 9)); taxa.push_back(i % 2 ? "k__A; p__B c" : ""); }     /* ids repeat */
		for(int64_t j = 0; j < S; ++j) names.push_back("s" + std::to_string(j));
		std::vector<const char*> pi, pt, pn;
		for(auto& s : ids) pi.push_back(s.c_str());
		for(auto& s : taxa) pt.push_back(s.c_str());
		for(auto& s : names) pn.push_back(s.c_str());
		std::vector<double> cnt((size_t)(M * S) + 1);
		for(auto& v : cnt) v = rng() % 3 == 0 ? 0.0 : (double)(rng() % 400);
		if(S > 0 && k % 5 == 0) for(int64_t i = 0; i < M; ++i) cnt[(size_t)(i * S)] = 0;      /* an empty sample */
		hu_otu_table *a = nullptr, *b = nullptr;
		if(hu_otu_table_new(M, S, pi.data(), pt.data(), pn.data(), cnt.data(), &a) != HU_OK) FAIL(4, "new");
		if(hu_otu_table_write(a, scratch, " x") != HU_OK || hu_otu_table_read(scratch, &b) != HU_OK) FAIL(4, "round trip");
		int64_t m0 = 0, s0 = 0, m1 = 0, s1 = 0;
		hu_otu_table_dims(a, &m0, &s0); hu_otu_table_dims(b, &m1, &s1);
		if((m0 != m1 || s0 != s1 || (m0 * s0 > 0 && memcmp(hu_otu_table_counts(a), hu_otu_table_counts(b), (size_t)(m0 * s0) * 8) != 0))) FAIL(4, "round trip: %lld x %lld came back as %lld x %lld", (long long) m0, (long long) s0, (long long) m1, (long long) s1);
		/* the host subset of the table, both methods */
		const uint64_t size = 1 + rng() % 300;
		if(m0 > 0 && s0 > 0) for(int method = 0; method < 2; ++method) {
			std::vector<uint64_t> total; hu_otu_opts eff; hu_otu_opts o = {64, k % 3 == 0 ? 3 : 64};
			std::vector<double> out((size_t)(m0 * s0));
			const double* c = hu_otu_table_counts(a);
			if(hu_otu_subset_check("driver", m0, s0, c, size, method, &o, out.data(), &eff, total) != HU_OK) FAIL(5, "check");
			hu_otu_subset_host(m0, s0, c, total, size, method, (uint64_t) k, eff.key_bits, out.data());
			for(int64_t j = 0; j < s0; ++j) {
				uint64_t sum = 0;
				for(int64_t i = 0; i < m0; ++i) { const double v = out[(size_t)(i * s0 + j)]; sum += (uint64_t) v; if(method == 0 && v > c[i * s0 + j]) FAIL(5, "subset: more reads than the cell had"); }
				if(sum != (total[j] > size ? size : total[j])) FAIL(5, "subset: sample %lld has %llu reads of %llu, size %llu", (long long) j, (unsigned long long) sum, (unsigned long long) total[j], (unsigned long long) size);
			}
			++subsampled;
		}
		if(hu_otu_table_merge(b, a) != HU_OK) FAIL(6, "merge");
		int64_t zero = 0;
		if(hu_otu_table_prune_samples(b, size) != HU_OK || hu_otu_table_prune_otus(b) != HU_OK || hu_otu_table_normalize(b, (double)(k % 2 ? 1000 : 0), &zero) != HU_OK) FAIL(6, "prune / normalise");
		if(hu_otu_table_write(b, scratch, " y") != HU_OK) FAIL(6, "write");
		hu_otu_table_free(a); hu_otu_table_free(b);
	}
	{ /* refusals of the subset's checks */
		std::vector<uint64_t> total; hu_otu_opts eff; double c[2] = {1.5, 3}, out[2];
		if(hu_otu_subset_check("driver", 2, 1, c, 1, 0, nullptr, out, &eff, total) == HU_OK) FAIL(7, "a fraction was accepted");
		c[0] = 4294967295.0;
		if(hu_otu_subset_check("driver", 2, 1, c, 1, 0, nullptr, out, &eff, total) == HU_OK) FAIL(7, "a total of 2^32 + 2 was accepted");
	}
	remove(scratch);
	printf("otu table: %d trials, %d damaged copies refused, %d subsamples; the valid table came back byte for byte\n", trials, refused, subsampled);
	return 0;
}
