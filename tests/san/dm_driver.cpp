// Test infrastructure: the prior-file reader and the profile writer of hmmufotu-amd-train-hmm (hu_hmm_io.cpp: no HIP headers, no
// device code) built for the CPU with AddressSanitizer + UBSan; tests/test_train_hmm.py compiles this file together with that source
// and runs it stand-alone.  The reader is fed a valid .dm file and damaged copies of it: truncations, byte flips, lines dropped or
// doubled, and dimensions overwritten with large, zero or negative values.  A reader may accept or refuse a damaged file; it may not
// touch memory it does not own or overflow (the sanitizer aborts on those).  The writer is run on what the reader returned, with
// probabilities of 0 and 1 among them.  Exit code 0 = every trial returned.
//
// usage: dm_driver <valid .dm file> <scratch path> <trials>
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
static void spit(const char* p, const std::string& v) {
	std::ofstream out(p, std::ios::binary | std::ios::trunc);
	out.write(v.data(), (std::streamsize) v.size());
}
static std::vector<std::string> lines_of(const std::string& s) {
	std::vector<std::string> v; size_t a = 0;
	while(a < s.size()) { size_t b = s.find('\n', a); if(b == std::string::npos) b = s.size(); v.push_back(s.substr(a, b - a)); a = b + 1; }
	return v;
}
static std::string join(const std::vector<std::string>& v) { std::string s; for(const auto& l : v) { s += l; s += '\n'; } return s; }

int main(int argc, char** argv) {
	if(argc < 4) { fprintf(stderr, "usage: dm_driver <file.dm> <scratch> <trials>\n"); return 2; }
	const std::string good = slurp(argv[1]);
	const char* scratch = argv[2];
	const int trials = atoi(argv[3]);
	if(good.empty()) { fprintf(stderr, "empty input\n"); return 2; }
	hu_hmm_prior pr;
	if(hu_hmm_prior_read(argv[1], &pr) != HU_OK) { fprintf(stderr, "the undamaged file was refused: %s\n", g_err); return 3; }
	if(pr.me_L < 1 || pr.me_L > HU_HMM_MAX_MIX) { fprintf(stderr, "L = %d\n", pr.me_L); return 3; }
	{ /* the writer, on a profile of 3 positions made of the prior's own numbers, with the specials 0 and 1 */
		const int K = 3;
		std::vector<double> pm(4 * (K + 1)), pi(4 * (K + 1)), pt(9 * (K + 1), 0.0);
		for(int k = 0; k <= K; ++k) for(int b = 0; b < 4; ++b) { pm[4 * k + b] = pr.me_alpha[b][k % pr.me_L] / 1000.0; pi[4 * k + b] = pr.ie_alpha[b] / 4.0; }
		for(int k = 0; k <= K; ++k) { for(int q = 0; q < 3; ++q) pt[9 * k + q] = pr.mt_alpha[q] / 100.0; pt[9 * k + 3] = pr.it_alpha[0]; pt[9 * k + 4] = pr.it_alpha[1]; pt[9 * k + 6] = 1.0; }
		pm[5] = 0.0;
		const int32_t map[3] = {1, 4, 9};
		const std::string out = std::string(scratch) + ".hmm";
		if(hu_hmm_write(out.c_str(), "dm_driver", "a name with blanks", K, 9, pm.data(), pi.data(), pt.data(), map, "AcG", 7, 3.25, "some date") != HU_OK) { fprintf(stderr, "writer: %s\n", g_err); return 3; }
		const std::string text = slurp(out.c_str());
		if(text.find("\n//\n") == std::string::npos || text.find("*") == std::string::npos || text.find("inf") == std::string::npos) { fprintf(stderr, "writer: unexpected text\n"); return 3; }
		if(hu_hmm_write("/nonexistent-directory/x.hmm", "v", "n", K, 9, pm.data(), pi.data(), pt.data(), map, "AcG", 7, 3.25, "d") == HU_OK) { fprintf(stderr, "writer: wrote into a missing directory\n"); return 3; }
		remove(out.c_str());
	}
	std::mt19937_64 rng(4242);
	static const char* junk[] = {"99999999", "-3", "0", "2147483647", "1e999", "nan", "x", "", "4294967296", "33"};
	int accepted = 0, refused = 0;
	for(int t = 0; t < trials; ++t) {
		std::string v = good;
		std::vector<std::string> ln = lines_of(good);
		const int how = t % 5;
		if(how == 0) v.resize(rng() % v.size());                                                        /* truncate */
		else if(how == 1) { const int k = 1 + (int)(rng() % 6); for(int i = 0; i < k; ++i) v[rng() % v.size()] ^= (char)(1 + rng() % 255); }     /* flip bytes */
		else if(how == 2) { ln.erase(ln.begin() + (long)(rng() % ln.size())); v = join(ln); }            /* drop a line */
		else if(how == 3) { const size_t at = rng() % ln.size(); ln.insert(ln.begin() + (long) at, ln[rng() % ln.size()]); v = join(ln); }     /* double a line elsewhere */
		else { /* overwrite the number after a "K:" or "L:" or any number on a random line */
			std::string& l = ln[rng() % ln.size()];
			size_t at = l.find(rng() % 2 ? "L: " : "K: ");
			at = at == std::string::npos ? l.find_first_of("0123456789") : at + 3;
			if(at != std::string::npos) { size_t e = l.find_first_of(" \t", at); l.replace(at, e == std::string::npos ? std::string::npos : e - at, junk[rng() % 10]); }
			v = join(ln);
		}
		spit(scratch, v);
		hu_hmm_prior p;
		if(hu_hmm_prior_read(scratch, &p) == HU_OK) {
			if(p.me_L < 1 || p.me_L > HU_HMM_MAX_MIX) { fprintf(stderr, "accepted a file with L = %d\n", p.me_L); return 4; }
			accepted++;
		}
		else refused++;
	}
	remove(scratch);
	printf("dm: %d trials, %d accepted, %d refused\n", trials, accepted, refused);
	return 0;
}
