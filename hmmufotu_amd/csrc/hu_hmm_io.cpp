// hmmufotu-train-hmm's two files, host only and free of HIP headers, so that a plain C++ compiler builds this file
// for the sanitizer run of tests/san/dm_driver.cpp: the reader of the prior file (.dm; operator>> of BandedHMMP7Prior,
// src/BandedHMMP7Prior.cpp:39-62, with the read() of src/math/DirichletMixture.cpp:254-285 and src/math/DirichletDensity.cpp:135-162)
// and the writer of the profile (operator<< of BandedHMMP7, src/BandedHMMP7.cpp:324-378).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

namespace {
struct DmLines {
	std::vector<std::string> line; size_t at = 0;
	bool more() const { return at < line.size(); }
};
bool starts_with(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

/* `want` numbers from the lines that follow, whole lines only; why: what is wrong when false */
bool dm_numbers(DmLines& in, size_t want, double* out, std::string& why) {
	size_t got = 0;
	while(got < want) {
		if(!in.more()) { why = "the file ends after " + std::to_string(got) + " of " + std::to_string(want) + " numbers"; return false; }
		const std::string& s = in.line[in.at++];
		const char* p = s.c_str();
		for(;;) {
			while(*p == ' ' || *p == '\t' || *p == '\r') ++p;
			if(!*p) break;
			char* e = nullptr;
			const double v = strtod(p, &e);
			if(e == p || !(*e == 0 || *e == ' ' || *e == '\t' || *e == '\r') || !std::isfinite(v)) { why = "'" + std::string(p, strcspn(p, " \t\r")) + "' is not a finite number"; return false; }
			if(got == want) { why = "more than " + std::to_string(want) + " numbers"; return false; }
			out[got++] = v;
			p = e;
		}
	}
	return true;
}
bool dm_label(DmLines& in, const char* label, std::string& why) {
	if(!in.more() || !starts_with(in.line[in.at], label)) { why = std::string("the line '") + label + "' is missing"; return false; }
	++in.at;
	return true;
}
/* the lines of one model after its head line: a mixture of L components over wantK values, or a density of wantK values */
bool dm_model(DmLines& in, bool mixture, int wantK, int32_t* L, double* q, double* alpha, std::string& why) {
	if(!dm_label(in, mixture ? "Dirichlet Mixture Model" : "Dirichlet Density Model", why)) return false;
	if(!dm_label(in, "Training cost:", why)) return false;
	if(!in.more()) { why = "the line 'K:' is missing"; return false; }
	int K = 0, l = 0;
	const std::string& dims = in.line[in.at];
	if(mixture ? sscanf(dims.c_str(), "K: %d L: %d", &K, &l) != 2 : sscanf(dims.c_str(), "K: %d", &K) != 1) { why = mixture ? "the line 'K: .. L: ..' is missing" : "the line 'K: ..' is missing"; return false; }
	++in.at;
	if(K != wantK) { why = "K is " + std::to_string(K) + ", " + std::to_string(wantK) + " expected"; return false; }
	if(mixture) {
		if(l < 1 || l > HU_HMM_MAX_MIX) { why = "L is " + std::to_string(l) + ", 1 .. " + std::to_string(HU_HMM_MAX_MIX) + " expected"; return false; }
		*L = l;
		if(!dm_label(in, "Mixture coefficients:", why) || !dm_numbers(in, (size_t) l, q, why)) return false;
		for(int j = 0; j < l; ++j) if(q[j] < 0) { why = "a negative mixture coefficient"; return false; }
	}
	if(!dm_label(in, "alpha:", why)) return false;
	std::vector<double> a((size_t) K * (mixture ? l : 1));
	if(!dm_numbers(in, a.size(), a.data(), why)) return false;
	for(double v : a) if(!(v > 0)) { why = "an alpha that is not positive"; return false; }
	if(mixture) { for(int i = 0; i < K; ++i) for(int j = 0; j < l; ++j) alpha[i * HU_HMM_MAX_MIX + j] = a[(size_t) i * l + j]; }
	else memcpy(alpha, a.data(), a.size() * sizeof(double));
	return true;
}
}

extern "C" int hu_hmm_prior_read(const char* path, hu_hmm_prior* out) try {
	const char* fn = "hu_hmm_prior_read";
	if(!path || !out) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	std::ifstream f(path, std::ios::binary);
	if(!f.is_open()) { hu_set_error("%s: unable to open '%s'", fn, path); return HU_ERR_IO; }
	DmLines in;
	for(std::string s; std::getline(f, s); ) { if(!s.empty() && s.back() == '\r') s.pop_back(); in.line.push_back(s); }
	if(f.bad()) { hu_set_error("%s: unable to read '%s'", fn, path); return HU_ERR_IO; }
	static const char* heads[5] = {"Match emission:", "Insert emission:", "Match transition:", "Insert transition:", "Delete transition:"};
	static const int dims[5] = {4, 4, 3, 2, 2};
	hu_hmm_prior p;
	memset(&p, 0, sizeof(p));
	double* alpha[5] = {&p.me_alpha[0][0], p.ie_alpha, p.mt_alpha, p.it_alpha, p.dt_alpha};
	bool seen[5] = {false, false, false, false, false};
	while(in.more()) {
		int b = -1;
		for(int h = 0; h < 5; ++h) if(starts_with(in.line[in.at], heads[h])) b = h;
		++in.at;
		if(b < 0) continue;     /* the reference skips every other line between blocks too */
		std::string why;
		if(!dm_model(in, b == 0, dims[b], &p.me_L, p.me_q, alpha[b], why)) { hu_set_error("%s: '%s': block '%s' %s", fn, path, heads[b], why.c_str()); return HU_ERR_IO; }
		seen[b] = true;
	}
	for(int h = 0; h < 5; ++h) if(!seen[h]) { hu_set_error("%s: '%s': block '%s' is missing (empty or partial prior file)", fn, path, heads[h]); return HU_ERR_IO; }
	*out = p;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_hmm_prior_read"); }

extern "C" int hu_hmm_write(const char* path, const char* version, const char* name, int32_t K, int32_t cs_len, const double* p_m, const double* p_i,
		const double* p_t, const int32_t* map, const char* cons, int64_t n_seq, double eff_n, const char* date) try {
	const char* fn = "hu_hmm_write";
	if(!path || !version || !name || K < 1 || cs_len < K || !p_m || !p_i || !p_t || !map || !cons || n_seq < 1 || !date) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	char t[64];
	auto cost = [&](double p, bool star) -> std::string {     /* ostream << -log(p) at the default precision; hmmPrintValue (src/BandedHMMP7.h:922-924) */
		const double c = -std::log(p);
		if(c == std::numeric_limits<double>::infinity()) return star ? "*" : "inf";
		snprintf(t, sizeof(t), "%g", c);
		return t;
	};
	std::string o = std::string("HMMER3/f\t") + version + "\nNAME\t" + name + "\nLENG\t" + std::to_string(K) + "\nALPH\tDNA\n";
	snprintf(t, sizeof(t), "%g", eff_n);
	o += "MAXL  " + std::to_string(cs_len) + "\nRF  no\nMM  no\nCONS  yes\nCS  no\nMAP  yes\nNSEQ  " + std::to_string(n_seq) + "\nEFFN  " + t + "\nDATE  " + date + "\n";
	o += "HMM\t\tA\tC\tG\tT\n\t\tm->m\tm->i\tm->d\ti->m\ti->i\td->m\td->d\n";
	for(int32_t k = 0; k <= K; ++k) {
		o += k == 0 ? std::string("\tCOMPO") : "\t" + std::to_string(k);
		for(int b = 0; b < 4; ++b) o += "\t" + cost(p_m[(size_t) k * 4 + b], false);
		if(k > 0) { o += "\t" + std::to_string(map[k - 1]) + "\t"; o += cons[k - 1]; o += "\t-\t-\t-"; }
		o += "\n\t";
		for(int b = 0; b < 4; ++b) o += "\t" + cost(p_i[(size_t) k * 4 + b], true);
		const double* T = p_t + (size_t) k * 9;
		o += "\n\t";
		for(int q : {0, 1, 2, 3, 4, 6, 8}) o += "\t" + cost(T[q], true);     /* m->m m->i m->d i->m i->i d->m d->d */
		o += "\n";
	}
	o += "//\n";
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
} catch(...) { return hu_catch_all("hu_hmm_write"); }
