// Host baseline of profiles/otu_cs_rate.py: the accumulation loop of hmmufotu-sum (src/hmmufotu-sum.cpp:391-397) restated in plain C++ with
// the reference's storage — per OTU a column-major 4 x L matrix of doubles (freq) and a row of L doubles (gap) — on one core.
//   for j < L: b = encode(toupper(aln[j])); b >= 0 ? freq(b, j)++ : gap(j)++
// Built by the script with g++ -O2 -shared -fPIC.
#include <cctype>
#include <cstdint>
#include <cstring>
extern "C" void otu_cs_baseline(int64_t n_rows, int64_t L, const int32_t* slot_of_row, const char* rows, const int8_t* enc /* [256] */,
		double* freq /* [slots][L][4] */, double* gap /* [slots][L] */) {
	for(int64_t i = 0; i < n_rows; ++i) {
		const char* aln = rows + i * L;
		double* f = freq + (int64_t) slot_of_row[i] * L * 4;
		double* g = gap + (int64_t) slot_of_row[i] * L;
		for(int64_t j = 0; j < L; ++j) {
			const int8_t b = enc[(unsigned char) ::toupper((unsigned char) aln[j])];
			if(b >= 0) f[j * 4 + b]++;
			else g[j]++;
		}
	}
}
