// "A valid assignment" of hmmufotu-sum (src/hmmufotu-sum.cpp:374-382) on the integers behind it, in ONE place: the readers of an assignment
// file (hu_tsv_reader.h) count them from the alignment string, a run that summarises its own batches (hu_batch_get_summary)
// gets them from the device; both then decide with the expressions below, so the two routes cannot part at a threshold.  Host only.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

/* DegenAlphabet::isSymbol (src/DegenAlphabet.h:89-91: sym_map[c] >= 0) over IUPACNucl (src/IUPACNucl.cpp:33-50): the four bases and the
 * degenerate codes, which map to their first expansion — upper case only (inserts are lower case in an alignment and do not count):
 * what alignIdentity / hmmIdentity count (src/HmmUFOtu_main.cpp:218-239) */
#define HU_SUM_SYMBOLS "ACGTUMRWSYKVHDBN"

namespace hu_tsv {

inline bool is_symbol(char c) { return c != '\0' && strchr(HU_SUM_SYMBOLS, c) != nullptr; }

/* alignIdentity = symbols / columns of the region, hmmIdentity = symbols at match columns / match columns of the region: 0 / 0 is NaN,
 * which no threshold accepts */
inline double identity(int id, int n) { return (double) id / n; }

struct Accept { double minQ = 0, minAln = 0, minHmm = 0; };
/* n_cols = CS_end - CS_start + 1; n_sym, n_match, n_match_sym over the columns CS_start - 1 .. CS_end - 1 of the alignment; a filter at 0 is off */
inline bool accept_counts(const Accept& f, long taxon, double qTaxon, int n_cols, int n_sym, int n_match, int n_match_sym) {
	return taxon >= 0 && qTaxon >= f.minQ && (f.minAln == 0 || identity(n_sym, n_cols) >= f.minAln)
		&& (f.minHmm == 0 || identity(n_match_sym, n_match) >= f.minHmm);
}

/* a double as an assignment file shows it (operator<<(ostream&, double) at default precision == printf("%g")) and as its readers take it back (atof) */
inline int put_gd(char* p, double v) { return snprintf(p, 40, "%g", v); }
inline double through_tsv(double v) { char t[40]; put_gd(t, v); return atof(t); }

} // namespace hu_tsv
