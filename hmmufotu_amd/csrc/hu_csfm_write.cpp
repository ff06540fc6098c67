// Writing the reference's seed index file, <DB>.csfm: CSFMIndex::save (src/CSFMIndex.cpp:176-198) over buildBasic,
// buildConcatSeq and buildBWT (:275-368), restated.  The suffix array comes from the device (hu_csfm_write) or from the caller
// (hu_csfm_encode); everything else here is host work, threaded with hu_run_threads on at most 16 threads.
//
// The two libcds structures of the file are written by this project's own encoders, the inverse of the decoders in hu_seedindex.cpp:
//     BitSequenceRRR     blocks of 15 bits; per block its popcount c in 4 bits and its index among the 15-bit words of popcount c — in
//                        the order TableOffsetRRR generates them — in bits(binomial(15, c) - 1) bits; sample rate 8 in the header (the
//                        samples themselves are not serialised)
//     WaveletTreeNoptrs  height = bits(max symbol); one padding symbol appended for every value of 0..max_v that does not occur; level l
//                        holds bit (height - 1 - l) of the symbols stably grouped by their higher bits; OCC has max_v + 2 entries
// Tested byte for byte against files written by the real libcds + libdivsufsort (oracle/csfm_ref.cpp, tests/test_csfm_write.py).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <thread>
#include <vector>
#include "hu_common.h"

namespace {
const unsigned SA_SAMPLE_RATE = 4, RRR_SAMPLE_RATE = 8, RRR_BLOCK = 15;      /* src/CSFMIndex.h:133-134, BitSequenceRRR.h */

unsigned n_threads() { unsigned nt = std::thread::hardware_concurrency(); if(nt > 16) nt = 16; return nt < 1 ? 1 : nt; }
/* body(a, e) over [0, n) in shares of `grain` */
template<class F> void par(size_t n, size_t grain, F body) {
	std::atomic<size_t> next{0};
	hu_run_threads(n <= grain ? 1 : n_threads(), [&] { for(;;) { const size_t a = next.fetch_add(grain); if(a >= n) break; body(a, std::min(n, a + grain)); } });
}
inline uint32_t bits_of(uint32_t n) { uint32_t b = 0; while(n) { ++b; n >>= 1; } return b; }

/* the index of every 15-bit word among the words of its popcount, in libcds's generation order, and the width of that index */
struct RrrTables {
	std::vector<uint16_t> index; uint32_t width[16]; uint32_t made[16];
	RrrTables() : index(1u << RRR_BLOCK, 0) {
		for(int c = 0; c <= 15; ++c) { made[c] = 0; gen(c, 0, 0, 0); width[c] = bits_of(made[c] - 1); }
	}
	void gen(int cls, int placed, int from, uint32_t word) {
		if(placed == cls) { index[word] = (uint16_t) made[cls]++; return; }
		for(int i = from; i < (int) RRR_BLOCK; ++i) gen(cls, placed + 1, i + 1, word | (1u << i));
	}
};
/* bits [len] in 64-bit words, bit i at bit i & 63 of word i / 64; the words hold zeros beyond len and one spare word follows */
inline uint32_t block15(const uint64_t* w, size_t k) {
	const size_t b = k * RRR_BLOCK; const unsigned s = (unsigned)(b & 63);
	uint64_t v = w[b >> 6] >> s;
	if(s > 49) v |= w[(b >> 6) + 1] << (64 - s);
	return (uint32_t) v & 0x7fffu;
}
/* BitSequenceRRR::save of the sequence BitSequenceRRR::build makes of these bits (BitSequenceRRR.cpp:51-87, :379-402) */
bool write_rrr(std::ostream& f, const uint64_t* w, size_t len) {
	static const RrrTables T;
	const size_t cLen = (len + RRR_BLOCK - 1) / RRR_BLOCK;
	const size_t share = 1 << 16;                                              /* blocks per share: a multiple of 8, so shares own whole words of C */
	const size_t nShare = (cLen + share - 1) / share;
	std::vector<uint32_t> C((cLen * 4 + 31) / 32, 0);
	std::vector<uint64_t> shareBits(nShare + 1, 0), shareOnes(nShare, 0);
	par(nShare, 1, [&](size_t a, size_t e) {
		for(size_t s = a; s < e; ++s) {
			uint64_t ob = 0, on = 0;
			for(size_t k = s * share; k < std::min(cLen, (s + 1) * share); ++k) {
				const uint32_t c = (uint32_t) __builtin_popcount(block15(w, k));
				C[k >> 3] |= c << (4 * (k & 7));
				ob += T.width[c]; on += c;
			}
			shareBits[s + 1] = ob; shareOnes[s] = on;
		}
	});
	uint64_t ones = 0;
	for(size_t s = 0; s < nShare; ++s) { shareBits[s + 1] += shareBits[s]; ones += shareOnes[s]; }
	const uint64_t oBits = shareBits[nShare];
	if(oBits >= (1ull << 32) || cLen >= (1ull << 32)) return false;              /* the file holds both as uint32 */
	std::vector<uint32_t> O((size_t)((oBits + 31) / 32), 0);
	par(nShare, 1, [&](size_t a, size_t e) {                                     /* a word shared by two shares is completed with atomic ORs */
		for(size_t s = a; s < e; ++s) {
			uint64_t at = shareBits[s];
			size_t word = (size_t)(at >> 5); uint64_t acc = 0;                   /* acc: bits of O[word], O[word + 1] not yet flushed */
			auto flush = [&](size_t wd, uint32_t v) { if(v) __atomic_fetch_or(&O[wd], v, __ATOMIC_RELAXED); };
			for(size_t k = s * share; k < std::min(cLen, (s + 1) * share); ++k) {
				const uint32_t v = block15(w, k), wd = T.width[(uint32_t) __builtin_popcount(v)];
				if(!wd) continue;
				acc |= (uint64_t) T.index[v] << (at - ((uint64_t) word << 5));
				at += wd;
				if((at >> 5) != word) { flush(word, (uint32_t) acc); acc >>= 32; ++word; }
			}
			flush(word, (uint32_t) acc);
		}
	});
	const uint32_t hdr = 2, cLen32 = (uint32_t) cLen, cBits = 4, oLen = (uint32_t) O.size(), oBits32 = (uint32_t) oBits, rate = RRR_SAMPLE_RATE;
	const uint64_t len64 = len;
	f.write((const char*) &hdr, 4); f.write((const char*) &len64, 8); f.write((const char*) &ones, 8);
	f.write((const char*) &cLen32, 4); f.write((const char*) &cBits, 4); f.write((const char*) &oLen, 4); f.write((const char*) &oBits32, 4); f.write((const char*) &rate, 4);
	f.write((const char*) C.data(), (std::streamsize)(C.size() * 4)); f.write((const char*) O.data(), (std::streamsize)(O.size() * 4));
	return true;
}
/* WaveletTreeNoptrs::save of the tree its constructor makes of sym [n] (WaveletTreeNoptrs.cpp:157-225, :245-257, build_level :524-558) with a
 * MapperNone and RRR bitmaps */
bool write_wavelet(std::ostream& f, const uint8_t* sym, size_t n) {
	const size_t share = 1 << 20, nShare = (n + share - 1) / share;
	std::vector<uint64_t> cnt(nShare * 256, 0);
	par(nShare, 1, [&](size_t a, size_t e) { for(size_t s = a; s < e; ++s) { uint64_t* c = &cnt[s * 256]; for(size_t i = s * share; i < std::min(n, (s + 1) * share); ++i) c[sym[i]]++; } });
	uint64_t total[256] = {0};
	for(size_t s = 0; s < nShare; ++s) for(int v = 0; v < 256; ++v) total[v] += cnt[s * 256 + v];
	uint32_t maxV = 0;
	for(int v = 0; v < 256; ++v) if(total[v]) maxV = (uint32_t) v;
	const uint32_t height = bits_of(maxV);
	std::vector<uint8_t> pad;                                                    /* one symbol per absent value, ascending, behind the sequence */
	for(uint32_t v = 0; v <= maxV; ++v) if(!total[v]) { pad.push_back((uint8_t) v); total[v] = 1; }
	const size_t nn = n + pad.size();
	std::vector<uint32_t> OCC(maxV + 2, 0);
	for(uint32_t v = 0; v <= maxV; ++v) OCC[v + 1] = OCC[v] + (uint32_t) total[v];
	const uint32_t hdr = 3, mapper = 2;
	const uint64_t nn64 = nn, len64 = n;
	f.write((const char*) &hdr, 4); f.write((const char*) &nn64, 8); f.write((const char*) &len64, 8);
	f.write((const char*) &maxV, 4); f.write((const char*) &height, 4); f.write((const char*) &mapper, 4);
	std::vector<uint64_t> bm;
	for(uint32_t l = 0; l < height; ++l) {
		/* the symbols of one group (equal bits above this level's) lie together, groups ascending, symbols in sequence order inside */
		const uint32_t down = height - l, nGroup = 1u << l, bit = height - 1 - l;
		std::vector<uint64_t> gTot(nGroup + 1, 0);
		for(uint32_t v = 0; v <= maxV; ++v) gTot[(v >> down) + 1] += total[v];
		for(uint32_t g = 0; g < nGroup; ++g) gTot[g + 1] += gTot[g];
		std::vector<uint64_t> cursor((nShare + 1) * nGroup, 0);                  /* first slot of every (share, group); share nShare: the padding */
		{
			std::vector<uint64_t> run(gTot.begin(), gTot.end() - 1);
			for(size_t s = 0; s <= nShare; ++s) for(uint32_t g = 0; g < nGroup; ++g) {
				cursor[s * nGroup + g] = run[g];
				if(s < nShare) for(uint32_t v = g << down; v < ((g + 1) << down) && v < 256; ++v) run[g] += cnt[s * 256 + v];
			}
		}
		bm.assign(nn / 64 + 2, 0);
		auto place = [&](const uint8_t* p, size_t k, uint64_t* cur) {             /* runs of one group are consecutive slots: a word is flushed when left */
			std::vector<uint64_t> acc(nGroup, 0), word(nGroup, ~0ull);
			auto flush = [&](uint32_t g) { if(acc[g]) __atomic_fetch_or(&bm[(size_t) word[g]], acc[g], __ATOMIC_RELAXED); acc[g] = 0; };
			for(size_t i = 0; i < k; ++i) {
				const uint32_t v = p[i], g = v >> down;
				const uint64_t at = cur[g]++;
				if((at >> 6) != word[g]) { if(word[g] != ~0ull) flush(g); word[g] = at >> 6; }
				acc[g] |= (uint64_t)((v >> bit) & 1u) << (at & 63);
			}
			for(uint32_t g = 0; g < nGroup; ++g) if(word[g] != ~0ull) flush(g);
		};
		par(nShare, 1, [&](size_t a, size_t e) { for(size_t s = a; s < e; ++s) place(sym + s * share, std::min(n, (s + 1) * share) - s * share, &cursor[s * nGroup]); });
		place(pad.data(), pad.size(), &cursor[nShare * nGroup]);
		if(!write_rrr(f, bm.data(), nn)) return false;
	}
	f.write((const char*) OCC.data(), (std::streamsize)(OCC.size() * 4));
	return true;
}

/* buildConcatSeq (src/CSFMIndex.cpp:287-325): the residues of every row as encode(toupper(c)) + 1, a 0 behind every row and one more at the end;
 * concat2CS = the 1-based column of every residue, 0 elsewhere; C = the cumulative symbol counts */
struct Concat {
	std::vector<uint8_t> text; std::vector<uint16_t> c2cs; int32_t C[256]; int64_t concatLen = 0;
};
int build_concat(const char* fn, int64_t nSeq, int64_t L, const char* rows, Concat& out) {
	int8_t enc[256];
	hu_msa_encode_table(enc);
	std::vector<int64_t> off((size_t) nSeq + 1, 0);
	std::atomic<int64_t> badAt{-1};
	par((size_t) nSeq, 64, [&](size_t a, size_t e) {
		for(size_t i = a; i < e; ++i) {
			const unsigned char* r = (const unsigned char*) rows + i * (size_t) L;
			int64_t k = 0;
			for(int64_t j = 0; j < L; ++j) {
				const int8_t c = enc[r[j]];
				if(c >= 0) ++k;
				else if(c != -2) { int64_t at = (int64_t) i * L + j, seen = badAt.load(); while((seen < 0 || at < seen) && !badAt.compare_exchange_weak(seen, at)) { } break; }
			}
			off[i + 1] = k + 1;
		}
	});
	if(badAt >= 0) {
		const int64_t i = badAt / L, j = badAt % L; const unsigned char c = (unsigned char) rows[badAt];
		char shown[8]; if(c >= 33 && c < 127) snprintf(shown, sizeof(shown), "'%c'", c); else snprintf(shown, sizeof(shown), "0x%02x", c);
		hu_set_error("%s: row %lld, column %lld of the alignment holds %s, neither a gap nor a residue of the DNA alphabet", fn, (long long) i + 1, (long long) j + 1, shown);
		return HU_ERR_ARG;
	}
	for(int64_t i = 0; i < nSeq; ++i) off[i + 1] += off[i];
	out.concatLen = off[nSeq];
	if(out.concatLen + 1 >= (1ll << 31)) { hu_set_error("%s: the concatenated text would hold %lld symbols, the index format at most 2^31 - 1", fn, (long long) out.concatLen + 1); return HU_ERR_ARG; }
	const size_t N = (size_t) out.concatLen + 1;
	out.text.assign(N, 0); out.c2cs.assign(N, 0);
	const size_t nShare = ((size_t) nSeq + 63) / 64;
	std::vector<int64_t> cnt(nShare * 5, 0);
	par((size_t) nSeq, 64, [&](size_t a, size_t e) {
		int64_t* cn = &cnt[(a / 64) * 5];
		for(size_t i = a; i < e; ++i) {
			const unsigned char* r = (const unsigned char*) rows + i * (size_t) L;
			size_t at = (size_t) off[i];
			for(int64_t j = 0; j < L; ++j) { const int8_t c = enc[r[j]]; if(c >= 0) { out.text[at] = (uint8_t)(c + 1); out.c2cs[at] = (uint16_t)(j + 1); cn[c + 1]++; ++at; } }
			cn[0]++;
		}
	});
	int64_t tot[5] = {1, 0, 0, 0, 0};                                            /* the terminator */
	for(size_t s = 0; s < nShare; ++s) for(int v = 0; v < 5; ++v) tot[v] += cnt[s * 5 + v];
	memset(out.C, 0, sizeof(out.C));
	for(int v = 1; v <= 5; ++v) out.C[v] = out.C[v - 1] + (int32_t) tot[v - 1];
	return HU_OK;
}
int check_args(const char* fn, const char* path, int64_t nSeq, int64_t L, const char* rows, const char* csSeq, const double* ident) {
	if(!path || !rows || !csSeq || !ident || nSeq < 1 || L < 1) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(L > 65535) { hu_set_error("%s: %lld columns, the index format holds at most 65535", fn, (long long) L); return HU_ERR_ARG; }
	if(nSeq >= (1ll << 31)) { hu_set_error("%s: %lld rows: the concatenated text would hold 2^31 symbols or more", fn, (long long) nSeq); return HU_ERR_ARG; }
	const size_t k = strnlen(csSeq, (size_t) L + 1);
	if(k != (size_t) L) { hu_set_error("%s: the consensus sequence has %s%zu characters, the alignment %lld columns", fn, k > (size_t) L ? "more than " : "", std::min(k, (size_t) L), (long long) L); return HU_ERR_ARG; }
	return HU_OK;
}
/* CSFMIndex::save */
int save(const char* fn, const char* path, int64_t L, const Concat& cc, const char* csSeq, const double* ident, const uint32_t* sampled, const uint64_t* marks, const uint8_t* bwt) {
	const size_t N = (size_t) cc.concatLen + 1;
	std::ofstream f(path, std::ios::binary);
	if(!f) { hu_set_error("cannot write CSFM file '%s'", path); return HU_ERR_IO; }
	std::vector<char> buf(1 << 22);
	f.rdbuf()->pubsetbuf(buf.data(), (std::streamsize) buf.size());
	hu_write_prog_info(f);
	const uint64_t three = 3, csN = (uint64_t) L + 1; const char gap = '-', blank = ' '; const uint16_t csLen = (uint16_t) L; const int32_t concatLen = (int32_t) cc.concatLen; const double zero = 0;
	f.write((const char*) &three, 8); f.write("DNA", 3); f.write(&gap, 1); f.write((const char*) &csLen, 2); f.write((const char*) &concatLen, 4);
	f.write((const char*) cc.C, sizeof(cc.C));
	f.write((const char*) &csN, 8); f.write(&blank, 1); f.write(csSeq, (std::streamsize) L);
	f.write((const char*) &zero, 8); f.write((const char*) ident, (std::streamsize)(8 * L));
	f.write((const char*) cc.c2cs.data(), (std::streamsize)(2 * N));
	f.write((const char*) sampled, (std::streamsize)(4 * ((size_t) cc.concatLen / SA_SAMPLE_RATE)));      /* ceil(N / 4) rows are sampled, the last in row order is not saved */
	if(!write_rrr(f, marks, N) || !write_wavelet(f, bwt, N)) { f.close(); remove(path); hu_set_error("%s: internal: a bit sequence too long for the format's 32-bit counters", fn); return HU_ERR_STATE; }
	f.flush();
	if(!f) { f.close(); remove(path); hu_set_error("%s: writing '%s' failed", fn, path); return HU_ERR_IO; }
	return HU_OK;
}
thread_local double g_timing[4] = {0, 0, 0, 0};
thread_local int32_t g_rounds = 0;
double since(std::chrono::steady_clock::time_point& t) { const auto now = std::chrono::steady_clock::now(); const double s = std::chrono::duration<double>(now - t).count(); t = now; return s; }
}

extern "C" int hu_csfm_encode(const char* path, int64_t n_seq, int64_t cs_len, const char* rows, const char* cs_seq, const double* cs_identity, const int32_t* sa) try {
	const char* fn = "hu_csfm_encode";
	int rc = check_args(fn, path, n_seq, cs_len, rows, cs_seq, cs_identity);
	if(rc != HU_OK) return rc;
	if(!sa) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	Concat cc;
	if((rc = build_concat(fn, n_seq, cs_len, rows, cc)) != HU_OK) return rc;
	const size_t N = (size_t) cc.concatLen + 1;
	/* buildBWT (src/CSFMIndex.cpp:327-368) from the given suffix array, which must be a permutation of 0 .. N - 1 */
	std::vector<uint8_t> bwt(N), seen(N, 0);
	std::vector<uint64_t> marks(N / 64 + 2, 0);
	std::vector<uint32_t> sampled(N / SA_SAMPLE_RATE + 1, 0);
	size_t k = 0;
	for(size_t i = 0; i < N; ++i) {
		const int32_t s = sa[i];
		if(s < 0 || (size_t) s >= N || seen[(size_t) s]) { hu_set_error("%s: the suffix array is not a permutation of 0 .. %zu (entry %zu)", fn, N - 1, i); return HU_ERR_ARG; }
		seen[(size_t) s] = 1;
		bwt[i] = s == 0 ? (uint8_t) 0 : cc.text[(size_t) s - 1];
		if(s % (int32_t) SA_SAMPLE_RATE == 0) { sampled[k++] = (uint32_t) s; marks[i >> 6] |= 1ull << (i & 63); }
	}
	return save(fn, path, cs_len, cc, cs_seq, cs_identity, sampled.data(), marks.data(), bwt.data());
} catch(...) { return hu_catch_all("hu_csfm_encode"); }

extern "C" int hu_csfm_write(const char* path, int64_t n_seq, int64_t cs_len, const char* rows, const char* cs_seq, const double* cs_identity, int device) try {
	const char* fn = "hu_csfm_write";
	auto t = std::chrono::steady_clock::now();
	int rc = check_args(fn, path, n_seq, cs_len, rows, cs_seq, cs_identity);
	if(rc != HU_OK) return rc;
	Concat cc;
	if((rc = build_concat(fn, n_seq, cs_len, rows, cc)) != HU_OK) return rc;
	const size_t N = (size_t) cc.concatLen + 1;
	g_timing[0] = since(t);
	std::vector<uint8_t> bwt(N);
	std::vector<uint64_t> marks(N / 64 + 2, 0);
	std::vector<uint32_t> sampled((N + 3) / 4 + 1, 0);
	if((rc = hu_csfm_device_pass(device, cc.text.data(), (int64_t) N, bwt.data(), marks.data(), sampled.data(), &g_rounds, &g_timing[3])) != HU_OK) return rc;
	g_timing[1] = since(t);
	std::vector<uint8_t>().swap(cc.text);
	rc = save(fn, path, cs_len, cc, cs_seq, cs_identity, sampled.data(), marks.data(), bwt.data());
	g_timing[2] = since(t);
	return rc;
} catch(...) { return hu_catch_all("hu_csfm_write"); }

extern "C" int hu_csfm_write_timing(double* seconds, int32_t* rounds) {
	if(seconds) memcpy(seconds, g_timing, sizeof(g_timing));
	if(rounds) *rounds = g_rounds;
	return HU_OK;
}
