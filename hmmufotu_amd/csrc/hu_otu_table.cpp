// The OTU table of hmmufotu-merge, hmmufotu-subset and hmmufotu-norm, host only, no HIP headers: the reader and the
// writer of the reference's "table" format (OTUTable::loadTable / saveTable, src/OTUTable.cpp:123-164; readProgInfo / writeProgInfo,
// src/util/ProgEnv.cpp:101-135), operator+= (:211-240), pruneSamples / pruneOTUs (:88-108), normalizeConst (:110-121), and the host path
// of hu_otu_subset (subsetUniform / subsetMultinom, :166-209, on the names of hu_otu_table.h), which the device path is tested against.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "hu_num_format.h"
#include "hu_otu_table.h"
#include "hu_draw.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

struct hu_otu_table {
	std::vector<std::string> samples, otus, taxa;
	std::vector<double> m;                                   /* [otus][samples], row-major */
	std::unordered_map<std::string, size_t> otuAt, sampleAt;
	size_t S() const { return samples.size(); }
	size_t M() const { return otus.size(); }
	bool empty() const { return m.empty(); }                 /* metric.size() == 0 */
	/* addOTU (:61-72): an id already there keeps its row */
	size_t addOTU(const std::string& id, const std::string& taxon, const double* row) {
		auto it = otuAt.find(id);
		if(it != otuAt.end()) return it->second;
		const size_t at = otus.size();
		otuAt.emplace(id, at); otus.push_back(id); taxa.push_back(taxon);
		if(row) m.insert(m.end(), row, row + S()); else m.insert(m.end(), S(), 0.0);
		return at;
	}
	/* addSample (:36-46): a new column of zeros at the right */
	size_t addSample(const std::string& name) {
		auto it = sampleAt.find(name);
		if(it != sampleAt.end()) return it->second;
		const size_t s0 = S(), rows = M();
		std::vector<double> w(rows * (s0 + 1), 0.0);
		for(size_t i = 0; i < rows; ++i) std::copy(m.begin() + i * s0, m.begin() + (i + 1) * s0, w.begin() + i * (s0 + 1));
		m.swap(w); sampleAt.emplace(name, s0); samples.push_back(name);
		return s0;
	}
	void keepSamples(const std::vector<char>& keep) {
		const size_t s0 = S(), rows = M();
		std::vector<std::string> names; std::vector<double> w;
		for(size_t j = 0; j < s0; ++j) if(keep[j]) names.push_back(samples[j]);
		w.reserve(rows * names.size());
		for(size_t i = 0; i < rows; ++i) for(size_t j = 0; j < s0; ++j) if(keep[j]) w.push_back(m[i * s0 + j]);
		samples.swap(names); m.swap(w);
		sampleAt.clear();
		for(size_t j = 0; j < samples.size(); ++j) sampleAt.emplace(samples[j], j);     /* a name the header repeats: the first column has it */
	}
	void keepOTUs(const std::vector<char>& keep) {
		const size_t s0 = S(), rows = M();
		std::vector<std::string> ids, tx; std::vector<double> w;
		for(size_t i = 0; i < rows; ++i) if(keep[i]) { ids.push_back(otus[i]); tx.push_back(taxa[i]); w.insert(w.end(), m.begin() + i * s0, m.begin() + (i + 1) * s0); }
		otus.swap(ids); taxa.swap(tx); m.swap(w);
		otuAt.clear();
		for(size_t i = 0; i < otus.size(); ++i) otuAt.emplace(otus[i], i);
	}
};

static const int HU_OTU_VER[3] = {1, 5, 1};

static int read_table(std::istream& in, const char* name, hu_otu_table& T) {
	const char* fn = "hu_otu_table_read";
	std::string line;
	/* readProgInfo: "# %s %s", the name, then the version as VersionSequence::parseString scans it ("v%d.%d.%d", fields it cannot read stay 0) */
	std::getline(in, line);
	char pname[256], ver[256];
	if(sscanf(line.c_str(), "# %255s %255s", pname, ver) != 2) { hu_set_error("%s: Unrecognized input file for HmmUFOtu", name); return HU_ERR_IO; }
	if(strcmp(pname, "HmmUFOtu") != 0) { hu_set_error("%s: Not an valid input file of HmmUFOtu", name); return HU_ERR_IO; }
	int v[3] = {0, 0, 0};
	sscanf(ver, "v%d.%d.%d", &v[0], &v[1], &v[2]);
	if(std::lexicographical_compare(HU_OTU_VER, HU_OTU_VER + 3, v, v + 3)) {
		hu_set_error("%s: You are using an old version of HmmUFOtu-v1.5.1 to read a newer input file that is build by HmmUFOtu-v%d.%d.%d please download the latest program from 'https://github.com/Grice-Lab/HmmUFOtu'", name, v[0], v[1], v[2]);
		return HU_ERR_IO;
	}
	bool header = false;
	size_t N = 0;
	std::vector<double> row;
	for(long long ln = 2; std::getline(in, line); ++ln) {
		if(line.empty()) continue;
		if(line.compare(0, 5, "otuID") == 0) {
			if(header) { hu_set_error("%s: line %lld: a second header", name, ln); return HU_ERR_IO; }
			std::vector<std::string> f;
			for(size_t at = 0;;) { const size_t tab = line.find('\t', at); f.push_back(line.substr(at, tab == std::string::npos ? tab : tab - at)); if(tab == std::string::npos) break; at = tab + 1; }
			if(f.size() < 2) { hu_set_error("%s: line %lld: a header of %zu field(s): otuID, the samples, taxonomy", name, ln, f.size()); return HU_ERR_IO; }
			N = f.size() - 2;
			for(size_t j = 0; j < N; ++j) { T.sampleAt.emplace(f[j + 1], j); T.samples.push_back(f[j + 1]); }
			row.resize(N);
			header = true;
			continue;
		}
		if(!header) { hu_set_error("%s: line %lld: a value line before the 'otuID' header", name, ln); return HU_ERR_IO; }
		std::string id, taxon;
		std::istringstream li(line);
		std::getline(li, id, '\t');
		for(size_t j = 0; j < N; ++j) if(!(li >> row[j])) { hu_set_error("%s: line %lld: OTU '%s' has %zu of %zu numbers", name, ln, id.c_str(), j, N); return HU_ERR_IO; }
		if(N > 0) li.ignore(1, '\t');                                     /* the tab after the last number; without samples the id's tab was it */
		std::getline(li, taxon);
		T.addOTU(id, taxon, row.data());
	}
	if(in.bad()) { hu_set_error("%s: %s: read error", fn, name); return HU_ERR_IO; }
	return HU_OK;
}

extern "C" int hu_otu_table_read(const char* path, hu_otu_table** out) try {
	if(!path || !out) { hu_set_error("hu_otu_table_read: null argument"); return HU_ERR_ARG; }
	*out = nullptr;
	std::ifstream in(path);
	if(!in) { hu_set_error("Unable to open OTUTable '%s'", path); return HU_ERR_IO; }
	hu_otu_table* t = new hu_otu_table;
	const int rc = read_table(in, path, *t);
	if(rc != HU_OK) { delete t; return rc; }
	*out = t;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_read"); }

extern "C" int hu_otu_table_new(int64_t n_otu, int64_t n_sample, const char* const* otu_ids, const char* const* taxa, const char* const* samples, const double* counts,
		hu_otu_table** out) try {
	if(n_otu < 0 || n_sample < 0 || !out || (n_otu > 0 && (!otu_ids || !taxa)) || (n_sample > 0 && !samples) || (n_otu > 0 && n_sample > 0 && !counts)) { hu_set_error("hu_otu_table_new: bad argument"); return HU_ERR_ARG; }
	*out = nullptr;
	hu_otu_table* t = new hu_otu_table;
	struct Drop { hu_otu_table* t; ~Drop() { delete t; } } drop{t};
	for(int64_t j = 0; j < n_sample; ++j) { if(!samples[j]) { hu_set_error("hu_otu_table_new: sample %lld has no name", (long long) j); return HU_ERR_ARG; } t->sampleAt.emplace(samples[j], (size_t) j); t->samples.push_back(samples[j]); }
	for(int64_t i = 0; i < n_otu; ++i) {
		if(!otu_ids[i] || !taxa[i]) { hu_set_error("hu_otu_table_new: OTU %lld has no id or no taxonomy", (long long) i); return HU_ERR_ARG; }
		t->addOTU(otu_ids[i], taxa[i], n_sample > 0 ? counts + (size_t) i * n_sample : nullptr);
	}
	*out = t; drop.t = nullptr;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_new"); }

extern "C" void hu_otu_table_free(hu_otu_table* t) { delete t; }

extern "C" int hu_otu_table_dims(const hu_otu_table* t, int64_t* n_otu, int64_t* n_sample) {
	if(!t) { hu_set_error("hu_otu_table_dims: null table"); return HU_ERR_ARG; }
	if(n_otu) *n_otu = (int64_t) t->M();
	if(n_sample) *n_sample = (int64_t) t->S();
	return HU_OK;
}
extern "C" const char* hu_otu_table_otu(const hu_otu_table* t, int64_t i) { return t && i >= 0 && (size_t) i < t->M() ? t->otus[(size_t) i].c_str() : nullptr; }
extern "C" const char* hu_otu_table_taxon(const hu_otu_table* t, int64_t i) { return t && i >= 0 && (size_t) i < t->M() ? t->taxa[(size_t) i].c_str() : nullptr; }
extern "C" const char* hu_otu_table_sample(const hu_otu_table* t, int64_t j) { return t && j >= 0 && (size_t) j < t->S() ? t->samples[(size_t) j].c_str() : nullptr; }
extern "C" double* hu_otu_table_counts(hu_otu_table* t) { return t ? t->m.data() : nullptr; }

extern "C" int hu_otu_table_write(const hu_otu_table* t, const char* path, const char* info) try {
	if(!t || !path) { hu_set_error("hu_otu_table_write: null argument"); return HU_ERR_ARG; }
	std::ofstream f;
	const bool toStdout = strcmp(path, "-") == 0;
	if(!toStdout) { f.open(path); if(!f) { hu_set_error("Unable to write to '%s'", path); return HU_ERR_IO; } }
	std::ostream& o = toStdout ? std::cout : f;
	o << "# HmmUFOtu v1.5.1" << (info ? info : "") << std::endl;          /* writeProgInfo */
	/* saveTable: "otuID\t" << join(samples, "\t") << "\ttaxonomy"; a table that has lost every sample is written as hmmufotu-amd-sum
	 * writes one, without the empty field the reference's join leaves, which its own reader takes for a sample without a name */
	o << "otuID";
	for(size_t j = 0; j < t->S(); ++j) o << "\t" << t->samples[j];
	o << "\ttaxonomy" << std::endl;
	const size_t S = t->S();
	for(size_t i = 0; i < t->M(); ++i) {
		o << t->otus[i];
		for(size_t j = 0; j < S; ++j) o << "\t" << hu_num(t->m[i * S + j]);
		o << "\t" << t->taxa[i] << std::endl;
	}
	o.flush();
	if(!o) { hu_set_error("Unable to write to '%s'", path); return HU_ERR_IO; }
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_write"); }

extern "C" int hu_otu_table_merge(hu_otu_table* dst, const hu_otu_table* src) try {
	if(!dst || !src || dst == src) { hu_set_error("hu_otu_table_merge: two different tables"); return HU_ERR_ARG; }
	if(dst->empty()) { *dst = *src; return HU_OK; }
	if(src->empty()) return HU_OK;
	std::vector<size_t> col(src->S());
	for(size_t j = 0; j < src->S(); ++j) col[j] = dst->addSample(src->samples[j]);
	const size_t S = dst->S(), s1 = src->S();
	for(size_t i = 0; i < src->M(); ++i) dst->addOTU(src->otus[i], src->taxa[i], nullptr);
	for(size_t i = 0; i < src->M(); ++i) {
		const size_t i0 = dst->otuAt.at(src->otus[i]);
		for(size_t j = 0; j < s1; ++j) dst->m[i0 * S + col[j]] += src->m[i * s1 + j];
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_merge"); }

/* metric.col(j).sum() / metric.row(i).sum() in ascending order: exact for the integer tables hmmufotu-amd-sum writes */
static double col_sum(const hu_otu_table& t, size_t j) { double s = 0; for(size_t i = 0; i < t.M(); ++i) s += t.m[i * t.S() + j]; return s; }

extern "C" int hu_otu_table_prune_samples(hu_otu_table* t, uint64_t min) try {
	if(!t) { hu_set_error("hu_otu_table_prune_samples: null table"); return HU_ERR_ARG; }
	if(min == 0) return HU_OK;
	std::vector<char> keep(t->S());
	for(size_t j = 0; j < t->S(); ++j) keep[j] = !(col_sum(*t, j) < (double) min);
	t->keepSamples(keep);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_prune_samples"); }

extern "C" int hu_otu_table_prune_otus(hu_otu_table* t) try {
	if(!t) { hu_set_error("hu_otu_table_prune_otus: null table"); return HU_ERR_ARG; }
	std::vector<char> keep(t->M());
	const size_t S = t->S();
	for(size_t i = 0; i < t->M(); ++i) { double s = 0; for(size_t j = 0; j < S; ++j) s += t->m[i * S + j]; keep[i] = !(s == 0); }
	t->keepOTUs(keep);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_prune_otus"); }

extern "C" int hu_otu_table_normalize(hu_otu_table* t, double Z, int64_t* zero_columns) try {
	if(!t || !(Z >= 0)) { hu_set_error("hu_otu_table_normalize: Z must be non-negative"); return HU_ERR_ARG; }
	if(zero_columns) *zero_columns = 0;
	if(t->empty() || std::all_of(t->m.begin(), t->m.end(), [](double v) { return v == 0; })) return HU_OK;
	const size_t S = t->S(), M = t->M();
	std::vector<double> sum(S);
	for(size_t j = 0; j < S; ++j) sum[j] = col_sum(*t, j);
	if(Z == 0) Z = *std::max_element(sum.begin(), sum.end());
	for(size_t j = 0; j < S; ++j) {
		if(sum[j] == 0) { if(zero_columns) ++*zero_columns; continue; }     /* the reference: 0 / 0 */
		const double norm = sum[j] / Z;
		for(size_t i = 0; i < M; ++i) t->m[i * S + j] /= norm;
	}
	return HU_OK;
} catch(...) { return hu_catch_all("hu_otu_table_normalize"); }

/* ---- hu_otu_subset: the checks and the host path ---- */

extern "C" void hu_otu_default_opts(hu_otu_opts* o) { if(o) { o->chunk = HU_OTU_CHUNK; o->key_bits = 64; } }

int hu_otu_subset_check(const char* fn, int64_t n_otu, int64_t n_sample, const double* counts, uint64_t size, int method, const hu_otu_opts* opts,
		const double* out, hu_otu_opts* eff, std::vector<uint64_t>& total) {
	if(n_otu < 0 || n_sample < 0 || n_otu > INT32_MAX || n_sample > INT32_MAX || (n_otu > 0 && n_sample > 0 && (!counts || !out || out == counts))) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	if(size == 0) { hu_set_error("%s: size must be positive", fn); return HU_ERR_ARG; }
	if(method != HU_OTU_UNIFORM && method != HU_OTU_MULTINOMIAL) { hu_set_error("%s: unknown method %d", fn, method); return HU_ERR_ARG; }
	hu_otu_default_opts(eff);
	if(opts) *eff = *opts;
	if(eff->chunk < 1 || eff->chunk > (1 << 24)) { hu_set_error("%s: chunk %d: 1 .. %d reads per workgroup", fn, eff->chunk, 1 << 24); return HU_ERR_ARG; }
	if(eff->key_bits < 1 || eff->key_bits > 64) { hu_set_error("%s: key_bits %d: 1 .. 64", fn, eff->key_bits); return HU_ERR_ARG; }
	return hu_otu_cells_check(fn, n_otu, n_sample, counts, total);
}

int hu_otu_cells_check(const char* fn, int64_t n_otu, int64_t n_sample, const double* counts, std::vector<uint64_t>& total) {
	total.assign((size_t) n_sample, 0);
	for(int64_t i = 0; i < n_otu; ++i) for(int64_t j = 0; j < n_sample; ++j) {
		const double v = counts[(size_t) i * n_sample + j];
		if(!(v >= 0) || !(v < 4294967296.0) || v != std::floor(v)) {
			if(v >= 4294967296.0) hu_set_error("%s: OTU %lld, sample %lld: %.17g reads: a sample's total must be below 2^32", fn, (long long) i, (long long) j, v);
			else hu_set_error("%s: OTU %lld, sample %lld: the count %.17g is not a non-negative integer", fn, (long long) i, (long long) j, v);
			return HU_ERR_ARG;
		}
		total[(size_t) j] += (uint64_t) v;
		if(total[(size_t) j] >= (1ull << 32)) { hu_set_error("%s: sample %lld holds 2^32 reads or more", fn, (long long) j); return HU_ERR_ARG; }
	}
	return HU_OK;
}

void hu_otu_subset_host(int64_t n_otu, int64_t n_sample, const double* counts, const std::vector<uint64_t>& total, uint64_t size, int method, uint64_t seed,
		int key_bits, double* out) {
	const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
	std::copy(counts, counts + (size_t) n_otu * n_sample, out);
	std::vector<uint64_t> keys, prefix;
	std::vector<int64_t> rowOf;
	for(int64_t j = 0; j < n_sample; ++j) {
		const uint64_t T = total[(size_t) j];
		if(T <= size) continue;                                            /* not enough reads to subset */
		auto cell = [&](int64_t i) -> uint64_t { return (uint64_t) counts[(size_t) i * n_sample + j]; };
		if(method == HU_OTU_UNIFORM) {
			/* the cut (hu_draw.h), then the reads in row order */
			keys.resize((size_t) T);
			for(uint64_t t = 0; t < T; ++t) keys[(size_t) t] = hu_otu_key(key, t, (uint32_t) j, key_bits);
			uint64_t cut, need, end = 0;
			hu_draw_cut(keys, size, cut, need);
			hu_draw_walk(cut, need, (uint64_t) n_otu, [&](uint64_t i) { return end += cell((int64_t) i); },
				[&](uint64_t t) { return hu_otu_key(key, t, (uint32_t) j, key_bits); }, [&](uint64_t i, uint64_t kept) { out[(size_t) i * n_sample + j] = (double) kept; });
		}
		else {
			prefix.clear(); rowOf.clear();
			uint64_t p = 0;
			for(int64_t i = 0; i < n_otu; ++i) if(cell(i) > 0) { prefix.push_back(p); rowOf.push_back(i); p += cell(i); }
			for(int64_t i = 0; i < n_otu; ++i) out[(size_t) i * n_sample + j] = 0;
			for(uint64_t m = 0; m < size; ++m) {
				const uint64_t t = hu_otu_draw(key, m, (uint32_t) j, T);
				const size_t c = (size_t)(std::upper_bound(prefix.begin(), prefix.end(), t) - prefix.begin()) - 1;
				out[(size_t) rowOf[c] * n_sample + j] += 1;
			}
		}
	}
}
