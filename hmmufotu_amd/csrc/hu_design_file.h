// The META file of hmmufotu-amd-permanova --design: tab-separated, the first non-empty line the header (a leading '#' of
// it is dropped, so a QIIME '#SampleID' file reads as is), later lines that start with '#' and empty lines skipped, the first column the
// sample name.  Lines that name no sample of the matrix are ignored and counted.  Header only and without output of its own: a refusal is
// returned as text, so that the program and the sanitizer driver (tests/san/permanova_design_driver.cpp) share it.
#pragma once
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>
#include <vector>

struct HuMeta {
	std::vector<std::string> column;                 /* the header's names after the sample column */
	std::vector<std::vector<std::string>> value;     /* [n][columns]: the fields of the matrix's samples */
	long long ignored = 0;                           /* lines that name no sample of the matrix */
};

struct HuMetaVar {
	bool numeric = false;
	std::vector<double> value;                       /* numeric: [n] */
	std::vector<int32_t> label;                      /* categorical: [n], levels in order of first appearance */
	std::vector<std::string> level;
};

inline void hu_meta_split(const std::string& line, char sep, std::vector<std::string>& f) {
	f.clear();
	size_t b = 0;
	for(;;) {
		const size_t e = line.find(sep, b);
		f.push_back(line.substr(b, e == std::string::npos ? e : e - b));
		if(e == std::string::npos) break;
		b = e + 1;
	}
}

/* reads `path` against the samples of the matrix (sample [n]); false: refused, err says why */
inline bool hu_meta_read(const std::string& path, const std::vector<std::string>& sample, HuMeta& m, std::string& err) {
	std::ifstream in(path);
	if(!in) { err = "Unable to open design file '" + path + "'"; return false; }
	std::map<std::string, size_t> at;
	for(size_t i = 0; i < sample.size(); ++i) at[sample[i]] = i;
	m.column.clear(); m.value.assign(sample.size(), std::vector<std::string>()); m.ignored = 0;
	std::vector<char> seen(sample.size(), 0);
	std::string line; std::vector<std::string> f; long long ln = 0; bool header = false;
	while(std::getline(in, line)) {
		++ln;
		if(!line.empty() && line.back() == '\r') line.pop_back();
		if(line.empty()) continue;
		if(!header) {
			if(line[0] == '#') line.erase(0, 1);
			hu_meta_split(line, '\t', f);
			if(f.size() < 2) { err = path + ": line " + std::to_string(ln) + ": the header names the sample column and one variable at the least"; return false; }
			m.column.assign(f.begin() + 1, f.end());
			for(size_t a = 0; a < m.column.size(); ++a) for(size_t b = 0; b < a; ++b) if(m.column[a] == m.column[b]) {
				err = path + ": line " + std::to_string(ln) + ": column '" + m.column[a] + "' is named twice"; return false; }
			header = true;
			continue;
		}
		if(line[0] == '#') continue;
		hu_meta_split(line, '\t', f);
		if(f.size() != m.column.size() + 1) {
			err = path + ": line " + std::to_string(ln) + ": " + std::to_string(f.size()) + " fields where the header has " + std::to_string(m.column.size() + 1); return false; }
		const auto it = at.find(f[0]);
		if(it == at.end()) { ++m.ignored; continue; }
		if(seen[it->second]) { err = "Sample '" + f[0] + "' is named twice in '" + path + "'"; return false; }
		seen[it->second] = 1;
		m.value[it->second].assign(f.begin() + 1, f.end());
	}
	if(!header) { err = path + ": no header line"; return false; }
	for(size_t i = 0; i < sample.size(); ++i) if(!seen[i]) { err = "Sample '" + sample[i] + "' of the matrix has no line in '" + path + "'"; return false; }
	return true;
}

/* the column `name` as a variable: numeric when every value parses as a finite double and `factor` is not set; false: no such column,
 * or an empty or NA value (by sample and column) */
inline bool hu_meta_variable(const HuMeta& m, const std::vector<std::string>& sample, const std::string& name, bool factor, HuMetaVar& v, std::string& err) {
	size_t c = 0;
	while(c < m.column.size() && m.column[c] != name) ++c;
	if(c == m.column.size()) { err = "'" + name + "' is no column of the design file"; return false; }
	const size_t n = sample.size();
	v = HuMetaVar();
	v.numeric = !factor;
	v.value.assign(n, 0.0);
	for(size_t i = 0; i < n; ++i) {
		const std::string& s = m.value[i][c];
		if(s.empty() || s == "NA") { err = "Sample '" + sample[i] + "' has " + (s.empty() ? "an empty" : "the NA") + " value in column '" + name + "'"; return false; }
		if(v.numeric) {
			char* end = nullptr;
			const double x = strtod(s.c_str(), &end);
			if(end == s.c_str() || *end || !std::isfinite(x)) v.numeric = false; else v.value[i] = x;
		}
	}
	if(v.numeric) return true;
	v.value.clear();
	std::map<std::string, int32_t> id;
	v.label.resize(n);
	for(size_t i = 0; i < n; ++i) {
		auto it = id.find(m.value[i][c]);
		if(it == id.end()) { it = id.emplace(m.value[i][c], (int32_t) v.level.size()).first; v.level.push_back(m.value[i][c]); }
		v.label[i] = it->second;
	}
	return true;
}
