// The GROUPS file of hmmufotu-amd-permanova and hmmufotu-amd-diffabund: lines of sample<TAB>group; lines that start with '#' and empty
// lines are skipped, and so are lines that name no sample of the input.  Header only, for the programs: refusals go to stderr.
#pragma once
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

/* reads `path` against the n samples of the input (`at`: name -> index; `what`: "matrix" or "table"): seen[i] whether sample i has a
 * line, groupOf[i] its group.  false: refused, and said why */
inline bool hu_groups_read(const std::string& path, int64_t n, const std::map<std::string, int64_t>& at, const char* what, bool verbose,
		std::vector<std::string>& groupOf, std::vector<char>& seen) {
	groupOf.assign((size_t) n, std::string()); seen.assign((size_t) n, 0);
	std::ifstream in(path);
	if(!in) { std::cerr << "Unable to open group file '" << path << "'" << std::endl; return false; }
	std::string line; long long ln = 0, ignored = 0;
	while(std::getline(in, line)) {
		++ln;
		if(!line.empty() && line.back() == '\r') line.pop_back();
		if(line.empty() || line[0] == '#') continue;
		const size_t tab = line.find('\t');
		if(tab == std::string::npos || tab == 0 || tab + 1 >= line.size() || line.find('\t', tab + 1) != std::string::npos) {
			std::cerr << path << ": line " << ln << ": expected sample<TAB>group" << std::endl; return false; }
		const auto it = at.find(line.substr(0, tab));
		if(it == at.end()) { ++ignored; continue; }
		if(seen[(size_t) it->second]) { std::cerr << "Sample '" << it->first << "' is named twice in '" << path << "'" << std::endl; return false; }
		seen[(size_t) it->second] = 1; groupOf[(size_t) it->second] = line.substr(tab + 1);
	}
	if(verbose) std::cerr << ignored << " line(s) of '" << path << "' name no sample of the " << what << std::endl;
	return true;
}

/* the labels of the kept samples, groups numbered in order of first appearance among them; gname [a] receives the groups' names */
inline std::vector<int32_t> hu_groups_label(const std::vector<std::string>& groupOf, const std::vector<int64_t>& kept, std::vector<std::string>& gname) {
	std::map<std::string, int32_t> gid;
	std::vector<int32_t> label(kept.size());
	gname.clear();
	for(size_t k = 0; k < kept.size(); ++k) {
		const std::string& g = groupOf[(size_t) kept[k]];
		auto it = gid.find(g);
		if(it == gid.end()) { it = gid.emplace(g, (int32_t) gname.size()).first; gname.push_back(g); }
		label[k] = it->second;
	}
	return label;
}
