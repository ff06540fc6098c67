// The inputs of the programs that start from a reference MSA and its tree (hmmufotu-amd-build, hmmufotu-amd-train-sm; hmmufotu-amd-train-hmm
// takes the MSA alone): what
// src/hmmufotu-build.cpp:198-208, :346-392 and src/hmmufotu-train-sm.cpp:133-229 do before the model is used.  The FASTA reader
// (.gz / .bz2), hu_newick_parse with the reference's node ids and file-order children, the join of leaves and rows by name with the
// reference's messages (PTUnrooted::loadMSA, src/PhyloTreeUnrooted.cpp:185-221), and MSA::prune (src/MSA.cpp:87-138) behind
// hu_msa_stats with the encoding of hu_msa_encode_table.  Everything up to the join runs without a device; the prune asks for one.
// Every function prints its refusal on stderr as one line and returns false.
#pragma once
#include <cerrno>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>
#include "hu_reads_io.h"
#include "../../include/hmmufotu_amd.h"

static const auto unused_revcom [[maybe_unused]] = &revcom;     /* hu_reads_io.h is shared with the programs that read primers */
static bool ends_with(const std::string& s, const char* suf) { const size_t k = strlen(suf); return s.size() >= k && s.compare(s.size() - k, k, suf) == 0; }
static bool read_file(const std::string& fn, std::string& out) {
	std::ifstream in(fn, std::ios::binary);
	if(!in.is_open()) return false;
	std::ostringstream ss; ss << in.rdbuf(); out = ss.str();
	return !in.bad();
}

typedef std::function<void(const std::string&)> HuInfo;     /* the programs' verbose line */

struct HuBuildInputs {
	/* the MSA: rows as read (case kept), names = the ids */
	std::vector<std::string> rowName; std::vector<char> msa; size_t L0 = 0, nSeq = 0;
	std::unordered_map<std::string, uint32_t> name2row;
	/* the tree, as hu_newick_get returns it */
	int32_t n = 0;
	std::vector<int32_t> parent, childOff, childIdx; std::vector<double> blen; std::vector<std::string> nodeName;
	/* the join: every leaf's MSA row, -1 for the other nodes */
	std::vector<int32_t> rowOf;
	/* the prune: the columns kept, and the counts of hu_msa_stats over the columns as read */
	std::vector<uint32_t> keep; int32_t L = 0;
	std::vector<int32_t> res, gap; std::vector<double> wres, wgap;
	/* per row, from the same call: first / last residue column as read (-1: none) and the normalised sequence weight */
	std::vector<int32_t> start, end; std::vector<double> weight;
};

/* guess input format (src/hmmufotu-build.cpp:198-208) */
static void hu_guess_seq_format(const std::string& seqFn, std::string& fmt) {
	if(!fmt.empty()) return;
	std::string pre = seqFn;
	if(ends_with(pre, ".gz")) pre.erase(pre.size() - 3); else if(ends_with(pre, ".bz2")) pre.erase(pre.size() - 4);
	for(const char* e : {"fasta", "fas", "fa", "fna"}) if(ends_with(pre, e)) fmt = "fasta";
	if(fmt.empty()) for(const char* e : {"fastq", "fq"}) if(ends_with(pre, e)) fmt = "fastq";
}
static bool hu_is_newick_name(const std::string& treeFn) { return ends_with(treeFn, ".tree") || ends_with(treeFn, ".tre"); }

/* the MSA: rows as read (case kept), names = the ids.  msaName: what the reference calls the MSA in its message */
static bool hu_load_msa(LineIn& seqIn, const std::string& seqFn, const std::string& msaName, HuBuildInputs& in, const HuInfo& info) {
	Read r;
	while(next_read(seqIn, false, r, true)) {
		if(in.rowName.empty()) in.L0 = r.seq.size();
		else if(r.seq.size() != in.L0) { std::cerr << "Unable to load MSA from '" << seqFn << "': sequence '" << r.id << "' has " << r.seq.size() << " columns, the first one " << in.L0 << std::endl; return false; }
		if(!in.name2row.insert({r.id, (uint32_t) in.rowName.size()}).second) { std::cerr << "Non-unique seq name " << r.id << " found in your MSA data " << msaName << std::endl; return false; }
		in.rowName.push_back(r.id);
		in.msa.insert(in.msa.end(), r.seq.begin(), r.seq.end());
	}
	if(in.rowName.empty() || in.L0 == 0) { std::cerr << "Unable to load MSA from '" << seqFn << "'" << std::endl; return false; }
	in.nSeq = in.rowName.size();
	info("MSA loaded");
	return true;
}

/* the tree */
static bool hu_load_tree(const std::string& treeText, const std::string& treeFn, HuBuildInputs& in, const HuInfo& info) {
	hu_newick* nw = nullptr;
	if(hu_newick_parse(treeText.data(), (int64_t) treeText.size(), &nw) != HU_OK) { std::cerr << "Unable to read Newick tree in '" << treeFn << "': " << hu_last_error() << std::endl; return false; }
	info("Newick Tree read");
	int32_t n = 0;
	hu_newick_size(nw, &n);
	in.n = n;
	in.parent.resize(n); in.childOff.resize((size_t) n + 1); in.childIdx.resize((size_t) std::max(n - 1, 1)); in.blen.resize(n);
	hu_newick_get(nw, in.parent.data(), in.blen.data(), in.childOff.data(), in.childIdx.data());
	in.nodeName.resize(n);
	for(int32_t i = 0; i < n; ++i) in.nodeName[i] = hu_newick_name(nw, i);
	hu_newick_free(nw);
	info("Phylogenetic Tree constructed with total " + std::to_string(n) + " nodes");
	return true;
}

/* loadMSA (src/PhyloTreeUnrooted.cpp:185-221): every leaf takes the row of its name */
static bool hu_join_msa_tree(HuBuildInputs& in, const HuInfo& info) {
	in.rowOf.assign(in.n, -1);
	size_t nLeaves = 0, nRead = 0;
	for(int32_t i = 0; i < in.n; ++i) if(in.childOff[i] == in.childOff[i + 1]) {
		++nLeaves;
		auto it = in.name2row.find(in.nodeName[i]);
		if(it != in.name2row.end()) { in.rowOf[i] = (int32_t) it->second; ++nRead; }
	}
	if(nRead != nLeaves) { std::cerr << "Unmatched MSA and Tree. Found " << nRead << " leaf sequences from MSA but expecting " << nLeaves << " leaves in the Phylogenetic Tree " << std::endl; return false; }
	info("MSA loaded into Phylogenetic Tree");
	return true;
}

/* MSA::prune: the columns without a residue go (hu_msa_stats counts them on the device).  err: the library's message on failure */
static bool hu_prune_msa(int device, HuBuildInputs& in, const HuInfo& info, std::string& err) {
	const size_t L0 = in.L0, nSeq = in.nSeq;
	in.res.resize(4 * L0); in.gap.resize(L0); in.wres.resize(4 * L0); in.wgap.resize(L0);
	std::vector<int32_t> ln(nSeq);
	in.start.resize(nSeq); in.end.resize(nSeq); in.weight.resize(nSeq);
	if(hu_msa_stats(device, (int64_t) nSeq, (int64_t) L0, in.msa.data(), in.res.data(), in.gap.data(), in.start.data(), in.end.data(), ln.data(), in.weight.data(), in.wres.data(), in.wgap.data()) != HU_OK) {
		err = hu_last_error(); return false;
	}
	in.keep.clear();
	for(size_t j = 0; j < L0; ++j) if(in.res[j] + in.res[L0 + j] + in.res[2 * L0 + j] + in.res[3 * L0 + j] > 0) in.keep.push_back((uint32_t) j);
	in.L = (int32_t) in.keep.size();
	info("MSA pruned");
	info("MSA database created for " + std::to_string(nSeq) + " X " + std::to_string(in.L) + " aligned sequences");
	return true;
}

/* one row of the pruned MSA in the codes of hu_msa_encode_table (enc [256]) */
static void hu_encode_row(const HuBuildInputs& in, const int8_t* enc, size_t row, int8_t* dst) {
	const char* src = in.msa.data() + row * in.L0;
	for(int32_t j = 0; j < in.L; ++j) dst[j] = enc[(unsigned char) src[in.keep[j]]];
}
