// hmmufotu-amd-sim: simulated single or paired-end reads with a known answer from a built database — hmmufotu-sim
// (src/hmmufotu-sim.cpp:97-425).  Every read is a random point on a random branch of the tree; its bases are drawn column by column
// from the tree's own messages at that point, its gaps from the weighted gap fraction of the alignment, and its FASTA header records
// the branch, the nearer node and the consensus range.  The host draws branch, point and columns (hu_sim_plan); the sites of a whole
// batch of reads are drawn on the device, where the messages are (hu_sim_reads).  Options are checked, the inputs found and the
// outputs opened before a device is asked for; an output this run created is removed again when the run fails.
//   hmmufotu-amd-sim <HmmUFOtu-DB> <SEQ-OUT> [MATE-OUT] -N NUM [-k] [-d DBL] [-m DBL] [-s DBL] [-l DBL] [-u DBL] [-r INT] [-R BED]
//                    [--prefix STR] [-S INT] [-f fasta] [--msa FILE] [--batch N] [--device N] [-v]
// Only <DB>.hmm and <DB>.ptu are read: there is no reader of the reference's binary <DB>.msa here.  The gap fractions come from the
// leaf rows the .ptu keeps, or from the alignment the database was built from when --msa names it (FASTA, .gz / .bz2).
// Deviations from the reference: the random streams (Philox here, Boost's mt11213b there; the distributions are the same);
// --sd-size is read (the reference tests for "--sd-len" and then reads "--sd-size", :169-170, so neither spelling works there); a BED
// line that ends at the consensus length is dropped (the reference would read one column past the alignment); -S takes 64 bits.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cerrno>
#include <cstring>
#include <ctime>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "hu_reads_io.h"
#include "../../include/hmmufotu_amd.h"

static const auto unused_revcom [[maybe_unused]] = &revcom;     /* hu_reads_io.h is shared with the programs that read primers */

static void usage(const char* p) {
	std::cerr << "Usage:    " << p << "  <HmmUFOtu-DB> <SEQ-OUT> [MATE-OUT] <-N NUM-READS> [options]\n"
		"Options:    SEQ-OUT  FILE       : READ OUTPUT in FASTA format\n"
		"            MATE-OUT  FILE      : optional MATE OUTPUT in FASTA format, ignored if -k|--keep-gap is set\n"
		"            -N  LONG            : number of reads/pairs to generate\n"
		"            -f|--fmt  STRING    : output format [fasta]\n"
		"            -k|--keep-gap FLAG  : keep simulated gaps in generated reads, so final seq will be aligned\n"
		"            -d|--max-dist       : maximum height allowed for simulated reads (as shorted phylogenetic distance to any leaf) [inf]\n"
		"            -m|--mean-size  DBL : mean 16S amplicon size [500]\n"
		"            -s|--sd-size  DBL   : standard deviation of 16S amplicon size [30]\n"
		"            -l|--min-size  DBL  : minimum 16S amplicon size, 0 for no limit [0]\n"
		"            -u|--max-size  DBL  : maximum 16S amplicon size, 0 for no limit [0]\n"
		"            -r|--read-len  INT  : read length for generating single/paired-end reads, set to -1 to use the actual amplicon size [-1]\n"
		"            -R|--region  STRING : BED file for restricted consensus region where simulated reads should be drawn; setting this will ignore -m,-s,-l,-u togather\n"
		"            --prefix STRING  : prefix for random read IDs [r]\n"
		"            -S|--seed  INT      : random seed used for simulation, for debug purpose\n"
		"            --msa  FILE         : the alignment the database was built from (FASTA, .gz / .bz2), for the gap fractions; without it they\n"
		"                                  come from the leaf rows of <DB>.ptu.  Only <DB>.hmm and <DB>.ptu are read: <DB>.msa has no reader here\n"
		"            --batch  INT        : reads per device launch [65536]\n"
		"            --device  INT       : device index [0]\n"
		"            -v  FLAG            : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help           : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string regionFn, prefix = "r", fmt = "fasta", msaFn;
	bool keepGap = false, haveN = false;
	long N = 0; int readLen = -1, verbose = 0, device = 0; long batch = 65536;
	hu_sim_opts so; hu_sim_default_opts(&so);
	uint64_t seed = (uint64_t) time(nullptr);
	if(argc == 1) { std::cerr << "Generate simulated single or paired-end NGS reads, aligned or un-aligned, using a pre-built HmmUFOtu database" << std::endl; usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { std::cerr << "Generate simulated single or paired-end NGS reads, aligned or un-aligned, using a pre-built HmmUFOtu database" << std::endl; usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and simulation semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-N") { N = atol(val()); haveN = true; }
		else if(a == "-k" || a == "--keep-gap") keepGap = true;
		else if(a == "-d" || a == "--max-dist") so.max_dist = atof(val());
		else if(a == "-m" || a == "--mean-size") so.mean_size = atof(val());
		else if(a == "-s" || a == "--sd-size") so.sd_size = atof(val());
		else if(a == "-l" || a == "--min-size") so.min_size = atof(val());
		else if(a == "-u" || a == "--max-size") so.max_size = atof(val());
		else if(a == "-r" || a == "--read-len") readLen = atoi(val());
		else if(a == "-R" || a == "--region") regionFn = val();
		else if(a == "--prefix") prefix = val();
		else if(a == "-S" || a == "--seed") seed = strtoull(val(), nullptr, 10);
		else if(a == "-f" || a == "--fmt") fmt = val();
		else if(a == "--msa") msaFn = val();
		else if(a == "--batch") batch = atol(val());
		else if(a == "--device") device = atoi(val());
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(!((pos.size() == 2 || pos.size() == 3) && haveN)) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	auto info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	const std::string dbName = pos[0], outFn = pos[1], mateFn = pos.size() == 3 ? pos[2] : "";
	/* validate options (src/hmmufotu-sim.cpp:203-223; the -m message names --min-size there too) */
	if(!(N > 0)) { std::cerr << "-N must be positive" << std::endl; return EXIT_FAILURE; }
	if(!(so.mean_size > 0)) { std::cerr << "-m|--min-size must be positive" << std::endl; return EXIT_FAILURE; }
	if(!(so.sd_size > 0)) { std::cerr << "-s|--sd-size must be positive" << std::endl; return EXIT_FAILURE; }
	if(!(so.min_size >= 0)) { std::cerr << "-l|--min-size must be non-negative" << std::endl; return EXIT_FAILURE; }
	if(!(so.max_size >= 0 && so.max_size >= so.min_size)) { std::cerr << "-u|--max-size must be non-negative and non-less than -l|--min-size" << std::endl; return EXIT_FAILURE; }
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }
	if(batch < 1 || batch > (1 << 22)) { std::cerr << "--batch must be in [1, 4194304]" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative" << std::endl; return EXIT_FAILURE; }

	/* open inputs */
	const std::string hmmFn = dbName + ".hmm", ptuFn = dbName + ".ptu";
	for(const std::string& fn : {hmmFn, ptuFn}) { std::ifstream in(fn, std::ios::binary); if(!in.is_open()) { std::cerr << "Unable to open " << fn << " : " << strerror(errno) << std::endl; return EXIT_FAILURE; } }
	std::vector<int32_t> bed;
	std::ifstream regionIn;
	if(!regionFn.empty()) { regionIn.open(regionFn); if(!regionIn.is_open()) { std::cerr << "Unable to open " << regionFn << " : " << strerror(errno) << std::endl; return EXIT_FAILURE; } }
	std::vector<char> msa; size_t msaRows = 0, msaLen = 0;     /* the rows as read, case kept */
	if(!msaFn.empty()) {
		LineIn seqIn;
		if(!seqIn.open(msaFn)) { std::cerr << "Unable to open " << msaFn << " : " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		Read r;
		while(next_read(seqIn, false, r, true)) {
			if(msaRows == 0) msaLen = r.seq.size();
			else if(r.seq.size() != msaLen) { std::cerr << "Unable to load MSA from '" << msaFn << "': sequence '" << r.id << "' has " << r.seq.size() << " columns, the first one " << msaLen << std::endl; return EXIT_FAILURE; }
			msa.insert(msa.end(), r.seq.begin(), r.seq.end());
			++msaRows;
		}
		if(msaRows == 0 || msaLen == 0) { std::cerr << "Unable to load MSA from '" << msaFn << "'" << std::endl; return EXIT_FAILURE; }
		info("MSA data loaded, numSeq: " + std::to_string(msaRows) + " csLen:" + std::to_string(msaLen));
	}

	/* open outputs; a file that was not there before is removed again if the run fails */
	auto existed = [](const std::string& fn) { std::ifstream in(fn); return in.is_open(); };
	if(!mateFn.empty()) keepGap = false;     /* suppress -k if paired end */
	const bool hadOut = existed(outFn), hadMate = !mateFn.empty() && existed(mateFn);
	std::ofstream seqOut, mateOut;
	bool madeOut = false, madeMate = false;
	auto fail = [&](const std::string& msg) {
		if(!msg.empty()) std::cerr << msg << std::endl;
		if(seqOut.is_open()) seqOut.close();
		if(mateOut.is_open()) mateOut.close();
		if(madeOut && !hadOut) remove(outFn.c_str());
		if(madeMate && !hadMate) remove(mateFn.c_str());
		return EXIT_FAILURE;
	};
	seqOut.open(outFn);
	if(!seqOut.is_open()) return fail("Unable to write seq to '" + outFn + "' : " + strerror(errno));
	madeOut = true;
	if(!mateFn.empty()) {
		mateOut.open(mateFn);
		if(!mateOut.is_open()) return fail("Unable to write mate to '" + mateFn + "' : " + strerror(errno));
		madeMate = true;
	}

	/* load input database */
	if(hu_device_count() <= device) return fail("Error: device " + std::to_string(device) + " asked for, " + std::to_string(hu_device_count()) + " gfx950 device(s) visible");
	hu_db* db = nullptr;
	if(hu_db_load(hmmFn.c_str(), ptuFn.c_str(), device, &db) != HU_OK) return fail("Failed to load PTU data from " + ptuFn + ": " + hu_last_error());
	struct DbGuard { hu_db* h; ~DbGuard() { hu_db_destroy(h); } } dbGuard{db};
	int32_t csLen = 0, nNodes = 0;
	hu_db_info(db, nullptr, &csLen, &nNodes, nullptr, nullptr);
	info("Phylogenetic tree data loaded, numNode: " + std::to_string(nNodes) + " numSites:" + std::to_string(csLen));
	std::vector<int32_t> parent((size_t) nNodes); std::vector<double> blen((size_t) nNodes), height((size_t) nNodes);
	if(hu_db_get_tree(db, parent.data(), blen.data(), nullptr, height.data()) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
	std::vector<double> gapFrac((size_t) csLen);
	if(hu_sim_gap_frac(db, (int64_t) msaRows, (int64_t) msaLen, msaFn.empty() ? nullptr : msa.data(), gapFrac.data()) != HU_OK) {
		if(!msaFn.empty()) std::cerr << "Unmatched HmmUFOtu data files, please rebuild your database" << std::endl;
		return fail(std::string("Error: ") + hu_last_error());
	}
	std::vector<char>().swap(msa);

	/* read restricted regions, if provided (:294-310) */
	if(regionIn.is_open()) {
		std::string line;
		while(std::getline(regionIn, line)) {
			std::vector<std::string> f; size_t b = 0;
			for(;;) { const size_t t = line.find('\t', b); f.push_back(line.substr(b, t == std::string::npos ? t : t - b)); if(t == std::string::npos) break; b = t + 1; }
			if(f.size() < 3) continue;
			char *e1 = nullptr, *e2 = nullptr;
			const long s = strtol(f[1].c_str(), &e1, 10), e = strtol(f[2].c_str(), &e2, 10);
			if(f[1].empty() || f[2].empty() || *e1 || *e2) return fail("Region file " + regionFn + ": '" + f[1] + "' / '" + f[2] + "' is not a pair of integers");
			if(s < INT32_MIN || s > INT32_MAX || e < INT32_MIN || e > INT32_MAX || !hu_sim_region_ok((int32_t) s, (int32_t) e, csLen)) {
				std::cerr << "Region (" << s << "," << e << "] is not in the consensus range, ignored" << std::endl;
				continue;
			}
			bed.push_back((int32_t) s); bed.push_back((int32_t) e);
		}
		info("Read in " + std::to_string(bed.size() / 2) + " restricted regions");
	}
	so.n_regions = (int64_t) bed.size() / 2; so.regions = bed.data();

	/* PTUNode::getTaxon() with its default maxDist = inf (src/PhyloTreeUnrooted.h:1580-1582) */
	auto taxon = [&](int32_t u) { std::string t = hu_db_get_annotation(db, u); double ad = 0; hu_db_get_anno_dist(db, u, &ad); if(!(ad <= INFINITY)) t += ";Other"; return t; };

	info(mateFn.empty() ? "Simulating single-end reads" : "Simulating paired-end reads");
	const size_t B = (size_t) std::min<long>(batch, N);
	std::vector<int32_t> node(B), st(B), en(B), seqLen(B); std::vector<double> rc(B);
	std::vector<char> aligned, seq, mate, desc;
	std::string rec, out, mout;
	int64_t attempt = 0;
	const bool wantMate = !mateFn.empty();
	for(long n0 = 0; n0 < N; n0 += (long) B) {
		const int64_t m = std::min<long>((long) B, N - n0);
		if(hu_sim_plan(nNodes, csLen, parent.data(), blen.data(), height.data(), &so, seed, &attempt, m, node.data(), rc.data(), st.data(), en.data()) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
		size_t total = 0;
		for(int64_t r = 0; r < m; ++r) total += (size_t)(en[r] - st[r] + 1);
		aligned.resize(total); seq.resize(total); if(wantMate) mate.resize(total);
		if(hu_sim_reads(db, m, node.data(), rc.data(), st.data(), en.data(), gapFrac.data(), seed, (uint64_t) n0, wantMate, aligned.data(), seq.data(), wantMate ? mate.data() : nullptr, seqLen.data()) != HU_OK)
			return fail(std::string("Error: ") + hu_last_error());
		out.clear(); mout.clear();
		size_t off = 0;
		for(int64_t r = 0; r < m; ++r) {
			const size_t cols = (size_t)(en[r] - st[r] + 1);
			if(keepGap) { rec.assign((size_t) st[r], '.'); rec.append(aligned.data() + off, cols); rec.append((size_t)(csLen - 1 - en[r]), '.'); }
			else rec.assign(seq.data() + off, (size_t) seqLen[r]);
			const int32_t c = node[r], p = parent[c];
			const std::string tc = taxon(c), tp = taxon(p);
			const int64_t need = hu_sim_description(c, p, tc.c_str(), tp.c_str(), rc[r], st[r], en[r], (int64_t) rec.size(), nullptr, 0);
			if(need < 0) return fail(std::string("Error: ") + hu_last_error());
			desc.resize((size_t) need + 1);
			hu_sim_description(c, p, tc.c_str(), tp.c_str(), rc[r], st[r], en[r], (int64_t) rec.size(), desc.data(), (int64_t) desc.size());
			const std::string head = ">" + prefix + std::to_string(n0 + r + 1) + " " + desc.data() + "\n";
			/* PrimarySeq::trunc(0, readLen): a negative length keeps everything */
			const size_t cut = readLen < 0 ? std::string::npos : (size_t) readLen;
			out += head; out.append(rec, 0, cut); out += '\n';
			if(wantMate) { mout += head; mout.append(mate.data() + off, std::min((size_t) seqLen[r], cut)); mout += '\n'; }
			off += cols;
		}
		seqOut.write(out.data(), (std::streamsize) out.size());
		if(wantMate) mateOut.write(mout.data(), (std::streamsize) mout.size());
		if(!seqOut || (wantMate && !mateOut)) return fail(std::string("Unable to write reads: ") + strerror(errno));
		if(verbose > 1) std::cerr << (n0 + m) << " reads simulated" << std::endl;
	}
	seqOut.flush(); if(wantMate) mateOut.flush();
	if(!seqOut || (wantMate && !mateOut)) return fail(std::string("Unable to write reads: ") + strerror(errno));
	return EXIT_SUCCESS;
}
