// hmmufotu-amd-anneal — primer coverage of a database, with the option surface and output of the reference's `hmmufotu-anneal`
// (src/hmmufotu-anneal.cpp).  Host C++ only: option parsing, FASTA reading, strand choice and the TSV; the primers' Viterbi alignment
// (hu_align_batch, GLOBAL mode, no seeds) and the scan of every node (hu_anneal_batch) run on the device, a batch of primers at a time.
// Differences from the reference: only <DB>.hmm and <DB>.ptu are read (there is no seed lookup, so neither the .msa nor the .csfm is
// needed); a primer with no alignment (the reference asserts) gets no line, a warning on stderr, and the program exits non-zero after the
// last line.  Primers keep the case they were read in, as SeqIO keeps it: the report prints them so, the reverse strand is complemented
// case by case, and a matched lower-case base is lower-case in the alignment (an invalid symbol for the scan) as in the reference.  The
// Viterbi scores use the upper-cased bases: the reference indexes its emission table with the code -1 of a lower-case base there.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"
#include "hu_reads_io.h"

static void usage(const char* p) {
	std::cerr << "Anneal primer sequences to an HmmUFOtu database and evaluate the primer efficiency" << std::endl
		<< "Usage:    " << p << "  <HmmUFOtu-DB> <SEQ-FILE> [options]" << std::endl
		<< "SEQ-FILE  FILE                 : primer sequence read file in fasta format, degenerated bases are allowed" << std::endl
		<< "Options:    -o  FILE           : write the PLACEMENT output to FILE instead of stdout" << std::endl
		<< "            -i|--identity  DBL : minimum identity between aligned primer sequence and an OTU sequence considered as a good hit [0.9]" << std::endl
		<< "            -s|--strand  INT   : strand orientation for primers, 1 for forward, 2 for reverse, 3 for auto-detect by best alignment [3]" << std::endl
		<< "            -v  FLAG           : enable verbose information, you may set multiple -v for more details" << std::endl
		<< "            --batch  INT       : primers per device batch [4096]" << std::endl
		<< "            --gpu  INT         : device index [0]" << std::endl
		<< "            --version          : show program version and exit" << std::endl
		<< "            -h|--help          : print this message and exit" << std::endl;
}

static std::string fmt_g(double x) { char b[64]; snprintf(b, sizeof b, "%g", x); return b; }   /* ostream's default format */

int main(int argc, char** argv) {
	std::vector<std::string> pos;
	std::string outFn;
	double maxDist = 1 - 0.9;
	int strand = 3, batch = 4096, gpu = 0, verbose = 0;
	if(argc == 1) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and anneal semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val();
		else if(a == "-i" || a == "--identity") maxDist = 1 - atof(val());
		else if(a == "-s" || a == "--strand") strand = atoi(val());
		else if(a == "-v") verbose++;
		else if(a == "--batch") batch = atoi(val());
		else if(a == "--gpu") gpu = atoi(val());
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	/* validation as src/hmmufotu-anneal.cpp:126-133 */
	if(!(maxDist >= 0)) { std::cerr << "-i|--identity must between 0 and 1" << std::endl; return EXIT_FAILURE; }
	if(!(1 <= strand && strand <= 3)) { std::cerr << "-s|--strand must be 1, 2 or 3" << std::endl; return EXIT_FAILURE; }
	if(batch < 1 || batch > (1 << 20)) { std::cerr << "--batch must be in [1, 1048576]" << std::endl; return EXIT_FAILURE; }

	LineIn in;
	if(!in.open(pos[1])) { std::cerr << "Unable to open seq file '" << pos[1] << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	std::ofstream of;
	if(!outFn.empty()) {
		of.open(outFn);
		if(!of.is_open()) { std::cerr << "Unable to write to '" << outFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	}
	std::ostream& out = of.is_open() ? of : std::cout;

	if(hu_device_count() <= gpu) { std::cerr << "Error: device " << gpu << " asked for, " << hu_device_count() << " gfx950 device(s) visible" << std::endl; return EXIT_FAILURE; }
	hu_db* db = nullptr;
	if(hu_db_load((pos[0] + ".hmm").c_str(), (pos[0] + ".ptu").c_str(), gpu, &db) != HU_OK) { std::cerr << "Unable to load database '" << pos[0] << "': " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	int32_t K = 0, L = 0, nNodes = 0;
	int64_t nLeaves = 0;
	hu_db_info(db, &K, &L, &nNodes, nullptr, nullptr);
	hu_db_num_leaves(db, &nLeaves);
	if(verbose) std::cerr << "Database loaded: " << nNodes << " nodes, " << nLeaves << " leaves, CS length " << L << std::endl;
	const int rowsPer = (strand & 1) + ((strand >> 1) & 1);
	hu_batch* b = nullptr;
	if(hu_batch_create(db, batch * rowsPer, &b) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; hu_db_destroy(db); return EXIT_FAILURE; }
	hu_opts o; hu_default_opts(&o);
	o.align_mode = HU_MODE_GLOBAL;       /* hmm.setSequenceMode(GLOBAL); the engine's profile is wing-retracted at load */

	out << hu_anneal_header() << "\n";
	int64_t nFailed = 0, nDone = 0;
	bool more = true;
	std::vector<Read> prim;
	std::vector<hu_align_rec> recs;
	std::vector<char> rows;
	while(more) {
		prim.clear();
		Read r;
		while((int) prim.size() < batch && (more = next_read(in, false, r, true))) prim.push_back(r);
		const int n = (int) prim.size();
		if(n == 0) break;
		/* rows: the forward primers first (-s & 1), then their reverse complements (-s & 2) */
		std::string cat; std::vector<int64_t> offs(1, 0);
		std::vector<std::string> text;      /* each row as read: the primer, or its reverse complement with the case of each letter kept */
		for(int pass = 0; pass < 2; ++pass) {
			if(!(strand & (1 << pass))) continue;
			for(const Read& p : prim) {
				text.push_back(pass ? revcom(p.seq) : p.seq);
				for(char c : text.back()) cat += (char) toupper((unsigned char) c);
				offs.push_back((int64_t) cat.size());
			}
		}
		const int nRows = n * rowsPer;
		std::vector<int32_t> chosen(n, -1);
		std::vector<char> strandCh(n, '.');
		std::vector<int64_t> hitN(n), hitL(n);
		if(hu_batch_set_reads(b, nRows, cat.data(), offs.data(), nullptr, nullptr, nullptr, nullptr) != HU_OK || hu_align_batch(b, &o) != HU_OK) {
			std::cerr << "Error: " << hu_last_error() << std::endl; hu_batch_destroy(b); hu_db_destroy(db); return EXIT_FAILURE;
		}
		recs.resize(nRows); rows.resize((size_t) nRows * L);
		if(hu_batch_get_alignments(b, recs.data(), nullptr, nullptr, 0) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; hu_batch_destroy(b); hu_db_destroy(db); return EXIT_FAILURE; }
		for(int i = 0; i < n; ++i) { /* src/hmmufotu-anneal.cpp:249-265: a row with no alignment has cost +inf */
			double minCost = INFINITY;
			int row = 0;
			if(strand & 1) {
				strandCh[i] = '+';
				if(recs[i].status == HU_READ_OK) { chosen[i] = i; minCost = recs[i].cost; }
				row = n;
			}
			if(strand & 2) {
				const int rr = row + i;
				if(recs[rr].status == HU_READ_OK && recs[rr].cost < minCost) { strandCh[i] = '-'; chosen[i] = rr; }
			}
		}
		std::vector<const char*> asRead(n, nullptr);
		for(int i = 0; i < n; ++i) if(chosen[i] >= 0) asRead[i] = text[chosen[i]].c_str();
		/* the rows take the case of the text here: fetched after the scan */
		if(hu_anneal_batch(b, chosen.data(), n, asRead.data(), maxDist, hitN.data(), hitL.data()) != HU_OK ||
		   hu_batch_get_alignments(b, nullptr, rows.data(), nullptr, 0) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; hu_batch_destroy(b); hu_db_destroy(db); return EXIT_FAILURE; }
		std::string txt;
		for(int i = 0; i < n; ++i) {
			if(chosen[i] < 0) { std::cerr << "Warning: primer '" << prim[i].id << "' has no alignment to the profile; no line written" << std::endl; ++nFailed; continue; }
			const hu_align_rec& a = recs[chosen[i]];
			txt += prim[i].id; txt += '\t'; txt += prim[i].desc; txt += '\t'; txt += prim[i].seq; txt += '\t'; txt += strandCh[i]; txt += '\t';
			txt += std::to_string(a.cs_start); txt += '\t'; txt += std::to_string(a.cs_end); txt += '\t';
			txt.append(rows.data() + (size_t) chosen[i] * L + (a.cs_start - 1), (size_t)(a.cs_end - a.cs_start + 1)); txt += '\t';
			txt += std::to_string(nNodes); txt += '\t'; txt += std::to_string(nLeaves); txt += '\t';
			txt += std::to_string(hitN[i]); txt += '\t'; txt += std::to_string(hitL[i]); txt += '\t';
			txt += fmt_g(static_cast<double>(hitN[i]) / nNodes); txt += '\t'; txt += fmt_g(static_cast<double>(hitL[i]) / nLeaves); txt += '\n';
		}
		out << txt;
		nDone += n;
		if(verbose) std::cerr << nDone << " primers processed" << std::endl;
	}
	out.flush();
	hu_batch_destroy(b);
	hu_db_destroy(db);
	if(nFailed) { std::cerr << "Error: " << nFailed << " primer(s) had no alignment" << std::endl; return EXIT_FAILURE; }
	return out.good() ? EXIT_SUCCESS : EXIT_FAILURE;
}
