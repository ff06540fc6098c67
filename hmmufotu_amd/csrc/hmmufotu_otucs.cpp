// hmmufotu-amd-otu-cs: the consensus sequence of every observed OTU — the -c output of hmmufotu-sum (src/hmmufotu-sum.cpp:337-458).
// The records of the assignment files are accepted as hmmufotu-amd-sum accepts them (hu_tsv_reader.h), the OTUs kept are the rows of
// its table in the same order, and each gets one FASTA record: the per-column consensus of its reads' alignments with the node's
// message as a Dirichlet prior (PTUnrooted::inferPostCS).  The column counts (hu_otucs_add) and the inference (hu_otucs_infer) run
// on the device, where the node messages are; options and inputs are checked before the device is touched.
//   hmmufotu-amd-otu-cs <HmmUFOtu-DB> <INFILE [INFILE2 ...]> -c FILE [--no-gap] [-e|--effN DBL] [-l FILE] [--use-dbname] [-q DBL]
//                       [--aln-iden DBL] [--hmm-iden DBL] [-n INT] [-s INT] [--batch N] [--gpu N] [-v]
// Only <DB>.hmm and <DB>.ptu are read.  A database whose stored root is not node 0 is refused (hu_otucs_create).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <fstream>
#include <iostream>
#include <map>
#include "hu_tsv_reader.h"
#include "hu_otu_write.h"
#include "../../include/hmmufotu_amd.h"

static void usage(const char* p) {
	std::cerr << "Infer the consensus sequences of the OTUs of taxonomy assignment files\n"
		"Usage:    " << p << "  <HmmUFOtu-DB> <(INFILE [INFILE2 ...]> <-c FILE> [options]\n"
		"INFILE          FILE           : assignment file(s) from hmmufotu / hmmufotu-amd, plain or .gz\n"
		"Options:    -c  FILE           : OTU Consensus Sequence (CS) alignment output in fasta format, required\n"
		"            --no-gap  FLAG     : remove gaps in the OTU CS alignment\n"
		"            -e|--effN  DBL     : effective number of sequences (pseudo-count) for inferring CS of OTUs with Dirichlet Density models, set to 0 to disable [2]\n"
		"            -l  FILE           : sample name list, with 1st field sample-name and 2nd field assignment filename\n"
		"            --use-dbname  FLAG : use DBNAME as prefix for OTUs\n"
		"            -q  DBL            : minimum qTaxon score required [0]\n"
		"            --aln-iden  DBL    : minimum alignment identity required [0]\n"
		"            --hmm-iden  DBL    : minimum profile-HMM identity required [0]\n"
		"            -n  INT            : minimum number of observed reads required to define an OTU across all samples [0]\n"
		"            -s  INT            : minimum number of observed samples required to define an OTU [0]\n"
		"            --batch  INT       : accepted reads per device batch [8192]\n"
		"            --gpu  INT         : device index [0]\n"
		"            -v  FLAG           : verbose\n"
		"            -h|--help          : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string csFn, listFn;
	hu_tsv::Accept flt;
	double effN = 2; int minRead = 0, minSample = 0, verbose = 0, batch = 8192, gpu = 0; bool useDb = false, noGap = false;
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-c") csFn = val(); else if(a == "-l") listFn = val();
		else if(a == "-e" || a == "--effN") effN = atof(val());
		else if(a == "--use-dbname") useDb = true; else if(a == "--no-gap") noGap = true;
		else if(a == "-q") flt.minQ = atof(val()); else if(a == "--aln-iden") flt.minAln = atof(val()); else if(a == "--hmm-iden") flt.minHmm = atof(val());
		else if(a == "-n") minRead = atoi(val()); else if(a == "-s") minSample = atoi(val());
		else if(a == "--batch") batch = atoi(val()); else if(a == "--gpu") gpu = atoi(val());
		else if(a.size() > 1 && a.find_first_not_of('v', 1) == std::string::npos && a[0] == '-') verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() < 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(csFn.empty()) { std::cerr << "-c must be specified" << std::endl; return EXIT_FAILURE; }
	/* validation as src/hmmufotu-sum.cpp:195-207 */
	if(!(effN >= 0) || std::isinf(effN)) { std::cerr << "-e|--effN must be non-negative" << std::endl; return EXIT_FAILURE; }
	if(!(minRead >= 0)) { std::cerr << "-n must be non-negative integer" << std::endl; return EXIT_FAILURE; }
	if(!(minSample >= 0)) { std::cerr << "-s must be non-negative integer" << std::endl; return EXIT_FAILURE; }
	if(batch < 1 || batch > (1 << 20)) { std::cerr << "--batch must be in [1, 1048576]" << std::endl; return EXIT_FAILURE; }
	const std::string dbName = pos[0];
	std::vector<std::string> inFiles(pos.begin() + 1, pos.end());
	std::map<std::string, std::string> fn2name;
	for(const std::string& f : inFiles) fn2name[f] = f;                  /* the file name is the sample name by default */
	if(!listFn.empty() && !hu_tsv::read_sample_list(listFn, inFiles, fn2name)) { std::cerr << "Unable to open sample list '" << listFn << "'" << std::endl; return EXIT_FAILURE; }
	for(const std::string& f : inFiles) { /* every input is readable and an assignment file, before the device is asked for */
		hu_tsv::Scanner sc; std::string why;
		if(!sc.open(f, why)) { std::cerr << why << std::endl; return EXIT_FAILURE; }
	}
	std::ofstream csOut(csFn);
	if(!csOut) { std::cerr << "Unable to write to '" << csFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }

	if(hu_device_count() <= gpu) { std::cerr << "Error: device " << gpu << " asked for, " << hu_device_count() << " gfx950 device(s) visible" << std::endl; return EXIT_FAILURE; }
	hu_db* db = nullptr;
	if(hu_db_load((dbName + ".hmm").c_str(), (dbName + ".ptu").c_str(), gpu, &db) != HU_OK) { std::cerr << "Unable to load database '" << dbName << "': " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	hu_otucs* cs = nullptr;
	auto fail = [&](const std::string& msg) { std::cerr << msg << std::endl; hu_otucs_free(cs); hu_db_destroy(db); return EXIT_FAILURE; };
	int32_t K = 0, L = 0, N = 0;
	hu_db_info(db, &K, &L, &N, nullptr, nullptr);
	if(verbose) std::cerr << "Database loaded: " << N << " nodes, CS length " << L << std::endl;
	std::vector<int32_t> cs2p;
	if(flt.minHmm != 0) {
		std::vector<int32_t> p2cs((size_t) K + 1);
		if(hu_db_get_profile(db, nullptr, nullptr, nullptr, p2cs.data(), nullptr, nullptr) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
		cs2p = hu_tsv::cs_to_profile(K, L, p2cs);
	}
	if(hu_otucs_create(db, &cs) != HU_OK) return fail(std::string("Error: ") + hu_last_error());

	const size_t S = inFiles.size();
	const std::string prefix = useDb ? dbName + "_" : "";
	std::map<int32_t, std::vector<long>> count;                        /* node -> reads per sample */
	std::vector<int32_t> nodeOf; std::vector<char> rows;
	nodeOf.reserve((size_t) batch); rows.reserve((size_t) batch * L);
	long nAccepted = 0;
	auto flush = [&]() {
		if(nodeOf.empty()) return true;
		const bool ok = hu_otucs_add(cs, (int64_t) nodeOf.size(), nodeOf.data(), rows.data()) == HU_OK;
		nAccepted += (long) nodeOf.size();
		nodeOf.clear(); rows.clear();
		return ok;
	};
	for(size_t s = 0; s < S; ++s) {
		if(verbose) std::cerr << "Processing sample " << fn2name[inFiles[s]] << " ..." << std::endl;
		hu_tsv::Scanner sc; std::string why;
		if(!sc.open(inFiles[s], why)) return fail(why);
		while(sc.next()) {
			long taxon = -1;
			if(!hu_tsv::accepted(sc, flt, cs2p, taxon)) continue;
			if(taxon >= N) return fail("taxon_id " + std::to_string(taxon) + " of read '" + sc.get("id") + "' is not a node of " + dbName);
			const std::string& aln = sc.get("alignment");
			if(aln.size() != (size_t) L) return fail("the alignment of read '" + sc.get("id") + "' has " + std::to_string(aln.size()) + " columns, the database " + std::to_string(L));
			std::vector<long>& c = count[(int32_t) taxon];
			if(c.empty()) c.assign(S, 0);
			c[s]++;
			nodeOf.push_back((int32_t) taxon); rows.insert(rows.end(), aln.begin(), aln.end());
			if((int) nodeOf.size() == batch && !flush()) return fail(std::string("Error: ") + hu_last_error());
		}
	}
	if(!flush()) return fail(std::string("Error: ") + hu_last_error());
	/* the OTUs of the table, in node order (src/hmmufotu-sum.cpp:405-419), and their records (:437-457) */
	std::vector<long> nRead, nSample;
	const std::vector<int32_t> kept = hu_otu_kept(count, minRead, minSample, &nRead, &nSample);
	if(verbose) std::cerr << "Writing OTU Consensus Sequences" << std::endl;
	if(!hu_otucs_write_fasta(csOut, cs, db, dbName, prefix, kept, nRead, nSample, effN, noGap)) return fail(std::string("Error: ") + hu_last_error());
	if(verbose) std::cerr << kept.size() << " OTUs over " << S << " sample(s), " << nAccepted << " reads" << std::endl;
	hu_otucs_free(cs);
	hu_db_destroy(db);
	return csOut.good() ? EXIT_SUCCESS : EXIT_FAILURE;
}
