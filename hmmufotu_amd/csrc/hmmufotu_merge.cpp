// hmmufotu-amd-merge: one OTU table out of the tables of several runs (hmmufotu-merge, src/hmmufotu-merge.cpp:51-174): the tables are
// added up in the order given (OTUTable::operator+=, hu_otu_table_merge) and written with the reference's info line.
//   hmmufotu-amd-merge <OTU-FILE1> <OTU-FILE2> [OTU-FILE3 ...] [-o FILE] [-t FILE --db DB] [-v]
// -t: the OTU tree of the merged ids, the writer of hmmufotu-amd-sum -t (hu_otu_tree.h).  The ids must be node numbers of <DB>.ptu: an
// id with a DBNAME_ prefix (hmmufotu-sum --use-dbname) is refused, as boost::lexical_cast<size_t> throws on it in the reference (:169).
// Host only.
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "hu_otu_tree.h"
#include "../../include/hmmufotu_amd.h"

static void usage(const char* p) {
	std::cerr << "Merge two or more OTUTables, and optionally generate the merged OTU tree\n"
		"Usage:    " << p << "  <OTU-FILE1> <OTU-FILE2> [OTU-FILE3 ...] [options]\n"
		"OTU-FILE        FILE           : OTUFile from hmmufotu-amd-sum or other utils\n"
		"Options:    -o  FILE           : write merged OTU to FILE instead of stdout\n"
		"            -t  FILE           : OTU tree output\n"
		"            --db  STR          : database name (prefix) used to generate these OTUs, required only if -t is requested\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> inFiles; std::string otuFn, treeFn, dbName; int verbose = 0;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") otuFn = val(); else if(a == "-t") treeFn = val(); else if(a == "--db") dbName = val();
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else inFiles.push_back(a);
	}
	if(inFiles.size() < 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(!treeFn.empty() && dbName.empty()) { std::cerr << "--db is required when -t is requested" << std::endl; return EXIT_FAILURE; }
	hu_tree_info* ti = nullptr;
	std::ofstream treeOut;
	if(!treeFn.empty()) {
		treeOut.open(treeFn);
		if(!treeOut) { std::cerr << "Unable to write to '" << treeFn << "'" << std::endl; return EXIT_FAILURE; }
		if(hu_tree_info_load((dbName + ".ptu").c_str(), &ti) != HU_OK) { std::cerr << "Unable to load Phylogenetic tree data '" << dbName << ".ptu': " << hu_last_error() << std::endl; return EXIT_FAILURE; }
		if(verbose) std::cerr << "Phylogenetic tree loaded" << std::endl;
	}
	if(verbose) std::cerr << "Merging OTUTables" << std::endl;
	hu_otu_table* merged = nullptr;
	const char* none = nullptr;
	if(hu_otu_table_new(0, 0, &none, &none, &none, nullptr, &merged) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	for(const std::string& f : inFiles) {
		if(verbose) std::cerr << f << std::endl;
		hu_otu_table* t = nullptr;
		if(hu_otu_table_read(f.c_str(), &t) != HU_OK || hu_otu_table_merge(merged, t) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		hu_otu_table_free(t);
	}
	if(verbose) std::cerr << "Writing merged OTUTable" << std::endl;
	const std::string info = std::string(" OTU table merged by ") + argv[0];
	if(hu_otu_table_write(merged, otuFn.empty() ? "-" : otuFn.c_str(), info.c_str()) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	if(ti) {
		if(verbose) std::cerr << "Writing merged OTU tree" << std::endl;
		int32_t N = 0; int64_t M = 0;
		hu_tree_info_get(ti, &N, nullptr, nullptr, nullptr);
		hu_otu_table_dims(merged, &M, nullptr);
		std::vector<int32_t> otus;
		for(int64_t i = 0; i < M; ++i) {
			const char* id = hu_otu_table_otu(merged, i);
			char* end = nullptr;
			const long long u = strtoll(id, &end, 10);
			if(!*id || *end || id[0] < '0' || id[0] > '9') { std::cerr << "OTU id '" << id << "' is not a node number: a tree needs tables made without --use-dbname" << std::endl; return EXIT_FAILURE; }
			if(u >= N) { std::cerr << "OTU id '" << id << "' is not a node of " << dbName << std::endl; return EXIT_FAILURE; }
			otus.push_back((int32_t) u);
		}
		hu_otu_tree_write(treeOut, ti, otus, "");
		hu_tree_info_free(ti);
	}
	hu_otu_table_free(merged);
	return EXIT_SUCCESS;
}
