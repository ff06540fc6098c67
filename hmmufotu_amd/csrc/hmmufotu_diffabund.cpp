// hmmufotu-amd-diffabund: which OTUs of a table differ between the groups of samples?  (Kruskal-Wallis per OTU with permutation
// p-values, single-step maxT and Benjamini-Hochberg)  The table is the one the assignment run and the table tools
// write, GROUPS the file of hmmufotu-amd-permanova, and the same seed relabels the samples as that program does.
//   hmmufotu-amd-diffabund <OTU-FILE> <GROUPS> [-o FILE] [-n|--perms 999] [-S|--seed 1] [--rank-by fraction|count] [--min-prevalence 1]
//                          [--ignore-missing] [--perm-out FILE] [--chunk N] [--mem GB] [--device N] [--host] [-v]
// The statistics are hu_diffabund's: on the device (hu_kern_diffabund.h), or with --host by the library's host path.  Every refusal
// comes before a device is asked for, and the outputs are opened only after the computation: a refused run leaves no file.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"
#include "hu_num_format.h"
#include "hu_groups_file.h"

static void usage(const char* p) {
	std::cerr << "Test every OTU of a table for a difference between groups of samples (Kruskal-Wallis on ranks, permutation p-values, maxT and BH)\n"
		"Usage:    " << p << "  <OTU-FILE> <GROUPS> [options]\n"
		"OTU-FILE  FILE                 : OTU table from hmmufotu-amd-sum, -merge, -subset or -norm\n"
		"GROUPS    FILE                 : lines of sample<TAB>group; lines that start with '#' and empty lines are skipped\n"
		"Options:    -o  FILE           : result table output [stdout]\n"
		"            -n|--perms  INT    : number of permutations [999]\n"
		"            -S|--seed  INT     : seed of the permutations [1]\n"
		"            --rank-by  STR     : rank an OTU's cells by their 'fraction' of the sample's reads or by their 'count' [fraction]\n"
		"            --min-prevalence  INT : test only OTUs present in this many samples at the least [1]\n"
		"            --ignore-missing  FLAG : leave samples without a line in GROUPS out of the test instead of refusing\n"
		"            --perm-out  FILE   : also write the largest H among the OTUs of every permutation\n"
		"            --chunk  INT       : permutations per launch [a function of the table's size and the memory]\n"
		"            --mem  DBL         : device memory to use, in GB [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, permFn, rankBy = "fraction"; bool host = false, ignoreMissing = false; int device = 0, verbose = 0;
	hu_diffabund_opts o;
	hu_diffabund_default_opts(&o);
	long long perms = o.perms, chunk = 0, minPrev = o.min_prevalence; bool haveChunk = false, haveMem = false; double memGB = 0;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--perm-out") permFn = val();
		else if(a == "-n" || a == "--perms") perms = atoll(val());
		else if(a == "-S" || a == "--seed") o.seed = strtoull(val(), nullptr, 10);
		else if(a == "--rank-by") rankBy = val();
		else if(a == "--min-prevalence") minPrev = atoll(val());
		else if(a == "--ignore-missing") ignoreMissing = true;
		else if(a == "--chunk") { chunk = atoll(val()); haveChunk = true; }
		else if(a == "--mem") { memGB = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(perms < 1 || perms > 10000000) { std::cerr << "--perms must lie between 1 and 10000000" << std::endl; return EXIT_FAILURE; }
	if(rankBy != "fraction" && rankBy != "count") { std::cerr << "--rank-by must be 'fraction' or 'count'" << std::endl; return EXIT_FAILURE; }
	if(minPrev < 0) { std::cerr << "--min-prevalence must be non-negative" << std::endl; return EXIT_FAILURE; }
	if(haveChunk && chunk < 1) { std::cerr << "--chunk must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(haveMem && !(memGB > 0 && memGB < 1e6)) { std::cerr << "--mem must be a positive number of GB" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	o.perms = perms; o.chunk = chunk; o.host = host ? 1 : 0; o.rank_by = rankBy == "count" ? 1 : 0; o.min_prevalence = minPrev;
	o.mem_budget = haveMem ? (int64_t)(memGB * 1073741824.0) : 0;
	if(haveMem && o.mem_budget < 1) o.mem_budget = 1;
	if(verbose) std::cerr << "Loading OTUTable" << std::endl;
	hu_otu_table* t = nullptr;
	if(hu_otu_table_read(pos[0].c_str(), &t) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	int64_t M = 0, S = 0;
	hu_otu_table_dims(t, &M, &S);
	if(M < 1 || S < 1) { std::cerr << "'" << pos[0] << "' is a table without " << (M < 1 ? "OTUs" : "samples") << std::endl; return EXIT_FAILURE; }
	const double* cnt = hu_otu_table_counts(t);
	std::map<std::string, int64_t> at;
	for(int64_t j = 0; j < S; ++j) at[hu_otu_table_sample(t, j)] = j;
	std::vector<std::string> groupOf, gname; std::vector<char> seen;
	if(!hu_groups_read(pos[1], S, at, "table", verbose != 0, groupOf, seen)) return EXIT_FAILURE;
	/* the samples of the test: all of them, or with --ignore-missing those that have a line */
	std::vector<int64_t> col;
	for(int64_t j = 0; j < S; ++j) {
		if(seen[(size_t) j]) col.push_back(j);
		else if(!ignoreMissing) { std::cerr << "Sample '" << hu_otu_table_sample(t, j) << "' of the table has no line in '" << pos[1] << "'" << std::endl; return EXIT_FAILURE; }
	}
	const int64_t N = (int64_t) col.size();
	if(verbose && ignoreMissing) std::cerr << S - N << " sample(s) of the table have no line in '" << pos[1] << "' and are left out" << std::endl;
	const std::vector<int32_t> label = hu_groups_label(groupOf, col, gname);
	std::vector<double> sub;
	const double* use = cnt;
	if(N != S) {
		sub.resize((size_t)(M * N));
		for(int64_t i = 0; i < M; ++i) for(int64_t k = 0; k < N; ++k) sub[(size_t)(i * N + k)] = cnt[i * S + col[(size_t) k]];
		use = sub.data();
	}
	/* the refusals that name an OTU or a sample */
	for(int64_t k = 0; k < N; ++k) {
		double tot = 0;
		for(int64_t i = 0; i < M; ++i) {
			const double v = use[i * N + k];
			if(!(v >= 0) || !std::isfinite(v)) { std::cerr << "OTU '" << hu_otu_table_otu(t, i) << "' has a negative or non-finite cell in sample '" << hu_otu_table_sample(t, col[(size_t) k]) << "'" << std::endl; return EXIT_FAILURE; }
			tot += v;
		}
		if(o.rank_by == 0 && !(tot > 0)) { std::cerr << "Sample '" << hu_otu_table_sample(t, col[(size_t) k]) << "' has no reads: its fractions do not exist (--rank-by count ranks the counts)" << std::endl; return EXIT_FAILURE; }
	}
	std::vector<hu_diffabund_rec> rec((size_t) M);
	std::vector<double> mx(permFn.empty() ? 0 : (size_t) perms);
	if(hu_diffabund(host ? -1 : device, M, N, use, label.data(), &o, rec.data(), permFn.empty() ? nullptr : mx.data()) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	long long m = 0;
	for(const auto& r : rec) m += r.tested;
	if(verbose) {
		std::cerr << N << " samples in " << gname.size() << " groups, " << m << " OTU(s) tested, " << M - m << " not tested (every cell ties, or fewer than " << minPrev << " samples)" << std::endl;
		if(!host) {
			double s[4];
			hu_diffabund_timing(s);
			std::cerr << "copies up " << s[0] << " s, shuffles " << s[1] << " s, sums " << s[2] << " s, finish and copy back " << s[3] << " s" << std::endl;
		}
	}
	auto writeAll = [&](std::ostream& out) {
		out << "otu\tprevalence\tH\tp\tp_maxT\tq\tbest\ttaxonomy\n";
		for(int64_t i = 0; i < M; ++i) {
			const hu_diffabund_rec& r = rec[(size_t) i];
			out << hu_otu_table_otu(t, i) << '\t' << r.prevalence << '\t';
			if(r.tested) out << hu_num17(r.H) << '\t' << hu_num17(r.p) << '\t' << hu_num17(r.p_maxT) << '\t' << hu_num17(r.q) << '\t' << gname[(size_t) r.best];
			else out << "NA\tNA\tNA\tNA\tNA";
			out << '\t' << hu_otu_table_taxon(t, i) << '\n';
		}
		out << "# tested: " << m << " of " << M << "\n# perms: " << perms << "\n# seed: " << o.seed << '\n';
	};
	/* every file is opened before one is written */
	std::ofstream fo, fp;
	if(!outFn.empty()) { fo.open(outFn); if(!fo) { std::cerr << "Unable to write to '" << outFn << "'" << std::endl; return EXIT_FAILURE; } }
	if(!permFn.empty()) { fp.open(permFn); if(!fp) { std::cerr << "Unable to write to '" << permFn << "'" << std::endl; return EXIT_FAILURE; } }
	if(outFn.empty()) writeAll(std::cout); else writeAll(fo);
	if(!permFn.empty()) {
		fp << "perm\tmax_H\n";
		for(long long p = 0; p < perms; ++p) fp << p << '\t' << hu_num17(mx[(size_t) p]) << '\n';
	}
	hu_otu_table_free(t);
	return EXIT_SUCCESS;
}
