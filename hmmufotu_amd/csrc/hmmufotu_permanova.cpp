// hmmufotu-amd-permanova: do the groups of samples differ on a distance matrix?  (PERMANOVA, Anderson 2001)  The
// reference ends at the OTU table; here the matrix of hmmufotu-amd-unifrac -o goes straight into the test.
//   hmmufotu-amd-permanova <DIST> <GROUPS> [-o FILE] [-n|--perms 999] [-S|--seed 1] [--pairwise] [--perm-out FILE] [--chunk N] [--mem GB]
//                          [--device N] [--host] [-v]
// The sums are hu_permanova's: on the device (hu_kern_permanova.h), or with --host by the library's host path.  Every refusal comes
// before a device is asked for, and the outputs are opened only after the computation: a refused run leaves no file.
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
#include "hu_groups_file.h"

static void usage(const char* p) {
	std::cerr << "Test whether groups of samples differ on a distance matrix (PERMANOVA: pseudo-F and a permutation p-value)\n"
		"Usage:    " << p << "  <DIST> <GROUPS> [options]\n"
		"DIST      FILE                 : distance matrix from hmmufotu-amd-unifrac -o\n"
		"GROUPS    FILE                 : lines of sample<TAB>group; lines that start with '#' and empty lines are skipped\n"
		"Options:    -o  FILE           : result table output [stdout]\n"
		"            -n|--perms  INT    : number of permutations [999]\n"
		"            -S|--seed  INT     : seed of the permutations [1]\n"
		"            --pairwise  FLAG   : also test every pair of groups on its own samples\n"
		"            --perm-out  FILE   : also write SS_within and F of every permutation of the test on all groups\n"
		"            --chunk  INT       : permutations per launch [a function of the matrix's size and the memory]\n"
		"            --mem  DBL         : device memory to use, in GB [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

static std::string num17(double v) { char buf[64]; snprintf(buf, sizeof(buf), "%.17g", v); return buf; }

static std::string line_of(const std::string& name, const hu_permanova_result& r) {
	return name + '\t' + std::to_string(r.n) + '\t' + std::to_string(r.a) + '\t' + std::to_string(r.perms) + '\t' + num17(r.ss_total) + '\t' + num17(r.ss_within) + '\t' +
		num17(r.ss_among) + '\t' + num17(r.F) + '\t' + num17(r.R2) + '\t' + num17(r.p);
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, permFn; bool host = false, pairwise = false; int device = 0, verbose = 0;
	hu_permanova_opts o;
	hu_permanova_default_opts(&o);
	long long perms = o.perms, chunk = 0; bool haveChunk = false, haveMem = false; double memGB = 0;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--perm-out") permFn = val();
		else if(a == "-n" || a == "--perms") perms = atoll(val());
		else if(a == "-S" || a == "--seed") o.seed = strtoull(val(), nullptr, 10);
		else if(a == "--pairwise") pairwise = true;
		else if(a == "--chunk") { chunk = atoll(val()); haveChunk = true; }
		else if(a == "--mem") { memGB = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(perms < 1 || perms > 10000000) { std::cerr << "--perms must lie between 1 and 10000000" << std::endl; return EXIT_FAILURE; }
	if(haveChunk && chunk < 1) { std::cerr << "--chunk must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(haveMem && !(memGB > 0 && memGB < 1e6)) { std::cerr << "--mem must be a positive number of GB" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	o.perms = perms; o.chunk = chunk; o.host = host ? 1 : 0; o.mem_budget = haveMem ? (int64_t)(memGB * 1073741824.0) : 0;
	if(haveMem && o.mem_budget < 1) o.mem_budget = 1;
	if(verbose) std::cerr << "Loading distance matrix" << std::endl;
	hu_dist_matrix* m = nullptr;
	if(hu_dist_matrix_read(pos[0].c_str(), &m) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	int64_t n = 0;
	hu_dist_matrix_dims(m, &n);
	const double* dist = hu_dist_matrix_values(m);
	std::map<std::string, int64_t> at;
	for(int64_t i = 0; i < n; ++i) at[hu_dist_matrix_sample(m, i)] = i;
	std::vector<std::string> groupOf, gname; std::vector<char> seen; std::vector<int64_t> every((size_t) n);
	if(!hu_groups_read(pos[1], n, at, "matrix", verbose != 0, groupOf, seen)) return EXIT_FAILURE;
	for(int64_t i = 0; i < n; ++i) {
		if(!seen[(size_t) i]) { std::cerr << "Sample '" << hu_dist_matrix_sample(m, i) << "' of the matrix has no line in '" << pos[1] << "'" << std::endl; return EXIT_FAILURE; }
		every[(size_t) i] = i;
	}
	const std::vector<int32_t> label = hu_groups_label(groupOf, every, gname);
	const int dev = host ? -1 : device;
	std::vector<std::string> lines;
	hu_permanova_result all;
	std::vector<double> ssw(permFn.empty() ? 0 : (size_t) perms);
	if(hu_permanova(dev, n, dist, label.data(), &o, &all, permFn.empty() ? nullptr : ssw.data()) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	lines.push_back(line_of("all", all));
	if(verbose && !host) {
		double s[4];
		hu_permanova_timing(s);
		std::cerr << "copies up " << s[0] << " s, shuffles " << s[1] << " s, pair kernel " << s[2] << " s, finish and copy back " << s[3] << " s" << std::endl;
	}
	if(pairwise) {
		long long na = 0;
		const size_t A = gname.size();
		for(size_t x = 0; x < A; ++x) for(size_t y = x + 1; y < A; ++y) {
			std::vector<int64_t> idx; std::vector<int32_t> lab; int64_t nx = 0, ny = 0;
			for(int64_t i = 0; i < n; ++i) if(label[(size_t) i] == (int32_t) x || label[(size_t) i] == (int32_t) y) {
				idx.push_back(i); lab.push_back(label[(size_t) i] == (int32_t) x ? 0 : 1); (label[(size_t) i] == (int32_t) x ? nx : ny)++; }
			const std::string name = gname[x] + ":" + gname[y];
			const int64_t k = (int64_t) idx.size();
			if(k < 3 || (nx < 2 && ny < 2)) {
				++na;
				lines.push_back(name + '\t' + std::to_string(k) + "\t2\t" + std::to_string(perms) + "\tNA\tNA\tNA\tNA\tNA\tNA");
				continue;
			}
			if(lab[0] == 1) for(auto& v : lab) v = 1 - v;                    /* labels in order of first appearance: the same partition */
			std::vector<double> sub((size_t)(k * k));
			for(int64_t r = 0; r < k; ++r) for(int64_t c = 0; c < k; ++c) sub[(size_t)(r * k + c)] = dist[idx[(size_t) r] * n + idx[(size_t) c]];
			hu_permanova_result res;
			if(hu_permanova(dev, k, sub.data(), lab.data(), &o, &res, nullptr) != HU_OK) { std::cerr << name << ": " << hu_last_error() << std::endl; return EXIT_FAILURE; }
			lines.push_back(line_of(name, res));
		}
		if(verbose) std::cerr << na << " pair(s) of groups too small to test" << std::endl;
	}
	auto writeAll = [&](std::ostream& out) {
		out << "test\tn\tgroups\tperms\tSS_total\tSS_within\tSS_among\tF\tR2\tp\n";
		for(const auto& l : lines) out << l << '\n';
	};
	if(outFn.empty()) writeAll(std::cout);
	else {
		std::ofstream f(outFn);
		if(!f) { std::cerr << "Unable to write to '" << outFn << "'" << std::endl; return EXIT_FAILURE; }
		writeAll(f);
	}
	if(!permFn.empty()) {
		std::ofstream f(permFn);
		if(!f) { std::cerr << "Unable to write to '" << permFn << "'" << std::endl; return EXIT_FAILURE; }
		f << "perm\tSS_within\tF\n";
		for(long long p = 0; p < perms; ++p) {
			const double w = ssw[(size_t) p], F = ((all.ss_total - w) / (double)(all.a - 1)) / (w / (double)(all.n - all.a));
			f << p << '\t' << num17(w) << '\t' << num17(F) << '\n';
		}
	}
	hu_dist_matrix_free(m);
	return EXIT_SUCCESS;
}
