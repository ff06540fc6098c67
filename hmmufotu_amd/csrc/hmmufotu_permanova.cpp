// hmmufotu-amd-permanova: do the groups of samples differ on a distance matrix?  (PERMANOVA, Anderson 2001)  The
// reference ends at the OTU table; here the matrix of hmmufotu-amd-unifrac -o goes straight into the test.
//   hmmufotu-amd-permanova <DIST> <GROUPS> [-o FILE] [-n|--perms 999] [-S|--seed 1] [--pairwise] [--perm-out FILE] [--chunk N] [--mem GB]
//                          [--device N] [--host] [-v]
//   hmmufotu-amd-permanova <DIST> --design META --terms a,b,a:b [--factor NAME]... [--strata NAME] [-o FILE] [-n -S --perm-out --chunk --mem
//                          --device --host -v]
// With --design the test is hu_permanova_design's: sequential sums of squares of the terms, in the order given, of a design
// of covariates, factors and interactions of two, permuted within the blocks of --strata.  Without it nothing changes.
// The sums are hu_permanova's: on the device (hu_kern_permanova.h), or with --host by the library's host path.  Every refusal comes
// before a device is asked for, and the outputs are opened only after the computation: a refused run leaves no file.
#include <algorithm>
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
#include "hu_design_file.h"

static void usage(const char* p) {
	std::cerr << "Test whether groups of samples differ on a distance matrix (PERMANOVA: pseudo-F and a permutation p-value)\n"
		"Usage:    " << p << "  <DIST> <GROUPS> [options]\n"
		"DIST      FILE                 : distance matrix from hmmufotu-amd-unifrac -o\n"
		"GROUPS    FILE                 : lines of sample<TAB>group; lines that start with '#' and empty lines are skipped\n"
		"Options:    -o  FILE           : result table output [stdout]\n"
		"            -n|--perms  INT    : number of permutations [999]\n"
		"            -S|--seed  INT     : seed of the permutations [1]\n"
		"            --pairwise  FLAG   : also test every pair of groups on its own samples\n"
		"            --design  FILE     : instead of GROUPS: tab-separated metadata, a header line, then one line per sample\n"
		"            --terms  LIST      : with --design: the terms to test in order, e.g. treatment,ph,treatment:ph\n"
		"            --factor  NAME     : with --design: read this numeric-looking column as categorical; may be given more than once\n"
		"            --strata  NAME     : with --design: permute only within the blocks of this column\n"
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

struct DesignArgs { std::string meta, terms, strata; std::vector<std::string> factor; bool haveTerms = false, haveStrata = false; };

/* the run with --design: every refusal before a device is asked for, the outputs opened after the computation */
static int run_design(const std::string& distFn, const DesignArgs& da, const hu_permanova_opts& o, int dev, const std::string& outFn, const std::string& permFn, int verbose) {
	auto fail = [](const std::string& why) { std::cerr << why << std::endl; return EXIT_FAILURE; };
	std::vector<std::string> termName;
	hu_meta_split(da.terms, ',', termName);
	std::vector<std::vector<std::string>> termVar(termName.size());
	std::vector<std::string> used;
	for(size_t t = 0; t < termName.size(); ++t) {
		hu_meta_split(termName[t], ':', termVar[t]);
		if(termVar[t].size() > 2) return fail("Term '" + termName[t] + "': an interaction of more than two variables is not supported");
		for(const auto& v : termVar[t]) {
			if(v.empty()) return fail("--terms '" + da.terms + "': an empty name");
			if(std::find(used.begin(), used.end(), v) == used.end()) used.push_back(v);
		}
	}
	if(verbose) std::cerr << "Loading distance matrix" << std::endl;
	hu_dist_matrix* m = nullptr;
	if(hu_dist_matrix_read(distFn.c_str(), &m) != HU_OK) return fail(hu_last_error());
	int64_t n = 0;
	hu_dist_matrix_dims(m, &n);
	const double* dist = hu_dist_matrix_values(m);
	std::vector<std::string> sample((size_t) n);
	for(int64_t i = 0; i < n; ++i) sample[(size_t) i] = hu_dist_matrix_sample(m, i);
	HuMeta meta; std::string err;
	if(!hu_meta_read(da.meta, sample, meta, err)) return fail(err);
	if(verbose) std::cerr << meta.ignored << " line(s) of '" << da.meta << "' name no sample of the matrix" << std::endl;
	auto isColumn = [&](const std::string& c) { return std::find(meta.column.begin(), meta.column.end(), c) != meta.column.end(); };
	for(const auto& v : used) if(!isColumn(v)) return fail("--terms: '" + v + "' is no column of '" + da.meta + "'");
	for(const auto& v : da.factor) if(!isColumn(v)) return fail("--factor: '" + v + "' is no column of '" + da.meta + "'");
	if(da.haveStrata && !isColumn(da.strata)) return fail("--strata: '" + da.strata + "' is no column of '" + da.meta + "'");
	std::vector<HuMetaVar> mv(used.size());
	std::vector<hu_design_var> var(used.size());
	for(size_t v = 0; v < used.size(); ++v) {
		const bool factor = std::find(da.factor.begin(), da.factor.end(), used[v]) != da.factor.end();
		if(!hu_meta_variable(meta, sample, used[v], factor, mv[v], err)) return fail(err);
		var[v].kind = mv[v].numeric ? 0 : 1; var[v].reserved = 0; var[v].value = mv[v].numeric ? mv[v].value.data() : nullptr; var[v].label = mv[v].numeric ? nullptr : mv[v].label.data();
	}
	HuMetaVar strata;
	if(da.haveStrata && !hu_meta_variable(meta, sample, da.strata, true, strata, err)) return fail(err);
	const int64_t T = (int64_t) termName.size();
	std::vector<hu_design_term> term((size_t) T);
	std::vector<const char*> tn((size_t) T);
	for(int64_t t = 0; t < T; ++t) {
		auto at = [&](const std::string& v) { return (int32_t)(std::find(used.begin(), used.end(), v) - used.begin()); };
		term[(size_t) t].a = at(termVar[(size_t) t][0]); term[(size_t) t].b = termVar[(size_t) t].size() == 2 ? at(termVar[(size_t) t][1]) : -1;
		tn[(size_t) t] = termName[(size_t) t].c_str();
	}
	const int64_t raw = hu_design_raw_columns(n, (int64_t) var.size(), var.data(), T, term.data());
	if(raw < 0) return fail(hu_last_error());
	std::vector<double> Q((size_t)(n * raw));
	std::vector<int64_t> termStart((size_t) T + 1), df((size_t) T), dropped((size_t) T);
	int64_t q = 0;
	if(hu_design_build(n, (int64_t) var.size(), var.data(), T, term.data(), tn.data(), Q.data(), &q, termStart.data(), df.data(), dropped.data()) != HU_OK) return fail(hu_last_error());
	if(verbose) for(int64_t t = 0; t < T; ++t) std::cerr << "term '" << termName[(size_t) t] << "': " << df[(size_t) t] << " column(s) kept, " << dropped[(size_t) t] << " dropped" << std::endl;
	hu_permanova_design_opts d;
	hu_permanova_design_default_opts(&d);
	d.perms = o.perms; d.seed = o.seed; d.host = o.host; d.chunk = o.chunk; d.mem_budget = o.mem_budget;
	std::vector<hu_permanova_design_term> res((size_t) T);
	std::vector<double> ss(permFn.empty() ? 0 : (size_t)(o.perms * T));
	if(hu_permanova_design(dev, n, dist, Q.data(), q, T, termStart.data(), da.haveStrata ? strata.label.data() : nullptr, &d, res.data(), permFn.empty() ? nullptr : ss.data()) != HU_OK)
		return fail(hu_last_error());
	if(verbose) {
		for(int64_t t = 0; t < T; ++t) std::cerr << "term '" << termName[(size_t) t] << "': " << res[(size_t) t].count_nan << " permutation(s) with F = NaN" << std::endl;
		if(dev >= 0) {
			double s[4];
			hu_permanova_design_timing(s);
			std::cerr << "copies up " << s[0] << " s, shuffles " << s[1] << " s, quadratic forms " << s[2] << " s, finish and copy back " << s[3] << " s" << std::endl;
		}
	}
	const hu_permanova_design_term& r0 = res[0];
	auto writeAll = [&](std::ostream& out) {
		out << "term\tdf\tSS\tR2\tF\tp\n";
		for(int64_t t = 0; t < T; ++t) { const auto& r = res[(size_t) t]; out << termName[(size_t) t] << '\t' << r.df << '\t' << num17(r.ss) << '\t' << num17(r.R2) << '\t' << num17(r.F) << '\t' << num17(r.p) << '\n'; }
		out << "Residual\t" << r0.df_res << '\t' << num17(r0.ss_res) << '\t' << num17(r0.ss_res / r0.ss_total) << "\tNA\tNA\n";
		out << "Total\t" << n - 1 << '\t' << num17(r0.ss_total) << '\t' << num17(1.0) << "\tNA\tNA\n";
		out << "# perms: " << o.perms << "\n# seed: " << o.seed << '\n';
		if(da.haveStrata) out << "# strata: " << da.strata << " (" << strata.level.size() << " blocks)\n";
	};
	if(outFn.empty()) writeAll(std::cout);
	else {
		std::ofstream f(outFn);
		if(!f) return fail("Unable to write to '" + outFn + "'");
		writeAll(f);
	}
	if(!permFn.empty()) {
		std::ofstream f(permFn);
		if(!f) return fail("Unable to write to '" + permFn + "'");
		f << "perm";
		for(int64_t t = 0; t < T; ++t) f << "\tSS_" << termName[(size_t) t] << "\tF_" << termName[(size_t) t];
		f << '\n';
		for(long long p = 0; p < o.perms; ++p) {
			const double* row = ss.data() + p * T;
			double sum = 0.0;
			for(int64_t t = 0; t < T; ++t) sum += row[t];
			const double resid = r0.ss_total - sum;                                /* the library's order: the terms ascending, then one subtraction */
			f << p;
			for(int64_t t = 0; t < T; ++t) f << '\t' << num17(row[t]) << '\t' << num17((row[t] / (double) res[(size_t) t].df) / (resid / (double) r0.df_res));
			f << '\n';
		}
	}
	hu_dist_matrix_free(m);
	return EXIT_SUCCESS;
}

int main(int argc, char** argv) {
	DesignArgs da; bool haveDesign = false;
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
		else if(a == "--design") { da.meta = val(); haveDesign = true; }
		else if(a == "--terms") { da.terms = val(); da.haveTerms = true; }
		else if(a == "--factor") da.factor.push_back(val());
		else if(a == "--strata") { da.strata = val(); da.haveStrata = true; }
		else if(a == "--chunk") { chunk = atoll(val()); haveChunk = true; }
		else if(a == "--mem") { memGB = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(!haveDesign && (da.haveTerms || da.haveStrata || !da.factor.empty())) { std::cerr << "--terms, --factor and --strata need --design" << std::endl; return EXIT_FAILURE; }
	if(haveDesign && pos.size() == 2) { std::cerr << "--design takes the place of the GROUPS file: give one of them" << std::endl; return EXIT_FAILURE; }
	if(haveDesign && pairwise) { std::cerr << "--pairwise tests groups: it does not go with --design" << std::endl; return EXIT_FAILURE; }
	if(haveDesign && (!da.haveTerms || da.terms.empty())) { std::cerr << "--design needs --terms: the terms to test, in order" << std::endl; return EXIT_FAILURE; }
	if(pos.size() != (haveDesign ? 1u : 2u)) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(perms < 1 || perms > 10000000) { std::cerr << "--perms must lie between 1 and 10000000" << std::endl; return EXIT_FAILURE; }
	if(haveChunk && chunk < 1) { std::cerr << "--chunk must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(haveMem && !(memGB > 0 && memGB < 1e6)) { std::cerr << "--mem must be a positive number of GB" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	o.perms = perms; o.chunk = chunk; o.host = host ? 1 : 0; o.mem_budget = haveMem ? (int64_t)(memGB * 1073741824.0) : 0;
	if(haveMem && o.mem_budget < 1) o.mem_budget = 1;
	if(haveDesign) return run_design(pos[0], da, o, host ? -1 : device, outFn, permFn, verbose);
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
