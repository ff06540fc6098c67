// hmmufotu-amd-pcoa: the samples of a distance matrix as points on the leading principal coordinates (PCoA, classical scaling, Gower
// 1966).  The reference ends at the OTU table; here the matrix of hmmufotu-amd-unifrac -o goes straight into the plot's axes.
//   hmmufotu-amd-pcoa <DIST> [-o FILE] [-k|--axes 3] [--eig-out FILE] [--tol 1e-10] [--max-it 1000] [--oversample 8] [-S|--seed 1] [--mem GB]
//                     [--device N] [--host] [-v]
// The axes are hu_pcoa's: a block iteration on the device (hu_kern_pcoa.h), or with --host by the library's host path.  Every refusal
// comes before a device is asked for or from the iteration itself, and the outputs are opened only after the computation: a refused run
// leaves no file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

static void usage(const char* p) {
	std::cerr << "Place the samples of a distance matrix on its leading principal coordinates (PCoA, classical multidimensional scaling)\n"
		"Usage:    " << p << "  <DIST> [options]\n"
		"DIST      FILE                 : distance matrix from hmmufotu-amd-unifrac -o\n"
		"Options:    -o  FILE           : coordinates output, a line per sample [stdout]\n"
		"            -k|--axes  INT     : number of axes [3]\n"
		"            --eig-out  FILE    : also write per axis its eigenvalue, its share of the trace and its residual\n"
		"            --tol  DBL         : stop when every kept axis has a residual of tol * eigenvalue 1 at the most [1e-10]\n"
		"            --max-it  INT      : iterations at the most [1000]\n"
		"            --oversample  INT  : columns of the block beyond the axes [8]\n"
		"            -S|--seed  INT     : seed of the start block [1]\n"
		"            --mem  DBL         : device memory to use, in GB [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

static std::string num17(double v) { char buf[64]; snprintf(buf, sizeof(buf), "%.17g", v); return buf; }

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, eigFn; bool host = false, haveMem = false; int device = 0, verbose = 0; double memGB = 0;
	hu_pcoa_opts o;
	hu_pcoa_default_opts(&o);
	long long axes = o.k, maxIt = o.max_it, over = o.oversample;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--eig-out") eigFn = val();
		else if(a == "-k" || a == "--axes") axes = atoll(val());
		else if(a == "--tol") o.tol = atof(val());
		else if(a == "--max-it") maxIt = atoll(val());
		else if(a == "--oversample") over = atoll(val());
		else if(a == "-S" || a == "--seed") o.seed = strtoull(val(), nullptr, 10);
		else if(a == "--mem") { memGB = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(axes < 1) { std::cerr << "--axes must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(!(o.tol > 0 && o.tol <= 1e-3)) { std::cerr << "--tol must lie above 0 and be 1e-3 at the most" << std::endl; return EXIT_FAILURE; }
	if(maxIt < 1) { std::cerr << "--max-it must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(over < 0) { std::cerr << "--oversample must be non-negative" << std::endl; return EXIT_FAILURE; }
	if(haveMem && !(memGB > 0 && memGB < 1e6)) { std::cerr << "--mem must be a positive number of GB" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	o.k = axes; o.max_it = maxIt; o.oversample = over; o.host = host ? 1 : 0; o.mem_budget = haveMem ? (int64_t)(memGB * 1073741824.0) : 0;
	if(haveMem && o.mem_budget < 1) o.mem_budget = 1;
	if(verbose) std::cerr << "Loading distance matrix" << std::endl;
	hu_dist_matrix* m = nullptr;
	if(hu_dist_matrix_read(pos[0].c_str(), &m) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	struct Free { hu_dist_matrix* m; ~Free() { hu_dist_matrix_free(m); } } freeMatrix{m};      /* on every exit from here on */
	int64_t n = 0;
	hu_dist_matrix_dims(m, &n);
	const int64_t k = axes;
	hu_pcoa_result res;
	std::vector<double> coords, eig, rs;
	if(n >= 3 && k <= n - 1) { coords.resize((size_t)(n * k)); eig.resize((size_t) k); rs.resize((size_t) k); }
	else { coords.resize(1); eig.resize(1); rs.resize(1); }                /* the library refuses such a call before it writes */
	if(hu_pcoa(host ? -1 : device, n, hu_dist_matrix_values(m), &o, &res, coords.data(), eig.data(), rs.data()) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	if(verbose) {
		double s[6];
		hu_pcoa_timing(s);
		std::cerr << res.iterations << " iteration(s), a block of " << res.m_final << " columns with " << res.positive_in_block << " positive axes" << std::endl;
		for(int64_t a = 0; a < k; ++a) std::cerr << "axis " << a + 1 << ": eigenvalue " << eig[(size_t) a] << ", residual " << rs[(size_t) a] << std::endl;
		if(!host) std::cerr << "copies up " << s[0] << " s, squares " << s[1] << " s, product kernel " << s[2] << " s, small kernels " << s[3] << " s, host m x m work " << s[4]
			<< " s, copy back " << s[5] << " s" << std::endl;
	}
	auto writeCoords = [&](std::ostream& out) {
		out << "sample";
		for(int64_t a = 0; a < k; ++a) out << "\tPC" << a + 1;
		out << '\n';
		for(int64_t i = 0; i < n; ++i) {
			out << hu_dist_matrix_sample(m, i);
			for(int64_t a = 0; a < k; ++a) out << '\t' << num17(coords[(size_t)(i * k + a)]);
			out << '\n';
		}
	};
	/* both outputs are opened before either is written: a file that cannot be opened leaves none behind */
	std::ofstream fc, fe;
	if(!outFn.empty()) {
		fc.open(outFn);
		if(!fc) { std::cerr << "Unable to write to '" << outFn << "'" << std::endl; return EXIT_FAILURE; }
	}
	if(!eigFn.empty()) {
		fe.open(eigFn);
		if(!fe) {
			std::cerr << "Unable to write to '" << eigFn << "'" << std::endl;
			if(!outFn.empty()) { fc.close(); remove(outFn.c_str()); }
			return EXIT_FAILURE;
		}
	}
	if(outFn.empty()) writeCoords(std::cout); else writeCoords(fc);
	if(!eigFn.empty()) {
		fe << "axis\teigenvalue\tproportion\tresidual\n";
		for(int64_t a = 0; a < k; ++a) fe << a + 1 << '\t' << num17(eig[(size_t) a]) << '\t' << num17(eig[(size_t) a] / res.trace) << '\t' << num17(rs[(size_t) a]) << '\n';
		fe << "# trace: " << num17(res.trace) << "\n# iterations: " << res.iterations << "\n# block: " << res.m_final << '\n';
	}
	return EXIT_SUCCESS;
}
