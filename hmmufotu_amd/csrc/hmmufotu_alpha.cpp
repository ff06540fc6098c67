// hmmufotu-amd-alpha: alpha diversity of the samples of an OTU table and rarefaction curves.  The reference hands this
// step to another package, which needs a tree matched to OTU names; here the OTU ids are node numbers of <DB>.ptu.
//   hmmufotu-amd-alpha <OTU-FILE> [--db DB] [-o FILE] [--depths a,b,c | --steps 10 [--max-depth M]] [--reps 10] [-S|--seed 1]
//                      [--curve-out FILE] [--draws-out FILE] [--chunk N] [--mem GB] [--device N] [--host] [-v]
// The statistics are hu_alpha's: on the device (hu_kern_draw.h, hu_kern_alpha.h), or with --host by the library's host path; the metrics and a curve's
// mean and deviation are the library's host code on both.  Every refusal comes before a device is asked for, and the outputs are opened
// only after the computation: a refused run leaves no file.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "hu_num_format.h"
#include "../../include/hmmufotu_amd.h"

static void usage(const char* p) {
	std::cerr << "Alpha diversity of the samples of an OTUTable (richness, Chao1, Shannon, Simpson, Good's coverage, Faith's PD) and rarefaction curves\n"
		"Usage:    " << p << "  <OTU-FILE> [options]\n"
		"OTU-FILE  FILE                 : OTUTable from hmmufotu-amd-sum, -merge, -subset or -norm\n"
		"Options:    --db  STR          : database name (prefix) used to generate these OTUs; adds Faith's PD on its tree\n"
		"            -o  FILE           : metrics of the whole samples [stdout]\n"
		"            --depths  LIST     : rarefaction depths, comma-separated and ascending\n"
		"            --steps  INT       : depths i * M / steps, i = 1 .. steps, instead of --depths [10]\n"
		"            --max-depth  INT   : M of --steps [the largest sample]\n"
		"            --reps  INT        : draws per sample and depth [10]\n"
		"            -S|--seed  INT     : seed of the draws; repeat r draws as hmmufotu-amd-subset -S seed + r does [1]\n"
		"            --curve-out  FILE  : mean and standard deviation of every metric per sample and depth\n"
		"            --draws-out  FILE  : the metrics of every draw\n"
		"            --chunk  INT       : reads per workgroup [16384]\n"
		"            --mem  DBL         : device memory to use, in GB [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

/* a whole number without a sign, nothing after it */
static bool whole(const char* s, uint64_t& out) {
	if(!s || !*s || *s < '0' || *s > '9') return false;
	char* end = nullptr;
	errno = 0;
	out = strtoull(s, &end, 10);
	return errno == 0 && *end == 0;
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string dbName, outFn, curveFn, drawsFn, depthList;
	bool host = false, haveDepths = false, haveSteps = false, haveMax = false, haveMem = false;
	uint64_t steps = 10, maxDepth = 0, reps = 10, seed = 1, chunk = 0, device = 0;
	bool haveChunk = false;
	double memGB = 0;
	int verbose = 0;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		auto num = [&](uint64_t& v) { const char* s = val(); if(!whole(s, v)) { std::cerr << "Error: option " << a << ": '" << s << "' is not a whole number" << std::endl; exit(EXIT_FAILURE); } };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "--db") dbName = val(); else if(a == "-o") outFn = val(); else if(a == "--curve-out") curveFn = val(); else if(a == "--draws-out") drawsFn = val();
		else if(a == "--depths") { depthList = val(); haveDepths = true; }
		else if(a == "--steps") { num(steps); haveSteps = true; }
		else if(a == "--max-depth") { num(maxDepth); haveMax = true; }
		else if(a == "--reps") num(reps);
		else if(a == "-S" || a == "--seed") num(seed);
		else if(a == "--chunk") { num(chunk); haveChunk = true; }
		else if(a == "--mem") {
			const char* s = val(); char* end = nullptr;
			memGB = strtod(s, &end); haveMem = true;
			if(!*s || *end) { std::cerr << "Error: option --mem: '" << s << "' is not a number" << std::endl; return EXIT_FAILURE; }
		}
		else if(a == "--device") num(device); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	if(haveDepths && (haveSteps || haveMax)) { std::cerr << "--depths does not go with --steps or --max-depth: the depths are listed or spaced, not both" << std::endl; return EXIT_FAILURE; }
	if(haveSteps && (steps < 1 || steps > 1000000)) { std::cerr << "--steps must lie between 1 and 1000000" << std::endl; return EXIT_FAILURE; }
	if(haveMax && (maxDepth < 1 || maxDepth >= (1ull << 32))) { std::cerr << "--max-depth must lie between 1 and 2^32 - 1" << std::endl; return EXIT_FAILURE; }
	if(reps > 0x7fffffffull) { std::cerr << "--reps must be below 2^31" << std::endl; return EXIT_FAILURE; }
	if(haveChunk && (chunk < 1 || chunk > (1u << 24))) { std::cerr << "--chunk must lie between 1 and " << (1 << 24) << std::endl; return EXIT_FAILURE; }
	if(haveMem && !(memGB > 0 && memGB < 1e6)) { std::cerr << "--mem must be a positive number of GB" << std::endl; return EXIT_FAILURE; }
	if(device > 1023) { std::cerr << "--device must be a device number; --host runs without one" << std::endl; return EXIT_FAILURE; }
	const bool wantDraws = !curveFn.empty() || !drawsFn.empty();
	if(!wantDraws && (haveDepths || haveSteps || haveMax)) { std::cerr << "--depths, --steps and --max-depth go with --curve-out or --draws-out, which take the draws" << std::endl; return EXIT_FAILURE; }
	std::vector<uint64_t> depths;
	if(haveDepths) {
		for(size_t at = 0;;) {
			const size_t comma = depthList.find(',', at);
			const std::string f = depthList.substr(at, comma == std::string::npos ? comma : comma - at);
			uint64_t m = 0;
			if(!whole(f.c_str(), m)) { std::cerr << "Error: option --depths: '" << f << "' is not a whole number" << std::endl; return EXIT_FAILURE; }
			depths.push_back(m);
			if(comma == std::string::npos) break;
			at = comma + 1;
		}
	}
	if(wantDraws && reps == 0) { std::cerr << "--curve-out and --draws-out need draws: --reps must be at least 1" << std::endl; return EXIT_FAILURE; }
	hu_alpha_opts o;
	hu_alpha_default_opts(&o);
	o.host = host ? 1 : 0;
	if(haveChunk) o.chunk = (int32_t) chunk;
	o.mem_budget = haveMem ? (int64_t)(memGB * 1073741824.0) : 0;
	if(haveMem && o.mem_budget < 1) o.mem_budget = 1;
	if(verbose) std::cerr << "Loading OTUTable" << std::endl;
	hu_otu_table* t = nullptr;
	if(hu_otu_table_read(pos[0].c_str(), &t) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	int64_t M = 0, S = 0;
	hu_otu_table_dims(t, &M, &S);
	if(S < 1) { std::cerr << "'" << pos[0] << "' is a table without samples" << std::endl; return EXIT_FAILURE; }
	const double* cnt = hu_otu_table_counts(t);
	double largest = 0;
	for(int64_t j = 0; j < S; ++j) {
		double tot = 0;
		for(int64_t i = 0; i < M; ++i) {
			const double v = cnt[i * S + j];
			if(!(v >= 0) || !std::isfinite(v) || v != std::floor(v)) { std::cerr << "OTU '" << hu_otu_table_otu(t, i) << "' has a cell that is not a non-negative integer in sample '" << hu_otu_table_sample(t, j) << "'" << std::endl; return EXIT_FAILURE; }
			tot += v;
		}
		if(!(tot > 0)) { std::cerr << "Sample '" << hu_otu_table_sample(t, j) << "' has no reads: hmmufotu-amd-subset drops such samples" << std::endl; return EXIT_FAILURE; }
		if(!(tot < 4294967296.0)) { std::cerr << "Sample '" << hu_otu_table_sample(t, j) << "' holds 2^32 reads or more" << std::endl; return EXIT_FAILURE; }
		largest = std::max(largest, tot);
	}
	if(wantDraws && !haveDepths) {
		const uint64_t top = haveMax ? maxDepth : (uint64_t) largest;
		for(uint64_t i = 1; i <= steps; ++i) { const uint64_t m = i * top / steps; if(m > 0 && (depths.empty() || m != depths.back())) depths.push_back(m); }
	}
	if(wantDraws && depths.empty()) { std::cerr << "--curve-out and --draws-out need draws: no depth is left" << std::endl; return EXIT_FAILURE; }
	std::vector<int32_t> parent, otuNode; std::vector<double> blen;
	hu_unifrac_tree tree; memset(&tree, 0, sizeof(tree));
	const bool withTree = !dbName.empty();
	if(withTree) {
		hu_tree_info* ti = nullptr;
		if(hu_tree_info_load((dbName + ".ptu").c_str(), &ti) != HU_OK) { std::cerr << "Unable to load Phylogenetic tree data '" << dbName << ".ptu': " << hu_last_error() << std::endl; return EXIT_FAILURE; }
		int32_t N = 0;
		hu_tree_info_get(ti, &N, nullptr, nullptr, nullptr);
		if(verbose) std::cerr << "Phylogenetic tree loaded, " << N << " nodes" << std::endl;
		parent.resize((size_t) N); blen.resize((size_t) N);
		for(int32_t v = 0; v < N; ++v) hu_tree_info_node(ti, v, &parent[(size_t) v], &blen[(size_t) v], nullptr, nullptr, nullptr, nullptr);
		hu_tree_info_free(ti);
		for(int64_t i = 0; i < M; ++i) {
			const char* id = hu_otu_table_otu(t, i);
			char* end = nullptr;
			const long long u = strtoll(id, &end, 10);
			if(!*id || *end || id[0] < '0' || id[0] > '9') { std::cerr << "OTU id '" << id << "' is not a node number: a tree needs tables made without --use-dbname" << std::endl; return EXIT_FAILURE; }
			if(u >= N) { std::cerr << "OTU id '" << id << "' is not a node of " << dbName << std::endl; return EXIT_FAILURE; }
			otuNode.push_back((int32_t) u);
		}
		tree.n_nodes = N; tree.parent = parent.data(); tree.blen = blen.data();
	}
	const size_t nD = depths.size(), R = wantDraws ? (size_t) reps : 0;
	std::vector<hu_alpha_rec> wholeRec((size_t) S), drawRec((size_t) S * nD * R);
	const int dev = host ? -1 : (int) device;
	if(hu_alpha(dev, withTree ? &tree : nullptr, M, S, withTree ? otuNode.data() : nullptr, cnt, (int64_t) nD, depths.data(), (int64_t) R, seed, &o, wholeRec.data(),
			drawRec.empty() ? nullptr : drawRec.data()) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	if(verbose) {
		int64_t sz[6] = {0, 0, 0, 0, 0, 0};
		hu_alpha_sizes(withTree ? &tree : nullptr, M, S, withTree ? otuNode.data() : nullptr, cnt, (int64_t) nD, depths.data(), (int64_t) R, &o, sz);
		std::cerr << "seed " << seed << ", " << sz[4] - S << " draws and " << S << " whole samples, " << sz[0] << " nonzero cells, " << sz[5] << " kept branches, " << sz[1] << " branch entries" << std::endl;
		std::cerr << "chunks of " << o.chunk << " reads, " << sz[3] << " at the most per sample; one resident draw takes " << 1136 + 4 * sz[2] + 24 * sz[3] << " bytes, the table "
			<< hu_alpha_need(S, sz[0], sz[1], sz[2], sz[3], 0) << std::endl;
		if(!host) {
			double s[6];
			hu_alpha_timing(s);
			std::cerr << "copies up " << s[0] << " s, select " << s[1] << " s, take " << s[2] << " s, metrics " << s[3] << " s, PD " << s[4] << " s, copy back " << s[5] << " s" << std::endl;
		}
	}
	auto metrics = [&](std::ostream& out, const hu_alpha_rec& r) {
		if(r.reads == 0) { out << "\tNA\tNA\tNA\tNA\tNA\tNA\tNA"; if(withTree) out << "\tNA"; return; }
		out << '\t' << r.S << '\t' << r.F1 << '\t' << r.F2 << '\t' << hu_num17(r.chao1) << '\t' << hu_num17(r.shannon) << '\t' << hu_num17(r.simpson) << '\t' << hu_num17(r.goods_coverage);
		if(withTree) out << '\t' << hu_num17(r.faith_pd);
	};
	static const char* const cols = "\tobserved\tsingles\tdoubles\tchao1\tshannon\tsimpson\tgoods_coverage";
	auto writeWhole = [&](std::ostream& out) {
		out << "sample\treads" << cols << (withTree ? "\tfaith_pd" : "") << '\n';
		for(int64_t j = 0; j < S; ++j) { out << hu_otu_table_sample(t, j) << '\t' << wholeRec[(size_t) j].reads; metrics(out, wholeRec[(size_t) j]); out << '\n'; }
	};
	auto writeDraws = [&](std::ostream& out) {
		out << "sample\tdepth\trep" << cols << (withTree ? "\tfaith_pd" : "") << '\n';
		for(int64_t j = 0; j < S; ++j) for(size_t d = 0; d < nD; ++d) for(size_t r = 0; r < R; ++r) {
			out << hu_otu_table_sample(t, j) << '\t' << depths[d] << '\t' << r; metrics(out, drawRec[((size_t) j * nD + d) * R + r]); out << '\n';
		}
		out << "# seed: " << seed << '\n';
	};
	auto writeCurve = [&](std::ostream& out) {
		static const char* const names[] = {"observed", "chao1", "shannon", "simpson", "goods_coverage", "faith_pd"};
		const int nm = withTree ? 6 : 5;
		out << "sample\tdepth\treps";
		for(int k = 0; k < nm; ++k) out << '\t' << names[k] << "_mean\t" << names[k] << "_sd";
		out << '\n';
		std::vector<double> x(R);
		for(int64_t j = 0; j < S; ++j) for(size_t d = 0; d < nD; ++d) {
			const hu_alpha_rec* r = &drawRec[((size_t) j * nD + d) * R];
			const bool exists = r[0].reads > 0;
			out << hu_otu_table_sample(t, j) << '\t' << depths[d] << '\t' << (exists ? R : 0);
			for(int k = 0; k < nm; ++k) {
				if(!exists) { out << "\tNA\tNA"; continue; }
				for(size_t i = 0; i < R; ++i) x[i] = k == 0 ? r[i].observed : k == 1 ? r[i].chao1 : k == 2 ? r[i].shannon : k == 3 ? r[i].simpson : k == 4 ? r[i].goods_coverage : r[i].faith_pd;
				double mean = 0, sd = 0;
				hu_alpha_curve((int64_t) R, x.data(), &mean, &sd);
				out << '\t' << hu_num17(mean) << '\t' << hu_num17(sd);
			}
			out << '\n';
		}
	};
	/* every file is opened before one is written */
	std::ofstream fo, fc, fd;
	if(!outFn.empty()) { fo.open(outFn); if(!fo) { std::cerr << "Unable to write to '" << outFn << "'" << std::endl; return EXIT_FAILURE; } }
	if(!curveFn.empty()) { fc.open(curveFn); if(!fc) { std::cerr << "Unable to write to '" << curveFn << "'" << std::endl; return EXIT_FAILURE; } }
	if(!drawsFn.empty()) { fd.open(drawsFn); if(!fd) { std::cerr << "Unable to write to '" << drawsFn << "'" << std::endl; return EXIT_FAILURE; } }
	if(outFn.empty()) writeWhole(std::cout); else writeWhole(fo);
	if(!curveFn.empty()) writeCurve(fc);
	if(!drawsFn.empty()) writeDraws(fd);
	hu_otu_table_free(t);
	return EXIT_SUCCESS;
}
