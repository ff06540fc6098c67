// hmmufotu-amd-unifrac: the distances between the samples of an OTU table on the database's tree.  The reference hands
// this step to another package; here the OTU ids are node numbers of <DB>.ptu, so no tree has to be matched to the table by name.
//   hmmufotu-amd-unifrac <OTU-FILE> [--db DB] [-o DIST] [--method M] [--alpha A] [--pd FILE] [--slab L] [--device N] [--host] [-v]
//                        [--rarefy M [--reps R] [-S|--seed N] [--sd-out FILE] [--draw-chunk N] [--chunk N] [--mem GB]]
// With --rarefy the matrix is the mean of hu_unifrac_rarefied over R rarefied draws of M reads, in the same format.
// The sums are hu_unifrac's: on the device (hu_kern_unifrac.h), or with --host by the library's host path.  Every refusal comes before
// a device is asked for, and the output is opened only after the computation: a refused run leaves no file.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../include/hmmufotu_amd.h"

static void usage(const char* p) {
	std::cerr << "Distances between the samples of an OTUTable on the phylogenetic tree of the database (UniFrac)\n"
		"Usage:    " << p << "  <OTU-FILE> [options]\n"
		"OTU-FILE  FILE                 : OTUTable from hmmufotu-amd-sum, -merge, -subset or -norm\n"
		"Options:    --db  STR          : database name (prefix) used to generate these OTUs, required unless the method is bray-curtis or jaccard\n"
		"            -o  FILE           : distance matrix output [stdout]\n"
		"            --method  STR      : unweighted, weighted, weighted-raw, generalized, bray-curtis or jaccard [weighted]\n"
		"            --alpha  DBL       : exponent of the generalized method, between 0 and 1 [0.5]\n"
		"            --pd  FILE         : also write Faith's PD of every sample\n"
		"            --slab  INT        : branches per slab of the pair kernel [a function of the table's size]\n"
		"            --rarefy  INT      : average the distances over rarefied draws of INT reads; samples with fewer reads are dropped\n"
		"            --reps  INT        : rarefied draws, 1 to 100000 [100]\n"
		"            -S|--seed  INT     : seed of the draws; draw r is hmmufotu-amd-subset -s INT -S seed+r [1]\n"
		"            --sd-out  FILE     : also write the standard deviation of every distance over the draws\n"
		"            --draw-chunk  INT  : draws resident on the device at once [as many as the memory holds]\n"
		"            --chunk  INT       : reads per workgroup of the draw kernels [16384]\n"
		"            --mem  DBL         : device memory to use in GB, with --rarefy [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

static std::string num17(double v) { char buf[64]; snprintf(buf, sizeof(buf), "%.17g", v); return buf; }

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string dbName, outFn, pdFn, method = "weighted"; bool host = false, haveAlpha = false; int device = 0, verbose = 0;
	hu_unifrac_opts o;
	hu_unifrac_default_opts(&o);
	long long slab = 0; bool haveSlab = false;
	std::string sdFn; long long rarefy = 0, reps = 100, drawChunk = 0, chunk = 0; unsigned long long seed = 1; double memGb = 0;
	bool haveRarefy = false, haveReps = false, haveSeed = false, haveDrawChunk = false, haveChunk = false, haveMem = false;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1" << std::endl; return EXIT_SUCCESS; }
		else if(a == "--db") dbName = val(); else if(a == "-o") outFn = val(); else if(a == "--method") method = val(); else if(a == "--pd") pdFn = val();
		else if(a == "--alpha") { o.alpha = atof(val()); haveAlpha = true; }
		else if(a == "--slab") { slab = atoll(val()); haveSlab = true; }
		else if(a == "--rarefy") { rarefy = atoll(val()); haveRarefy = true; }
		else if(a == "--reps") { reps = atoll(val()); haveReps = true; }
		else if(a == "-S" || a == "--seed") { seed = strtoull(val(), nullptr, 10); haveSeed = true; }
		else if(a == "--sd-out") sdFn = val();
		else if(a == "--draw-chunk") { drawChunk = atoll(val()); haveDrawChunk = true; }
		else if(a == "--chunk") { chunk = atoll(val()); haveChunk = true; }
		else if(a == "--mem") { memGb = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a.compare(0, 2, "-v") == 0) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	static const char* const names[] = {"unweighted", "weighted", "weighted-raw", "generalized", "bray-curtis", "jaccard"};
	o.method = -1;
	for(int m = 0; m < 6; ++m) if(method == names[m]) o.method = m;
	if(o.method < 0) { std::cerr << "Unsupported method '" << method << "': unweighted, weighted, weighted-raw, generalized, bray-curtis or jaccard" << std::endl; return EXIT_FAILURE; }
	const bool identity = o.method == HU_UF_BRAY_CURTIS || o.method == HU_UF_JACCARD;
	if(!identity && dbName.empty()) { std::cerr << "--db is required by the method '" << method << "': its distances are taken on the tree of the database" << std::endl; return EXIT_FAILURE; }
	if(identity && !dbName.empty()) { std::cerr << "--db does not go with the method '" << method << "', which reads no tree" << std::endl; return EXIT_FAILURE; }
	if(haveAlpha && o.method != HU_UF_GENERALIZED) { std::cerr << "--alpha goes with --method generalized only" << std::endl; return EXIT_FAILURE; }
	if(haveAlpha && !(o.alpha >= 0 && o.alpha <= 1)) { std::cerr << "--alpha must lie between 0 and 1" << std::endl; return EXIT_FAILURE; }
	if(haveSlab && slab < 1) { std::cerr << "--slab must be at least 1" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	if(!haveRarefy) {
		const char* lone = haveReps ? "--reps" : haveSeed ? "--seed" : !sdFn.empty() ? "--sd-out" : haveDrawChunk ? "--draw-chunk" : haveChunk ? "--chunk" : haveMem ? "--mem" : nullptr;
		if(lone) { std::cerr << lone << " goes with --rarefy only" << std::endl; return EXIT_FAILURE; }
	}
	else {
		if(!pdFn.empty()) { std::cerr << "--pd does not go with --rarefy: hmmufotu-amd-alpha gives Faith's PD of rarefied draws" << std::endl; return EXIT_FAILURE; }
		if(rarefy < 1) { std::cerr << "--rarefy must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(reps < 1 || reps > HU_UFR_MAX_REPS) { std::cerr << "--reps must lie between 1 and " << HU_UFR_MAX_REPS << std::endl; return EXIT_FAILURE; }
		if(haveDrawChunk && drawChunk < 1) { std::cerr << "--draw-chunk must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(haveChunk && (chunk < 1 || chunk > (1 << 24))) { std::cerr << "--chunk must lie between 1 and " << (1 << 24) << std::endl; return EXIT_FAILURE; }
		if(haveMem && !(memGb > 0)) { std::cerr << "--mem must be positive" << std::endl; return EXIT_FAILURE; }
	}
	o.slab = slab; o.host = host ? 1 : 0;
	if(verbose) std::cerr << "Loading OTUTable" << std::endl;
	hu_otu_table* t = nullptr;
	if(hu_otu_table_read(pos[0].c_str(), &t) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	int64_t M = 0, S = 0;
	hu_otu_table_dims(t, &M, &S);
	if(S < 1) { std::cerr << "'" << pos[0] << "' is a table without samples" << std::endl; return EXIT_FAILURE; }
	const double* cnt = hu_otu_table_counts(t);
	for(int64_t j = 0; j < S; ++j) {
		double tot = 0;
		for(int64_t i = 0; i < M; ++i) {
			const double v = cnt[i * S + j];
			if(!(v >= 0) || !std::isfinite(v)) { std::cerr << "OTU '" << hu_otu_table_otu(t, i) << "' has a cell that is negative or not finite in sample '" << hu_otu_table_sample(t, j) << "'" << std::endl; return EXIT_FAILURE; }
			tot += v;
		}
		if(!(tot > 0)) { std::cerr << "Sample '" << hu_otu_table_sample(t, j) << "' has no reads: hmmufotu-amd-subset drops such samples" << std::endl; return EXIT_FAILURE; }
	}
	std::vector<int32_t> parent, otuNode; std::vector<double> blen;
	hu_unifrac_tree tree; memset(&tree, 0, sizeof(tree));
	if(!identity) {
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
	std::vector<double> dist((size_t) S * S), pd(pdFn.empty() ? 0 : (size_t) S), sd;
	const int dev = host ? -1 : device;
	std::vector<int64_t> cols;                                          /* the samples of the matrix: with --rarefy the kept ones */
	if(haveRarefy) {
		hu_unifrac_rarefied_opts ro;
		hu_unifrac_rarefied_default_opts(&ro);
		ro.method = o.method; ro.host = o.host; ro.alpha = o.alpha; ro.slab = o.slab; ro.draw_chunk = drawChunk;
		if(haveChunk) ro.chunk = (int32_t) chunk;
		if(haveMem) ro.mem_budget = (int64_t)(memGb * 1073741824.0);
		std::vector<uint8_t> kept((size_t) S);
		sd.resize((size_t) S * S);
		if(hu_unifrac_rarefied(dev, identity ? nullptr : &tree, M, S, identity ? nullptr : otuNode.data(), cnt, (uint64_t) rarefy, reps, seed, &ro, kept.data(),
				dist.data(), sd.data(), nullptr) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		for(int64_t j = 0; j < S; ++j) {
			if(kept[(size_t) j]) cols.push_back(j);
			else std::cerr << "Sample '" << hu_otu_table_sample(t, j) << "' has fewer than " << rarefy << " reads: dropped" << std::endl;
		}
		if(verbose) {
			int64_t sz[8];
			hu_unifrac_rarefied_sizes(identity ? nullptr : &tree, M, S, identity ? nullptr : otuNode.data(), cnt, (uint64_t) rarefy, reps, &ro, sz);
			std::cerr << cols.size() << " samples kept, " << S - (int64_t) cols.size() << " dropped, B = " << sz[5] << " kept branches, L = " << sz[6] << " branches per slab, "
				<< reps << " draws of " << rarefy << " reads" << std::endl;
			if(!host) {
				double s[6]; int64_t resident = 0;
				hu_unifrac_rarefied_timing(s, &resident);
				std::cerr << resident << " draws resident at once; copies up " << s[0] << " s, draws " << s[1] << " s, embedding " << s[2] << " s, pair kernel " << s[3]
					<< " s, accumulate " << s[4] << " s, copy back " << s[5] << " s" << std::endl;
			}
		}
	}
	else if(hu_unifrac(dev, identity ? nullptr : &tree, M, S, identity ? nullptr : otuNode.data(), cnt, &o, dist.data(), pdFn.empty() ? nullptr : pd.data()) != HU_OK) {
		std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
	if(!haveRarefy) for(int64_t j = 0; j < S; ++j) cols.push_back(j);
	const int64_t K = (int64_t) cols.size();
	if(verbose && !haveRarefy) {
		int64_t B = 0;
		hu_unifrac_embed(dev, identity ? nullptr : &tree, M, S, identity ? nullptr : otuNode.data(), cnt, &o, &B, 0, nullptr, nullptr, nullptr);
		const int64_t L = o.slab > 0 ? o.slab : hu_unifrac_default_slab(S, B), nt = (S + 63) / 64;
		std::cerr << "B = " << B << " kept branches, L = " << L << " branches per slab, " << nt * (nt + 1) / 2 << " tiles" << std::endl;
		if(!host) {
			double s[4];
			hu_unifrac_timing(s);
			std::cerr << "copies up " << s[0] << " s, embedding " << s[1] << " s, pair kernel " << s[2] << " s, copy back " << s[3] << " s" << std::endl;
		}
	}
	auto writeAll = [&](std::ostream& out, const std::vector<double>& d) {
		for(int64_t j = 0; j < K; ++j) out << '\t' << hu_otu_table_sample(t, cols[(size_t) j]);
		out << '\n';
		for(int64_t i = 0; i < K; ++i) {
			out << hu_otu_table_sample(t, cols[(size_t) i]);
			for(int64_t j = 0; j < K; ++j) { const double v = d[(size_t)(i * K + j)]; out << '\t' << (std::isnan(v) ? std::string("NA") : num17(v)); }
			out << '\n';
		}
	};
	if(outFn.empty()) writeAll(std::cout, dist);
	else {
		std::ofstream f(outFn);
		if(!f) { std::cerr << "Unable to write to '" << outFn << "'" << std::endl; return EXIT_FAILURE; }
		writeAll(f, dist);
	}
	if(!sdFn.empty()) {
		std::ofstream f(sdFn);
		if(!f) { std::cerr << "Unable to write to '" << sdFn << "'" << std::endl; return EXIT_FAILURE; }
		writeAll(f, sd);
	}
	if(!pdFn.empty()) {
		std::ofstream f(pdFn);
		if(!f) { std::cerr << "Unable to write to '" << pdFn << "'" << std::endl; return EXIT_FAILURE; }
		for(int64_t j = 0; j < S; ++j) f << hu_otu_table_sample(t, j) << '\t' << num17(pd[(size_t) j]) << '\n';
	}
	hu_otu_table_free(t);
	return EXIT_SUCCESS;
}
