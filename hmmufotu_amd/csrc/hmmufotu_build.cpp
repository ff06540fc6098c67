// hmmufotu-amd-build: a <NAME>.ptu database from a reference MSA and its phylogenetic tree — the --no-hmm mode of hmmufotu-build
// (src/hmmufotu-build.cpp:307-503 without the hmm and msa parts), and with --csfm its seed index file <NAME>.csfm (csfm.build(msa), :320-328, and
// csfm.save, :479-485).  The host reads and joins the inputs; the wide loops run on
// the device: the MSA column counts behind MSA::prune (hu_msa_stats), the tree evaluated at every root (hu_tree_evaluate), the
// per-site mutation counts behind -V (hu_tree_count_mutations), the tree log-likelihood (hu_tree_loglik) and the gather of the
// messages for the file (hu_ptu_write_stream); with --col-window the same a window of columns at a time, for a message set beyond the device's
// memory (hu_tree_sweep_*, hu_ptu_writer_*); with --csfm the suffix array of the concatenated MSA rows, its BWT and samples (hu_csfm_write).  Options and inputs are checked, and every input read and joined, before a device
// is asked for.
//   hmmufotu-amd-build <MSA-FILE> <TREE-FILE> --no-hmm -sm FILE [-n NAME] [--fmt fasta] [-a|--anno FILE] [-r|--root STR] [-V|--var]
//                      [-k INT] [--csfm] [--col-window W|auto] [--mem GB] [--device N] [-v]
// Writes <NAME>.ptu, and <NAME>.csfm when asked (without it hmmufotu-amd rebuilds its seed index from the .ptu on every start; the reference's
// hmmufotu cannot start without it): no .msa, and no .hmm — the profile comes
// from a third-party trainer (HMMER3, hmmufotu-train-hmm) and is put beside the .ptu as <NAME>.hmm.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <sys/stat.h>
#include <unistd.h>
#include "hu_build_inputs.h"     /* the reading, joining and pruning shared with hmmufotu-amd-train-sm */

/* src/hmmufotu-build.cpp:59-61 */
static const int DEFAULT_DG_CATEGORY = 4, MIN_DG_CATEGORY = 2, MAX_DG_CATEGORY = 8;

static void usage(const char* p) {
	std::cerr << "Build the phylogenetic-tree database (.ptu) of an HmmUFOtu database from reference MSA and phylogenetic tree files\n"
		"Usage:    " << p << "  <MSA-FILE> <TREE-FILE> --no-hmm -sm FILE [options]\n"
		"MSA-FILE  FILE                   : multiple-sequence aligned (MSA) input, support .gz or .bz2 compressed file\n"
		"TREE-FILE  FILE                  : phylogenetic-tree file build on the MSA sequences (.tree / .tre)\n"
		"Options:    --no-hmm FLAG        : required: the Hmm profile is built by 3rd party programs, i.e. HMMER3, and supplied as <NAME>.hmm\n"
		"            -sm  FILE            : trained DNA Substitution Model, required\n"
		"            -n  STR              : database name (prefix), use 'MSA-FILE' by default\n"
		"            --fmt  STR           : MSA format, supported format: 'fasta'\n"
		"            -a|--anno  FILE      : use tab-delimited taxonamy annotation file for the sequences in the MSA and TREE files\n"
		"            -r|--root  STR       : root name if the original tree root is not named [cellular_organisms]\n"
		"            -V|--var FLAG        : enable among-site rate varation evaluation of the tree, using a Discrete Gamma Distribution based model\n"
		"            -k INT               : number of Discrete Gamma Distribution categories to evaluate the tree, ignored if -V not set [" << DEFAULT_DG_CATEGORY << "]\n"
		"            --csfm FLAG          : also write the seed index file <NAME>.csfm, over all rows of the pruned MSA (the suffix array is built on the device)\n"
		"            --col-window  INT|auto : evaluate and write the tree in windows of INT columns, so that only 64 x nodes x INT bytes of messages are on the device at once; 'auto': the widest window that fits, none when everything fits\n"
		"            --mem  GB            : device memory the build may use, in GB [what the device reports free]\n"
		"            --device  INT        : device index [0]\n"
		"            -f|--symfrac, -dm, -p|--process : accepted and ignored (they belong to the profile training)\n"
		"            -v  FLAG             : enable verbose information; -vv adds the wall time of every phase\n"
		"            -h|--help            : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string dbName, fmt, annoFn, smFn, smType, rootName = "cellular_organisms";
	bool noHmm = false, isVar = false, haveS = false, withCsfm = false;
	int K = DEFAULT_DG_CATEGORY, device = 0, verbose = 0;
	std::vector<std::string> ignored;
	std::string colWinArg, memArg; bool haveColWin = false, haveMem = false;
	if(argc == 1) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and build semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-n") dbName = val(); else if(a == "--fmt") fmt = val();
		else if(a == "-a" || a == "--anno") annoFn = val(); else if(a == "-r" || a == "--root") rootName = val();
		else if(a == "-s" || a == "--sub-model") { smType = val(); haveS = true; }
		else if(a == "-sm") smFn = val();
		else if(a == "--no-hmm") noHmm = true; else if(a == "--csfm") withCsfm = true; else if(a == "-V" || a == "--var") isVar = true;
		else if(a == "-k") K = atoi(val()); else if(a == "--device") device = atoi(val());
		else if(a == "--col-window") { colWinArg = val(); haveColWin = true; } else if(a == "--mem") { memArg = val(); haveMem = true; }
		else if(a == "-f" || a == "--symfrac" || a == "-dm" || a == "-p" || a == "--process") { ignored.push_back(a); val(); }
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	auto info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	/* -vv: wall time of every phase, for profiles/build_program_rate.py */
	auto tLap = std::chrono::steady_clock::now();
	auto lap = [&](const char* phase) {
		const auto now = std::chrono::steady_clock::now();
		if(verbose > 1) std::cerr << "[phase] " << phase << ": " << std::chrono::duration<double>(now - tLap).count() << " s" << std::endl;
		tLap = now;
	};
	const std::string seqFn = pos[0], treeFn = pos[1];
	if(!noHmm) { std::cerr << "profile training is not provided here; pass --no-hmm and supply <NAME>.hmm (HMMER3 or hmmufotu-train-hmm)" << std::endl; return EXIT_FAILURE; }
	if(smFn.empty()) {
		if(haveS) std::cerr << "-s|--sub-model " << smType << ": the built-in models are read from the reference's installed data directory, which is not shipped here; pass the trained model with -sm FILE" << std::endl;
		else std::cerr << "-sm FILE must be specified: the built-in models of the reference's data directory are not shipped here" << std::endl;
		return EXIT_FAILURE;
	}
	/* guess input format (src/hmmufotu-build.cpp:198-208) */
	hu_guess_seq_format(seqFn, fmt);
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }
	if(!hu_is_newick_name(treeFn)) { std::cerr << "Unrecognized TREE-FILE format, must be in Newick format" << std::endl; return EXIT_FAILURE; }
	if(!(MIN_DG_CATEGORY <= K && K <= MAX_DG_CATEGORY)) { std::cerr << "-k must be an integer between " << MIN_DG_CATEGORY << " and " << MAX_DG_CATEGORY << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative" << std::endl; return EXIT_FAILURE; }
	int64_t colWin = -1, memBytes = 0;            /* colWin: -1 not asked for, 0 auto, else the width */
	if(haveColWin && colWinArg != "auto") {
		char* end = nullptr;
		errno = 0;
		const long long v = strtoll(colWinArg.c_str(), &end, 10);
		if(colWinArg.empty() || *end || errno || v < 1) { std::cerr << "--col-window must be 'auto' or an integer >= 1, got '" << colWinArg << "'" << std::endl; return EXIT_FAILURE; }
		colWin = v;
	}
	else if(haveColWin) colWin = 0;
	if(haveMem) {
		char* end = nullptr;
		const double gb = strtod(memArg.c_str(), &end);
		if(memArg.empty() || *end || !(gb > 0) || !std::isfinite(gb) || gb * 1e9 >= 9e18) { std::cerr << "--mem must be a positive number of GB, got '" << memArg << "'" << std::endl; return EXIT_FAILURE; }
		memBytes = (int64_t)(gb * 1e9);
	}
	for(const std::string& o : ignored) info("Note: " + o + " belongs to the profile training and is ignored under --no-hmm");

	/* open and read the inputs */
	LineIn seqIn;
	if(!seqIn.open(seqFn)) { std::cerr << "Unable to open seq file '" << seqFn << "' " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	std::string smText, treeText, annoText;
	if(!read_file(smFn, smText)) { std::cerr << "Unable to open '" << smFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	if(!read_file(treeFn, treeText)) { std::cerr << "Unable to open '" << treeFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	if(!annoFn.empty() && !read_file(annoFn, annoText)) { std::cerr << "Unable to open '" << annoFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	if(dbName.empty()) dbName = seqFn.substr(seqFn.find_last_of('/') + 1);      /* StringUtils::basename(seqFn) */
	const std::string ptuFn = dbName + ".ptu", csfmFn = dbName + ".csfm";

	/* the MSA, the tree, and loadMSA: every leaf takes the row of its name */
	HuBuildInputs inp;
	if(!hu_load_msa(seqIn, seqFn, dbName, inp, info)) return EXIT_FAILURE;
	const size_t nSeq = inp.nSeq, L0 = inp.L0;
	std::vector<char>& msa = inp.msa;
	lap("read");
	if(!hu_load_tree(treeText, treeFn, inp, info)) return EXIT_FAILURE;
	const int32_t n = inp.n;
	std::vector<int32_t> &parent = inp.parent, &childOff = inp.childOff, &childIdx = inp.childIdx, &rowOf = inp.rowOf;
	std::vector<double>& blen = inp.blen;
	std::vector<std::string>& nodeName = inp.nodeName;
	if(n < 2) { std::cerr << "Unable to build a database from a tree of " << n << " node" << std::endl; return EXIT_FAILURE; }
	if(!hu_join_msa_tree(inp, info)) return EXIT_FAILURE;

	info("Verifying and fixing branch length");
	for(int32_t i = 0; i < n; ++i) if(parent[i] >= 0 && childOff[i] == childOff[i + 1] && blen[i] <= 0) blen[i] = 1e-5;     /* fixBranchLength, BRANCH_EPS */

	/* annotation */
	hu_tree_anno* an = nullptr;
	{
		std::vector<const char*> nm(n);
		for(int32_t i = 0; i < n; ++i) nm[i] = nodeName[i].c_str();
		if(hu_tree_annotate(n, parent.data(), blen.data(), nm.data(), annoFn.empty() ? nullptr : annoText.data(), (int64_t) annoText.size(), rootName.c_str(), &an) != HU_OK) {
			std::cerr << "Failed to load taxonomy annotation from '" << annoFn << "': " << hu_last_error() << std::endl; return EXIT_FAILURE;
		}
	}
	if(!annoFn.empty()) info("Taxonomy annotation loaded");
	info("Taxon names formatted");
	info("Unnamed tree nodes annotated");
	lap("join");
	std::vector<const char*> names(n), annos(n);
	std::vector<double> annoDist(n);
	for(int32_t i = 0; i < n; ++i) { names[i] = hu_tree_anno_name(an, i); annos[i] = hu_tree_anno_anno(an, i); }
	hu_tree_anno_dist(an, annoDist.data());

	/* the model: the type is the word behind "Type:" (src/hmmufotu-build.cpp:393-405) */
	hu_model_desc model;
	{
		std::istringstream in(smText);
		std::string tag, type, line;
		while(in >> tag) { if(tag[0] == '#') { std::getline(in, line); continue; } if(tag == "Type:") { in >> type; break; } }
		const std::string withType = type + "\n" + smText;
		if(type.empty() || hu_model_parse_text(withType.data(), (int64_t) withType.size(), &model) != HU_OK) {
			std::cerr << "Unable to load DNA Substitution Model from: '" << smFn << "'" << (type.empty() ? "" : std::string(": ") + hu_last_error()) << std::endl; hu_tree_anno_free(an); return EXIT_FAILURE;
		}
	}
	model.dg_k = 0;
	info("DNA Substitution Model loaded");

	/* the output, then the device */
	struct stat stBefore;
	const bool existed = stat(ptuFn.c_str(), &stBefore) == 0;
	{ std::ofstream probe(ptuFn, std::ios::binary | std::ios::app); if(!probe.is_open()) { std::cerr << "Unable to write to '" << ptuFn << "': " << strerror(errno) << std::endl; hu_tree_anno_free(an); return EXIT_FAILURE; } }
	struct stat stCsfm;
	const bool csfmExisted = withCsfm && stat(csfmFn.c_str(), &stCsfm) == 0;
	if(withCsfm) { std::ofstream probe(csfmFn, std::ios::binary | std::ios::app); if(!probe.is_open()) { std::cerr << "Unable to write to '" << csfmFn << "': " << strerror(errno) << std::endl; hu_tree_anno_free(an); if(!existed) unlink(ptuFn.c_str()); return EXIT_FAILURE; } }
	void *dUp = nullptr, *dDown = nullptr;
	hu_tree_sweep* sweep = nullptr; hu_ptu_writer* writer = nullptr;
	auto fail = [&](const std::string& msg) {
		std::cerr << msg << std::endl;
		hu_ptu_writer_abort(writer); hu_tree_sweep_destroy(sweep);
		hu_device_free(device, dUp); hu_device_free(device, dDown); hu_tree_anno_free(an);
		if(!existed) unlink(ptuFn.c_str());       /* only the probe's empty file */
		if(withCsfm && !csfmExisted) unlink(csfmFn.c_str());
		return EXIT_FAILURE;
	};
	if(hu_device_count() <= device) return fail("Error: device " + std::to_string(device) + " asked for, " + std::to_string(hu_device_count()) + " gfx950 device(s) visible");

	/* MSA::prune: the columns without a residue go (hu_msa_stats counts them on the device) */
	std::vector<int8_t> seq;
	int32_t L = 0;
	{
		std::string err;
		if(!hu_prune_msa(device, inp, info, err)) return fail("Error: " + err);
		const std::vector<int32_t>& res = inp.res; const std::vector<double> &wres = inp.wres, &wgap = inp.wgap; const std::vector<uint32_t>& keep = inp.keep;
		L = inp.L;
		if(L < 1) return fail("Unable to build a database: the MSA has no column with a residue");
		if(L > 65535) return fail("Unable to build a database: " + std::to_string(L) + " columns after pruning, the .ptu readers take at most 65535");
		int8_t enc[256];
		hu_msa_encode_table(enc);
		seq.assign((size_t) n * L, (int8_t) 0);
		for(int32_t i = 0; i < n; ++i) if(rowOf[i] >= 0) hu_encode_row(inp, enc, (size_t) rowOf[i], seq.data() + (size_t) i * L);
		if(withCsfm) { /* csfm.build(msa) over ALL rows of the pruned MSA in file order, csSeq from the weighted counts (MSA::calculateCS, src/MSA.cpp:211-226),
		                * csIdentity from the raw ones (identityAt, :59-61) */
			std::vector<char> rows(nSeq * (size_t) L);
			for(size_t i = 0; i < nSeq; ++i) { const char* src = msa.data() + i * L0; char* dst = rows.data() + i * (size_t) L; for(int32_t j = 0; j < L; ++j) dst[j] = src[keep[j]]; }
			std::string cs((size_t) L, '-');
			std::vector<double> ident((size_t) L);
			for(int32_t j = 0; j < L; ++j) {
				const size_t c = keep[j];
				int best = 0, rawMax = res[c];
				for(int b = 1; b < 4; ++b) { if(wres[b * L0 + c] > wres[best * L0 + c]) best = b; rawMax = std::max(rawMax, res[b * L0 + c]); }
				if(wres[best * L0 + c] >= wgap[c]) cs[j] = "ACGT"[best];
				ident[j] = rawMax / static_cast<double>(nSeq);
			}
			if(hu_csfm_write(csfmFn.c_str(), (int64_t) nSeq, L, rows.data(), cs.c_str(), ident.data(), device) != HU_OK) return fail(std::string("Unable to build CSFM index: ") + hu_last_error());
			info("CSFM index built");
			info("CSFM saved");                     /* the reference saves it with the other files at the end; here it is written while the device is still free */
			lap("csfm");
		}
	}
	std::vector<char>().swap(msa);
	lap("stats");

	/* device memory: both message sets, and the largest of the later steps' scratch: the sweep's node rows and tables, the mutation count's
	 * states, the writer's staging buffers */
	int32_t W = 0;                                /* the window width of a windowed build; 0: everything resident */
	{
		int64_t freeB = 0, totB = 0;
		if(hu_device_mem_info(device, &freeB, &totB) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
		if(haveMem) freeB = std::min(freeB, memBytes);
		const int64_t msgs = 2ll * n * L * 32, sweep = (int64_t) n * L + (int64_t) n * 28 + 64, mut = isVar ? (int64_t) n * L + (int64_t) n * 4 + (int64_t) L * 4 : 0;
		const int64_t stage = 2 * std::min<int64_t>((int64_t) 256 << 20, (2ll * n - 1) * L * 32) + 8ll * n;     /* hu_ptu_write_stream's two staging buffers */
		const int64_t need = msgs + std::max(std::max(sweep, mut), stage) + (int64_t) L * 8;
		char buf[320];
		if(colWin > 0 && colWin < L) {
			W = (int32_t) colWin;
			const int64_t needW = hu_build_window_need(n, W, isVar);
			if(needW > freeB) {
				snprintf(buf, sizeof(buf), "Unable to build the database on device %d: %d nodes x windows of %d columns need %.3f GB of device memory, %.3f GB are free (--col-window auto chooses a width that fits)", device, n, W, needW / 1e9, freeB / 1e9);
				return fail(buf);
			}
		}
		else if(colWin == 0 && need > freeB) {
			int64_t needW = 0;
			if(hu_build_window_plan(n, L, isVar, freeB, &W, &needW) != HU_OK) {
				snprintf(buf, sizeof(buf), "Unable to build the database on device %d: one column of %d nodes needs %.6f GB of device memory, %.6f GB are free", device, n, needW / 1e9, freeB / 1e9);
				return fail(buf);
			}
			if(W >= L) W = 0;
		}
		else if(need > freeB) {
			snprintf(buf, sizeof(buf), "Unable to build the database on device %d: %d nodes x %d columns need %.3f GB of device memory, %.3f GB are free (--col-window auto builds it in column windows)", device, n, L, need / 1e9, freeB / 1e9);
			return fail(buf);
		}
		if(W == 0 && (hu_device_malloc(device, msgs / 2, &dUp) != HU_OK || hu_device_malloc(device, msgs / 2, &dDown) != HU_OK)) return fail(std::string("Error: ") + hu_last_error());
	}
	if(W > 0) { /* the windowed build: the resident one below, a window of columns at a time */
		const int32_t nWin = (L + W - 1) / W;
		if(verbose) std::cerr << "Building in " << nWin << " column windows of " << W << " columns" << std::endl;
		auto err = [&]() { return std::string("Error: ") + hu_last_error(); };
		std::vector<double> height(n), perCol((size_t) L);
		if(hu_tree_sweep_create(n, L, parent.data(), blen.data(), device, &sweep) != HU_OK) return fail(err());
		if(hu_device_malloc(device, (int64_t) n * W * 32, &dUp) != HU_OK) return fail(err());
		info(std::string("Evaluating Phylogenetic Tree at root id: 0") + (isVar ? " with fixed rate model first" : ""));
		double alpha = 0;
		std::vector<double> breaks;
		if(isVar) { /* pass 1: the post-order levels and the mutation counts of every window, joined in column order */
			info("Estimating the shape parameter of the Discrete Gamma Distributin based among-site variation ...");
			std::vector<int32_t> cnt(L);
			for(int32_t a = 0; a < L; a += W) {
				const int32_t wl = std::min(W, L - a);
				if(hu_tree_sweep_window(sweep, &model, seq.data(), a, wl, (double*) dUp, nullptr) != HU_OK) return fail(err());
				if(hu_tree_count_mutations(device, n, wl, parent.data(), (const double*) dUp, cnt.data() + a) != HU_OK) return fail(err());
			}
			std::vector<double> numMut(cnt.begin(), cnt.end());
			alpha = hu_dg_estimate_shape(L, numMut.data());
			lap("first sweep and mutation count");
			if(alpha == std::numeric_limits<double>::infinity()) std::cerr << "Unable to estimate the shape parameter with less than 2 alignment sites" << std::endl;
			else if(!(alpha > 0)) std::cerr << "Unable to estimate the shape parameter with near invariant rates, reducing to fixed rate model" << std::endl;
			else {
				if(verbose) std::cerr << "Estimated alpha = " << alpha << std::endl;
				breaks.resize((size_t) K + 1);
				if(hu_dg_model(K, alpha, breaks.data(), model.dg_rate) != HU_OK) return fail(err());
				model.dg_k = K;
			}
			for(int32_t i = 0; i < n; ++i) if(rowOf[i] < 0) memset(seq.data() + (size_t) i * L, 0, (size_t) L);
		}
		info(model.dg_k == 0 ? "Evaluating Phylogenetic Tree at all other " + std::to_string(n - 1) + " nodes" : "Re-evaluating Phylogenetic Tree at all " + std::to_string(n) + " nodes");
		if(hu_device_malloc(device, (int64_t) n * W * 32, &dDown) != HU_OK) return fail(err());
		hu_tree_desc td;
		memset(&td, 0, sizeof(td));
		td.n_nodes = n; td.cs_len = L; td.parent = parent.data(); td.blen = blen.data(); td.anno_dist = annoDist.data();
		if(hu_ptu_writer_open(ptuFn.c_str(), &td, names.data(), annos.data(), childOff.data(), childIdx.data(), rowOf.data(), 0, &writer) != HU_OK)
			return fail(std::string("Unable to save Phylogenetic Tree index: ") + hu_last_error());
		double tSweep = 0, tLik = 0, tWrite = 0;
		auto since = [](std::chrono::steady_clock::time_point& t0) { const auto now = std::chrono::steady_clock::now(); const double d = std::chrono::duration<double>(now - t0).count(); t0 = now; return d; };
		for(int32_t a = 0; a < L; a += W) { /* pass 2: the full sweep under the final model, the column log-likelihoods, the window to the file */
			const int32_t wl = std::min(W, L - a);
			auto t0 = std::chrono::steady_clock::now();
			double part = 0;
			if(hu_tree_sweep_window(sweep, &model, seq.data(), a, wl, (double*) dUp, (double*) dDown) != HU_OK) return fail(err());
			tSweep += since(t0);
			if(hu_tree_loglik(device, n, wl, 0, &model, (const double*) dUp, perCol.data() + a, &part) != HU_OK) return fail(err());
			tLik += since(t0);
			if(hu_ptu_writer_window(writer, a, wl, (const double*) dUp, (const double*) dDown, 1) != HU_OK) return fail(std::string("Unable to save Phylogenetic Tree index: ") + hu_last_error());
			tWrite += since(t0);
		}
		if(verbose > 1) std::cerr << "[phase] second sweep: " << tSweep << " s\n[phase] log-likelihood: " << tLik << " s\n[phase] write windows: " << tWrite << " s" << std::endl;
		tLap = std::chrono::steady_clock::now();
		if(hu_tree_sweep_heights(sweep, height.data()) != HU_OK) return fail(err());
		info("Node height calculated");
		double loglik = 0;
		for(int32_t j = 0; j < L; ++j) loglik += perCol[j];     /* serial column order over all windows: the resident build's sum */
		if(verbose) std::cerr << "Final Tree log-liklihood: " << loglik << std::endl;
		info("Ancestor sequence of all intermediate nodes inferred");
		info("Saving database files ...");
		hu_ptu_writer* w = writer;
		writer = nullptr;                            /* close frees the handle whatever happens */
		if(hu_ptu_writer_close(w, seq.data(), height.data(), &model, smText.c_str(), alpha, model.dg_k ? breaks.data() : nullptr) != HU_OK)
			return fail(std::string("Unable to save Phylogenetic Tree index: ") + hu_last_error());
		info("Phylogenetic Tree index saved");
		lap("write");
		hu_tree_sweep_destroy(sweep); hu_device_free(device, dUp); hu_device_free(device, dDown); hu_tree_anno_free(an);
		return EXIT_SUCCESS;
	}
	std::vector<double> height(n);
	info(std::string("Evaluating Phylogenetic Tree at root id: 0") + (isVar ? " with fixed rate model first" : ""));
	if(hu_tree_evaluate(n, L, parent.data(), blen.data(), seq.data(), &model, device, 0, 0, (double*) dUp, (double*) dDown, height.data()) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
	info("Node height calculated");
	lap("first sweep");
	double alpha = 0;
	std::vector<double> breaks;
	if(isVar) { /* src/hmmufotu-build.cpp:431-447 */
		info("Estimating the shape parameter of the Discrete Gamma Distributin based among-site variation ...");
		std::vector<int32_t> cnt(L);
		if(hu_tree_count_mutations(device, n, L, parent.data(), (const double*) dUp, cnt.data()) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
		std::vector<double> numMut(cnt.begin(), cnt.end());
		alpha = hu_dg_estimate_shape(L, numMut.data());
		lap("mutation count");
		if(alpha == std::numeric_limits<double>::infinity()) std::cerr << "Unable to estimate the shape parameter with less than 2 alignment sites" << std::endl;
		else if(!(alpha > 0)) std::cerr << "Unable to estimate the shape parameter with near invariant rates, reducing to fixed rate model" << std::endl;
		else {
			if(verbose) std::cerr << "Estimated alpha = " << alpha << std::endl;
			breaks.resize((size_t) K + 1);
			if(hu_dg_model(K, alpha, breaks.data(), model.dg_rate) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
			model.dg_k = K;
		}
	}
	if(model.dg_k == 0) info("Evaluating Phylogenetic Tree at all other " + std::to_string(n - 1) + " nodes");     /* the sweep above left every directed edge's message */
	else {
		info("Re-evaluating Phylogenetic Tree at all " + std::to_string(n) + " nodes");
		for(int32_t i = 0; i < n; ++i) if(rowOf[i] < 0) memset(seq.data() + (size_t) i * L, 0, (size_t) L);
		if(hu_tree_evaluate(n, L, parent.data(), blen.data(), seq.data(), &model, device, 0, 0, (double*) dUp, (double*) dDown, height.data()) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
	}
	lap("second sweep");
	double loglik = 0;
	if(hu_tree_loglik(device, n, L, 0, &model, (const double*) dUp, nullptr, &loglik) != HU_OK) return fail(std::string("Error: ") + hu_last_error());
	if(verbose) std::cerr << "Final Tree log-liklihood: " << loglik << std::endl;
	info("Ancestor sequence of all intermediate nodes inferred");
	lap("log-likelihood");

	info("Saving database files ...");
	hu_tree_desc td;
	memset(&td, 0, sizeof(td));
	td.n_nodes = n; td.cs_len = L; td.parent = parent.data(); td.blen = blen.data(); td.seq = seq.data(); td.up = (const double*) dUp; td.down = (const double*) dDown;
	td.height = height.data(); td.anno_dist = annoDist.data(); td.msgs_on_device = 1;
	if(hu_ptu_write_stream(ptuFn.c_str(), &td, names.data(), annos.data(), &model, smText.c_str(), alpha, model.dg_k ? breaks.data() : nullptr,
			childOff.data(), childIdx.data(), rowOf.data(), 0) != HU_OK) {
		std::cerr << "Unable to save Phylogenetic Tree index: " << hu_last_error() << std::endl;
		hu_device_free(device, dUp); hu_device_free(device, dDown); hu_tree_anno_free(an);
		unlink(ptuFn.c_str());
		if(withCsfm && !csfmExisted) unlink(csfmFn.c_str());
		return EXIT_FAILURE;
	}
	info("Phylogenetic Tree index saved");
	lap("write");
	hu_device_free(device, dUp); hu_device_free(device, dDown); hu_tree_anno_free(an);
	return EXIT_SUCCESS;
}
