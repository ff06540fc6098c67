// hmmufotu-amd-train-dm: the Dirichlet prior file (.dm) of hmmufotu-amd-train-hmm trained on a reference MSA — hmmufotu-train-dm
// (src/hmmufotu-train-dm.cpp:88-374).  The host reads and prunes the MSA exactly as hmmufotu-amd-train-hmm does (hu_build_inputs.h);
// the five training sets are counted on the device (hu_dm_training_data); every model starts from a moment fit on the host
// (hu_dm_shuffle, hu_dm_moment_init); the -n match-emission mixtures and the four densities are trained side by side on the device
// (hu_dm_train, one workgroup each); the mixture of the smallest finite cost is kept and the file written (hu_dm_write).
// One difference from the reference, which trains one model object for every seed so that seed i > 1 starts from what seed i - 1
// left: here every seed starts fresh (q = 1 / qM, alpha = 1 where the fit fails) and only its shuffle continues the rand() stream.
// Seed 1, and so every run with -n 1, follows the reference.  DESIGN.md §16.
//   hmmufotu-amd-train-dm <MSA-FILE> [-o FILE] [--fmt fasta] [-qM 5] [-symfrac 0.5] [--max-it 0] [--pri-rate 0.05] [-s|--seed INT] [-n 1] [--device N] [--chunk 64] [-v]
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <ctime>
#include "hu_build_inputs.h"

/* the parts of hu_build_inputs.h that need a tree are for the other programs */
static const auto unused_tree [[maybe_unused]] = &hu_load_tree;
static const auto unused_join [[maybe_unused]] = &hu_join_msa_tree;
static const auto unused_newick [[maybe_unused]] = &hu_is_newick_name;
static const auto unused_encode [[maybe_unused]] = &hu_encode_row;
static const auto unused_file [[maybe_unused]] = &read_file;

static const int DEFAULT_QM = 5;               /* src/hmmufotu-train-dm.cpp:49-54 */
static const double DEFAULT_SYMFRAC = 0.5;
static const int MAX_NUM_COMPO = 10;
static const double DEFAULT_PRI_RATE = 0.05;
static const int DEFAULT_NSEED = 1;
static const int MAX_NSEED = 4092;             /* with the four densities: the batch hu_dm_train takes */
static const size_t MAX_CS = 65535;            /* as hmmufotu-amd-train-hmm: the profile these priors are for ends there */

static void usage(const char* p) {
	std::cerr << "Train an HmmUFOtu prior model using Dirichlet Density/Mixture models with customized data\n"
		"Usage:    " << p << "  <MSA-FILE> [options]\n"
		"MSA-FILE  FILE             : a multiple-alignment sequence file, support .gz or .bz2 compressed file\n"
		"Options:    -o FILE        : write output to FILE instead of stdout\n"
		"            --fmt  STR     : MSA format, supported format: 'fasta'\n"
		"            -qM INT[>=2]   : number of Dirichlet Mixture model components for match state emissions [" << DEFAULT_QM << "]\n"
		"            -symfrac       : conservation threshold for an MSA site to be considered as a Match state [" << DEFAULT_SYMFRAC << "]\n"
		"            --max-it INT   : maximum iteration allowed in gradient descent training, 0 for no limit [0]\n"
		"            --pri-rate DBL : adjust the sequence weights so the prior information is roughly this ratio in training [" << DEFAULT_PRI_RATE << "]\n"
		"            -s|--seed INT  : random seed used in Dirichlet Mixture model training (-qM > 1) for debug purpose\n"
		"            -n  INT        : number of different random seeds in Dirichlet Mixture model training, trained side by side [" << DEFAULT_NSEED << "]\n"
		"            --device  INT  : device index [0]\n"
		"            --chunk  INT   : iterations per kernel launch; changes no result [64]\n"
		"            -v  FLAG       : enable verbose information\n"
		"            --version      : show program version and exit\n"
		"            -h|--help      : print this help and exit\n";
}

static const char* why_nan(int32_t status) {
	return status == HU_DM_NAN_OVERFIT ? "Potential over-fitting detected. Please choose another MSA training set"
		: status == HU_DM_NAN_UNUSED ? "Potential unused (zero-coefficient) mixture component detected. Consider to use a smaller q, and a different random seed to run again"
		: "the training cost is not a finite number";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, fmt;
	int qM = DEFAULT_QM, maxIter = 0, nSeed = DEFAULT_NSEED, device = 0, verbose = 0, chunk = 0;
	double symfrac = DEFAULT_SYMFRAC, priRate = DEFAULT_PRI_RATE;
	unsigned seed = (unsigned) time(nullptr);     /* the time as default seed */
	if(argc == 1) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and training semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--fmt") fmt = val();
		else if(a == "-qM") qM = atoi(val());
		else if(a == "-symfrac") symfrac = atof(val());
		else if(a == "--max-it") maxIter = atoi(val());
		else if(a == "--pri-rate") priRate = atof(val());
		else if(a == "-s" || a == "--seed") seed = (unsigned) atoi(val());
		else if(a == "-n") nSeed = atoi(val());
		else if(a == "--device") device = atoi(val());
		else if(a == "--chunk") chunk = atoi(val());
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	const HuInfo info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	const std::string seqFn = pos[0];
	if(!(qM > 1 && qM <= MAX_NUM_COMPO)) { std::cerr << "-qM must between 2 and " << MAX_NUM_COMPO << std::endl; return EXIT_FAILURE; }
	if(!(symfrac >= 0 && symfrac <= 1)) { std::cerr << "-symfrac must between 0 and 1" << std::endl; return EXIT_FAILURE; }
	if(!(priRate > 0 && priRate <= 1)) { std::cerr << "--pri-rate must be in (0, 1]" << std::endl; return EXIT_FAILURE; }
	if(maxIter < 0) { std::cerr << "--max-it must be a non-negative integer" << std::endl; return EXIT_FAILURE; }
	if(nSeed < 1 || nSeed > MAX_NSEED) { std::cerr << "-n must be between 1 and " << MAX_NSEED << std::endl; return EXIT_FAILURE; }
	hu_dm_opts opts;
	hu_dm_default_opts(&opts);
	if(chunk == 0) chunk = opts.chunk;
	if(chunk < 1) { std::cerr << "--chunk must be a positive integer" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative" << std::endl; return EXIT_FAILURE; }
	opts.max_iter = maxIter; opts.chunk = chunk;
	/* guess input format (src/hmmufotu-train-dm.cpp:167-181) */
	if(fmt.empty() && ends_with(seqFn, ".msa")) fmt = "msa";
	hu_guess_seq_format(seqFn, fmt);
	if(fmt == "msa") { std::cerr << "MSA format 'msa': the reference's binary .msa database is not read here; pass the alignment as FASTA" << std::endl; return EXIT_FAILURE; }
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }

	LineIn seqIn;
	if(!seqIn.open(seqFn)) { std::cerr << "Unable to open seq file '" << seqFn << "' " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	HuBuildInputs inp;
	if(!hu_load_msa(seqIn, seqFn, seqFn, inp, info)) return EXIT_FAILURE;
	const size_t L0 = inp.L0, nSeq = inp.nSeq;
	{ /* the columns MSA::prune will keep are known from the text alone: too many of them are refused here, without a device */
		int8_t enc[256];
		hu_msa_encode_table(enc);
		std::vector<char> any(L0, 0);
		for(size_t i = 0; i < nSeq; ++i) { const char* row = inp.msa.data() + i * L0; for(size_t j = 0; j < L0; ++j) any[j] |= enc[(unsigned char) row[j]] >= 0; }
		const size_t kept = (size_t) std::count(any.begin(), any.end(), (char) 1);
		if(kept > MAX_CS) { std::cerr << "Unable to train the prior: the MSA has " << kept << " columns after pruning, the profile's index arrays end at " << MAX_CS << std::endl; return EXIT_FAILURE; }
		if(kept == 0) { std::cerr << "Unable to train the prior: the MSA has no column with a residue" << std::endl; return EXIT_FAILURE; }
	}

	/* the device: MSA::prune, then the five training sets */
	if(hu_device_count() <= device) { std::cerr << "Error: device " << device << " asked for, " << hu_device_count() << " gfx950 device(s) visible" << std::endl; return EXIT_FAILURE; }
	std::string err;
	if(!hu_prune_msa(device, inp, info, err)) { std::cerr << "Error: " << err << std::endl; return EXIT_FAILURE; }
	const size_t L = (size_t) inp.L;
	std::vector<char> text(nSeq * L);
	for(size_t i = 0; i < nSeq; ++i) { const char* src = inp.msa.data() + i * L0; char* dst = text.data() + i * L; for(size_t j = 0; j < L; ++j) dst[j] = src[inp.keep[j]]; }
	std::vector<char>().swap(inp.msa);
	std::vector<uint8_t> mask(L);
	std::vector<double> set[5] = {std::vector<double>(4 * L), std::vector<double>(4 * L), std::vector<double>(3 * L), std::vector<double>(2 * L), std::vector<double>(2 * L)};
	int64_t M[5];
	if(hu_dm_training_data(device, (int64_t) nSeq, (int64_t) L, text.data(), inp.weight.data(), priRate, symfrac, mask.data(),
			set[0].data(), set[1].data(), set[2].data(), set[3].data(), set[4].data(), M) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	info("MSA total weight scaled as: " + std::to_string(1 / priRate));
	info("Transition training data prepared: " + std::to_string(M[0]) + " match and " + std::to_string(M[1]) + " other columns; " + std::to_string(M[2]) + " M, " + std::to_string(M[3])
		+ " I and " + std::to_string(M[4]) + " D transition columns");
	if(M[0] == 0) { std::cerr << "Unable to train the prior: no column of " << L << " reaches the symbol fraction " << symfrac << std::endl; return EXIT_FAILURE; }

	/* where every model starts: momentInit.  A mixture's shuffle draws from rand(), seeded once; a set too small for a fit draws nothing */
	static const char* names[5] = {"Match Emission", "Insert Emission", "Match Transition", "Insert Transition", "Delete Transition"};
	static const int dims[5] = {4, 4, 3, 2, 2};
	srand(seed);
	info("Random seed: " + std::to_string(seed));
	const int nProb = nSeed + 4;
	std::vector<std::vector<double>> alpha0((size_t) nProb);
	std::vector<hu_dm_problem> prob((size_t) nProb);
	std::vector<int32_t> idx((size_t) M[0]);
	for(int s = 0; s < nSeed; ++s) {
		if(M[0] >= 2 * (int64_t) qM) hu_dm_shuffle(M[0], nullptr, idx.data());
		alpha0[(size_t) s].resize((size_t) 4 * qM);
		if(hu_dm_moment_init(4, qM, M[0], set[0].data(), idx.data(), alpha0[(size_t) s].data()) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
		prob[(size_t) s] = hu_dm_problem{4, qM, M[0], set[0].data(), alpha0[(size_t) s].data(), nullptr};
	}
	for(int b = 1; b < 5; ++b) {
		const size_t p = (size_t)(nSeed + b - 1);
		alpha0[p].resize((size_t) dims[b]);
		if(hu_dm_moment_init(dims[b], 1, M[b], set[b].data(), nullptr, alpha0[p].data()) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
		prob[p] = hu_dm_problem{dims[b], 1, M[b], set[b].data(), alpha0[p].data(), nullptr};
		if(M[b] == 0) std::cerr << "Warning: no training data for the " << names[b] << " model: alpha stays 1" << std::endl;
	}
	info("Dirichlet prior model initiated");
	info("Training Match Emission model with " + std::to_string(nSeed) + " seed(s) and the four density models");
	std::vector<hu_dm_result> res((size_t) nProb);
	hu_dm_progress progress = [](void* user, int64_t it, int32_t running) { if(*(int*) user) std::cerr << "  " << it << " iterations, " << running << " model(s) still training" << std::endl; };
	if(hu_dm_train(device, nProb, prob.data(), &opts, res.data(), progress, &verbose) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }

	/* the cheapest seed (src/hmmufotu-train-dm.cpp:344-358): a NaN is never cheaper */
	double costME = INFINITY; int best = -1;
	for(int s = 0; s < nSeed; ++s) {
		const double c = res[(size_t) s].cost;
		std::cerr << "  seed " << s + 1 << " trained, cost: " << c << std::endl;
		if(c < costME) { best = s; costME = c; }
	}
	if(best < 0) {
		std::cerr << "Unable to train Match Emission model: " << why_nan(res[0].status) << std::endl;
		return EXIT_FAILURE;
	}
	info("Best Match Emission model found at seed " + std::to_string(best + 1) + " after " + std::to_string(res[(size_t) best].iterations) + " iterations");
	hu_hmm_prior pri;
	memset(&pri, 0, sizeof(pri));
	double cost[5] = {costME, 0, 0, 0, 0};
	pri.me_L = qM;
	for(int j = 0; j < qM; ++j) { pri.me_q[j] = res[(size_t) best].q[j]; for(int i = 0; i < 4; ++i) pri.me_alpha[i][j] = res[(size_t) best].alpha[i][j]; }
	double* dst[5] = {nullptr, pri.ie_alpha, pri.mt_alpha, pri.it_alpha, pri.dt_alpha};
	for(int b = 1; b < 5; ++b) {
		const hu_dm_result& r = res[(size_t)(nSeed + b - 1)];
		/* the reference would print nan into the file; as hmmufotu-amd-train-sm does, a model that did not train is refused */
		if(!std::isfinite(r.cost)) { std::cerr << "Unable to train " << names[b] << " model: " << why_nan(r.status) << std::endl; return EXIT_FAILURE; }
		for(int i = 0; i < dims[b]; ++i) dst[b][i] = r.alpha[i][0];
		cost[b] = r.cost;
		info(std::string(names[b]) + " model trained after " + std::to_string(r.iterations) + " iterations");
	}
	if(hu_dm_write(outFn.empty() ? "-" : outFn.c_str(), &pri, cost) != HU_OK) { std::cerr << "Unable to write to " << (outFn.empty() ? "stdout" : outFn) << ": " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	return EXIT_SUCCESS;
}
