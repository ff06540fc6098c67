// hmmufotu-amd-train-sm: a DNA substitution model (.sm) trained on a reference MSA and its phylogenetic tree — hmmufotu-train-sm
// (src/hmmufotu-train-sm.cpp:77-243), whose output is the -sm FILE of hmmufotu-amd-build.  The host reads, joins and prunes the
// inputs exactly as the build program does (hu_build_inputs.h) and chooses the leaf rows to compare (hu_sm_training_set); the wide
// loops, the per-column counts over pairs and triples of rows and the base counts, run on the device (hu_sm_counts); the trainers
// are a few lines of 4 x 4 arithmetic on the host (hu_sm_train).  Options and inputs are checked, and the inputs read and joined,
// before a device is asked for.
//   hmmufotu-amd-train-sm <MSA-FILE> <TREE-FILE> [-o FILE] [--fmt fasta] [-s|--sub-model GTR|TN93|HKY85|F81|K80|JC69]
//                         [-m|--method Gojobori|Goldman] [--device N] [-v]
#include <algorithm>
#include <cstdlib>
#include "hu_build_inputs.h"

static void usage(const char* p) {
	std::cerr << "Train a DNA Substitution Model with customized data\n"
		"Usage:    " << p << "  <MSA-FILE> <TREE-FILE> [options]\n"
		"MSA-FILE  FILE                   : a multiple-alignment sequence file, support .gz or .bz2 compressed file\n"
		"TREE-FILE  FILE                  : phylogenetic-tree file build on the MSA sequences (.tree / .tre)\n"
		"Options:    -o FILE              : write output to FILE instead of stdout\n"
		"            --fmt  STR           : MSA format, supported format: 'fasta'\n"
		"            -s|--sub-model STR   : build a time-reversible DNA Substitution Model type, must be one of GTR, TN93, HKY85, F81, K80 or JC69 [GTR]\n"
		"            -m|--method  STR     : model training method using known phylogenetic tree data, either 'Gojobori' or 'Goldman' [Gojobori]\n"
		"            --device  INT        : device index [0]\n"
		"            -v  FLAG             : enable verbose information\n"
		"            --version            : show program version and exit\n"
		"            -h|--help            : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, fmt, smType = "GTR", method = "Gojobori";
	int device = 0, verbose = 0;
	if(argc == 1) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and training semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--fmt") fmt = val();
		else if(a == "-s" || a == "--sub-model") smType = val();
		else if(a == "-m" || a == "--method") method = val();
		else if(a == "--device") device = atoi(val());
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 2) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	const HuInfo info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	const std::string seqFn = pos[0], treeFn = pos[1];
	if(!hu_is_newick_name(treeFn)) { std::cerr << "Unrecognized TREE-FILE format, must be in Newick format" << std::endl; return EXIT_FAILURE; }
	/* guess input format (src/hmmufotu-train-sm.cpp:133-147) */
	if(fmt.empty() && ends_with(seqFn, ".msa")) fmt = "msa";
	hu_guess_seq_format(seqFn, fmt);
	if(fmt == "msa") { std::cerr << "MSA format 'msa': the reference's binary .msa database is not read here; pass the alignment as FASTA" << std::endl; return EXIT_FAILURE; }
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }
	/* DNASubModelFactory::createModel (src/DNASubModelFactory.cpp:38-53) and getModelTransitionSet (src/PhyloTreeUnrooted.h:1458-1466) */
	static const char* types[] = {"GTR", "TN93", "HKY85", "F81", "K80", "JC69"};
	int type = -1;
	for(int i = 0; i < 6; ++i) if(smType == types[i]) type = i;
	if(type < 0) { std::cerr << "Unknown DNA substitution model type '" << smType << "'" << std::endl; return EXIT_FAILURE; }
	std::string lowMethod = method;
	std::transform(lowMethod.begin(), lowMethod.end(), lowMethod.begin(), [](unsigned char c) { return (char) tolower(c); });
	if(lowMethod != "gojobori" && lowMethod != "goldman") { std::cerr << "Unknown DNA substitution model training method '" << method << "'" << std::endl; return EXIT_FAILURE; }
	const int how = lowMethod == "goldman" ? HU_SM_GOLDMAN : HU_SM_GOJOBORI;
	if(device < 0) { std::cerr << "--device must be non-negative" << std::endl; return EXIT_FAILURE; }

	/* open and read the inputs */
	LineIn seqIn;
	if(!seqIn.open(seqFn)) { std::cerr << "Unable to open MSA file '" << seqFn << "' " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	std::string treeText;
	if(!read_file(treeFn, treeText)) { std::cerr << "Unable to open '" << treeFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	HuBuildInputs inp;
	if(!hu_load_msa(seqIn, seqFn, seqFn, inp, info)) return EXIT_FAILURE;
	if(!hu_load_tree(treeText, treeFn, inp, info)) return EXIT_FAILURE;
	if(!hu_join_msa_tree(inp, info)) return EXIT_FAILURE;

	/* which rows are compared.  rand() is never seeded: the picks of randomLeaf are the reference's */
	std::vector<int32_t> items((size_t) inp.n * 3);
	int64_t nItems = 0;
	if(hu_sm_training_set(inp.n, inp.parent.data(), inp.childOff.data(), inp.childIdx.data(), inp.rowOf.data(), how, items.data(), &nItems) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }

	/* the device: MSA::prune, then the counts */
	if(hu_device_count() <= device) { std::cerr << "Error: device " << device << " asked for, " << hu_device_count() << " gfx950 device(s) visible" << std::endl; return EXIT_FAILURE; }
	std::string err;
	if(!hu_prune_msa(device, inp, info, err)) { std::cerr << "Error: " << err << std::endl; return EXIT_FAILURE; }
	if(inp.L < 1) { std::cerr << "Unable to train a model: the MSA has no column with a residue" << std::endl; return EXIT_FAILURE; }
	const size_t L = (size_t) inp.L;
	std::vector<int8_t> rows(inp.nSeq * L);
	{
		int8_t enc[256];
		hu_msa_encode_table(enc);
		for(size_t i = 0; i < inp.nSeq; ++i) hu_encode_row(inp, enc, i, rows.data() + i * L);
	}
	std::vector<char>().swap(inp.msa);
	std::vector<int32_t> counts((size_t) nItems * 16), dn((size_t) nItems * 4), pass((size_t) nItems), base(inp.nSeq * 4);
	if(hu_sm_counts(device, (int64_t) inp.nSeq, (int64_t) L, rows.data(), nItems, items.data(), counts.data(), dn.data(), base.data()) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	if(hu_sm_item_pass(nItems, items.data(), dn.data(), pass.data()) != HU_OK) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	/* getModelFreqEst: the base counts of every leaf's row */
	int64_t freq[4] = {0, 0, 0, 0};
	for(int32_t i = 0; i < inp.n; ++i) if(inp.rowOf[i] >= 0) for(int b = 0; b < 4; ++b) freq[b] += base[(size_t) inp.rowOf[i] * 4 + b];
	int64_t nPass = 0;
	for(int64_t i = 0; i < nItems; ++i) nPass += pass[i];
	info("Training set (" + std::string(how == HU_SM_GOLDMAN ? "Goldman" : "Gojobori") + "): " + std::to_string(nItems) + " candidates, " + std::to_string(nPass) + " within p-distance 0.15");

	std::vector<double> mats(counts.begin(), counts.end());
	hu_model_desc model;
	int64_t nUsed = 0;
	if(hu_sm_train(type, nItems, mats.data(), pass.data(), freq, &model, &nUsed) != HU_OK) { std::cerr << "Unable to train the model: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	info("Matrices kept: " + std::to_string(nUsed));
	info("DNA Substitution Model trained");

	/* output */
	const int64_t len = hu_sm_write_text(&model, nullptr, 0);
	if(len < 0) { std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	std::string text((size_t) len + 1, '\0');
	hu_sm_write_text(&model, &text[0], len + 1);
	text.resize((size_t) len);
	if(outFn.empty()) { std::cout << text; std::cout.flush(); if(!std::cout) { std::cerr << "Unable to write model: " << strerror(errno) << std::endl; return EXIT_FAILURE; } }
	else {
		std::ofstream of(outFn, std::ios::binary);
		if(!of.is_open()) { std::cerr << "Unable to write to '" << outFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		of << text; of.flush();
		if(!of) { std::cerr << "Unable to write model: " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	}
	info("Model written");
	return EXIT_SUCCESS;
}
