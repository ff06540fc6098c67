// hmmufotu-amd-tree: a neighbour-joining tree from a reference MSA, the TREE-FILE that hmmufotu-amd-train-sm and
// hmmufotu-amd-build start from.  The reference leaves this step to another package.  Plain neighbour joining on the pairwise
// distances of the rows, not a maximum-likelihood search: the usual starting tree of the ML packages.
//   hmmufotu-amd-tree <MSA-FILE> [-o TREE] [-sm FILE] [--dist pdist|JC69|K80|F81|HKY85|TN93] [--dist-out FILE] [--sat DBL] [--mem GB]
//                     [--device N] [--host] [-v]
//                     [--ml-lengths [--start-tree FILE] [--ml-rounds N] [--ml-eps DBL] [--min-len DBL] [--max-len DBL] [--ml-log FILE]
//                      [--nni [--nni-rounds N] [--nni-min-gain DBL] [--nni-log FILE]]
//                      [--spr [--spr-radius N] [--spr-rounds N] [--spr-min-gain DBL] [--spr-log FILE]]
//                      [--support N [--support-seed N] [--support-out FILE]]
//                      [--start-tree FILE --add [--add-log FILE]]
//                      [--gamma K [--gamma-alpha DBL] [--gamma-rounds N] [--gamma-eps DBL] [--gamma-log FILE]]]
// The MSA is read and pruned as hmmufotu-amd-build does (hu_build_inputs.h; the columns without a residue are found on the host here,
// the same columns hu_prune_msa finds), so the tree joins by name to the same MSA there.  The distances and the joins are
// hu_msa_tree's: on the device (hu_kern_dist.h, hu_kern_nj.h), or with --host by the library's host path.  Every refusal comes before
// a device is asked for, and the outputs are opened only after the computation: a refused run leaves no file.
// --ml-lengths keeps the topology, of the joins or of --start-tree, and fits its branch lengths by maximum likelihood
// under the fixed-rate model of -sm (hu_tree_optimize_lengths; a GTR file is used as GTR here).  The tree goes through hu_newick_parse
// either way, and hu_newick_write puts the same topology, names and order of children back with the new lengths.
// --nni lets the topology move: a hill climb over nearest-neighbour interchanges from that tree (hu_tree_nni_search),
// written by hu_newick_from_arrays with the same node ids, names and top node.
// --spr moves whole subtrees: a hill climb over subtree pruning and regrafting within a radius (hu_tree_spr_search).  With
// --nni the interchanges run first, then the SPR search, then the interchanges once more if a subtree was moved.
// --add keeps a tree current: the sequences of the MSA that are no leaf of --start-tree are inserted into it
// (hu_tree_add_search), and everything else runs on the grown tree.
// --support labels the inner edges of the final tree with their local bootstrap support (hu_tree_nni_support): the share
// of N resamplings of the columns in which the edge as it stands beats both of its nearest-neighbour interchanges.
// --gamma K is the last stage: on the tree everything above left, the lengths and the shape alpha are fitted under the
// discrete Gamma of K rates with mean 1 (hu_tree_gamma_fit).  Only the lengths change; the supports, computed before it, keep their place.
#include <cmath>
#include <cstdlib>
#include <memory>
#include "hu_build_inputs.h"

/* hu_build_inputs.h is shared with the programs that read a tree; the prune there asks for a device, the one here must not */
static const auto unused_tree [[maybe_unused]] = &hu_load_tree;
static const auto unused_join [[maybe_unused]] = &hu_join_msa_tree;
static const auto unused_newick [[maybe_unused]] = &hu_is_newick_name;
static const auto unused_prune [[maybe_unused]] = &hu_prune_msa;

static void usage(const char* p) {
	std::cerr << "Build a neighbour-joining tree (Newick, unrooted) from a multiple sequence alignment\n"
		"Usage:    " << p << "  <MSA-FILE> [options]\n"
		"MSA-FILE  FILE                 : a multiple-alignment sequence file, support .gz or .bz2 compressed file\n"
		"Options:    -o  FILE           : tree output [stdout]\n"
		"            --fmt  STR         : MSA format, supported format: 'fasta'\n"
		"            -sm  FILE          : DNA substitution model file (hmmufotu-amd-train-sm): its type is the default of --dist, its base frequencies go into F81, HKY85 and TN93; a GTR file gives TN93\n"
		"            --dist  STR        : pdist, JC69, K80, F81, HKY85 or TN93 [the type of -sm, or JC69]\n"
		"            --dist-out  FILE   : also write the distance matrix: a line n, then per row its name and n values\n"
		"            --sat  DBL         : distance of a saturated pair (its formula takes the logarithm of a value <= 0) [twice the largest finite distance]\n"
		"            --mem  DBL         : device memory to use at the most, in GB [what the device reports free]\n"
		"            --device  INT      : device to run on [0]\n"
		"            --host  FLAG       : run on the host, no device needed\n"
		"            --ml-lengths  FLAG : keep the topology and fit the branch lengths by maximum likelihood under the fixed-rate model of -sm (required then; a GTR file is used as GTR)\n"
		"            --start-tree  FILE : with --ml-lengths: fit the lengths of this Newick tree, no distances are computed; its leaves are the sequences of the MSA, by name\n"
		"            --ml-rounds  INT   : rounds of simultaneous branch steps at the most [50]\n"
		"            --ml-eps  DBL      : converged when every branch is within this of its own optimum, at least 1e-6 [1e-5]\n"
		"            --min-len  DBL     : smallest branch length [0]\n"
		"            --max-len  DBL     : largest branch length [10]\n"
		"            --ml-log  FILE     : write the rounds as TSV: round, ll, s, delta, capped; a last line '# stop: REASON'\n"
		"            --nni  FLAG        : with --ml-lengths: improve the topology by nearest-neighbour interchanges, a hill climb on the log-likelihood\n"
		"            --nni-rounds  INT  : rounds of interchanges at the most, at least 1 [20]\n"
		"            --nni-min-gain  DBL: smallest gain in log-likelihood for which an interchange is tried, above 0 [1e-3]\n"
		"            --nni-log  FILE    : write the accepted rounds as TSV: round, ll, scored, candidates, taken, applied; then '# stop: REASON' and '# skipped: N edges at polytomies'\n"
		"            --spr  FLAG        : with --ml-lengths: improve the topology by subtree pruning and regrafting, a hill climb on the log-likelihood; with --nni the interchanges run before it and, if a subtree was moved, once more after it\n"
		"            --spr-radius  INT  : a pruned subtree is tried in the edges up to this many nodes away, 1 to 32 [5]\n"
		"            --spr-rounds  INT  : rounds of moves at the most, at least 1 [10]\n"
		"            --spr-min-gain  DBL: smallest gain in log-likelihood for which a move is tried, above 0 [1e-3]\n"
		"            --spr-log  FILE    : write the accepted rounds as TSV: round, ll, pruned, targets, candidates, taken, applied; then '# stop: REASON' and '# skipped: N nodes'\n"
		"            --add  FLAG        : with --ml-lengths --start-tree: the sequences of the MSA that are no leaf of the start tree are inserted into it, each into the edge where the tree's likelihood is largest with its pendant at its optimum; a round takes one sequence per edge, the others are scored again against the grown tree\n"
		"            --add-log  FILE    : write the rounds as TSV: round, ll, scored, inserted; then per sequence '# insert: round name node edge t f' and '# stop: all inserted'\n"
		"            --support  INT     : with --ml-lengths: label every inner edge between two nodes of degree three with its local bootstrap support over INT replicates, 1 to 100000: the share of resampled alignments in which the edge beats both of its nearest-neighbour interchanges\n"
		"            --support-seed  INT: seed of the replicates [1]\n"
		"            --support-out  FILE: write the supports as TSV: node, name, kind, leaves, t0, alrt, count, replicates, support; then '# skipped: N edges at polytomies' and '# seed: S'\n"
		"            --gamma  INT       : with --ml-lengths, as the last stage: fit the branch lengths and the shape alpha under the discrete Gamma of INT rate categories with mean rate 1, 2 to 16; everything before it, the supports included, runs under the fixed-rate model\n"
		"            --gamma-alpha  DBL : keep the shape at this value, 0.05 to 100 [estimated by maximum likelihood]\n"
		"            --gamma-rounds  INT: passes of 'shape, then lengths' at the most, at least 1 [10]\n"
		"            --gamma-eps  DBL   : stop when a pass gains less than this in log-likelihood, above 0 [0.01]\n"
		"            --gamma-log  FILE  : write the passes as TSV: pass, alpha, ll, rounds; then '# rates: R1 ... RK' and '# stop: REASON'\n"
		"            -v  FLAG           : enable verbose information, you may set multiple -v for more details\n"
		"            --version          : show program version and exit\n"
		"            -h|--help          : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, fmt, smFn, distName, distFn; bool host = false, haveSat = false; int device = 0, verbose = 0;
	double sat = 0, memGB = 0; bool haveMem = false;
	bool mlLengths = false; std::string startFn, mlLogFn; int mlRounds = 50; double mlEps = 1e-5, minLen = 0.0, maxLen = 10.0;
	bool nni = false, haveNniOpt = false; std::string nniLogFn; int nniRounds = 20; double nniMinGain = 1e-3;
	bool spr = false, haveSprOpt = false; std::string sprLogFn; int sprRadius = 5, sprRounds = 10; double sprMinGain = 1e-3;
	bool add = false; std::string addLogFn;
	bool support = false, haveSupportOpt = false; long long supportN = 0; unsigned long long supportSeed = 1; std::string supportFn;
	bool gamma = false, haveGammaOpt = false, haveGammaAlpha = false; int gammaK = 0, gammaRounds = 10; double gammaAlpha = 0, gammaEps = 0.01; std::string gammaLogFn;
	if(argc < 2) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--fmt") fmt = val(); else if(a == "-sm") smFn = val(); else if(a == "--dist") distName = val();
		else if(a == "--dist-out") distFn = val();
		else if(a == "--sat") { sat = atof(val()); haveSat = true; }
		else if(a == "--mem") { memGB = atof(val()); haveMem = true; }
		else if(a == "--device") device = atoi(val()); else if(a == "--host") host = true;
		else if(a == "--ml-lengths") mlLengths = true; else if(a == "--start-tree") startFn = val(); else if(a == "--ml-log") mlLogFn = val();
		else if(a == "--ml-rounds") mlRounds = atoi(val()); else if(a == "--ml-eps") mlEps = atof(val());
		else if(a == "--min-len") minLen = atof(val()); else if(a == "--max-len") maxLen = atof(val());
		else if(a == "--nni") nni = true;
		else if(a == "--nni-rounds") { nniRounds = atoi(val()); haveNniOpt = true; } else if(a == "--nni-min-gain") { nniMinGain = atof(val()); haveNniOpt = true; }
		else if(a == "--nni-log") { nniLogFn = val(); haveNniOpt = true; }
		else if(a == "--spr") spr = true;
		else if(a == "--spr-radius") { sprRadius = atoi(val()); haveSprOpt = true; } else if(a == "--spr-rounds") { sprRounds = atoi(val()); haveSprOpt = true; }
		else if(a == "--spr-min-gain") { sprMinGain = atof(val()); haveSprOpt = true; } else if(a == "--spr-log") { sprLogFn = val(); haveSprOpt = true; }
		else if(a == "--add") add = true; else if(a == "--add-log") addLogFn = val();
		else if(a == "--support") { supportN = atoll(val()); support = true; }
		else if(a == "--support-seed") { supportSeed = strtoull(val(), nullptr, 10); haveSupportOpt = true; }
		else if(a == "--support-out") { supportFn = val(); haveSupportOpt = true; }
		else if(a == "--gamma") { gammaK = atoi(val()); gamma = true; }
		else if(a == "--gamma-alpha") { gammaAlpha = atof(val()); haveGammaOpt = haveGammaAlpha = true; }
		else if(a == "--gamma-rounds") { gammaRounds = atoi(val()); haveGammaOpt = true; } else if(a == "--gamma-eps") { gammaEps = atof(val()); haveGammaOpt = true; }
		else if(a == "--gamma-log") { gammaLogFn = val(); haveGammaOpt = true; }
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	const HuInfo info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	const std::string seqFn = pos[0];
	if(fmt.empty() && ends_with(seqFn, ".msa")) fmt = "msa";
	hu_guess_seq_format(seqFn, fmt);
	if(fmt == "msa") { std::cerr << "MSA format 'msa': the reference's binary .msa database is not read here; pass the alignment as FASTA" << std::endl; return EXIT_FAILURE; }
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }
	if(haveSat && (!(sat > 0) || !std::isfinite(sat))) { std::cerr << "--sat must be positive" << std::endl; return EXIT_FAILURE; }
	if(haveMem && (!(memGB > 0) || !std::isfinite(memGB))) { std::cerr << "--mem must be positive" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative; --host runs without one" << std::endl; return EXIT_FAILURE; }
	if(!mlLengths && (!startFn.empty() || !mlLogFn.empty())) { std::cerr << (startFn.empty() ? "--ml-log" : "--start-tree") << " goes with --ml-lengths" << std::endl; return EXIT_FAILURE; }
	if(add && startFn.empty()) { std::cerr << "--add goes with --ml-lengths --start-tree: the new sequences are inserted into a start tree" << std::endl; return EXIT_FAILURE; }
	if(!addLogFn.empty() && !add) { std::cerr << "--add-log goes with --add" << std::endl; return EXIT_FAILURE; }
	if(nni && !mlLengths) { std::cerr << "--nni goes with --ml-lengths" << std::endl; return EXIT_FAILURE; }
	if(haveNniOpt && !nni) { std::cerr << "--nni-rounds, --nni-min-gain and --nni-log go with --nni" << std::endl; return EXIT_FAILURE; }
	if(spr && !mlLengths) { std::cerr << "--spr goes with --ml-lengths" << std::endl; return EXIT_FAILURE; }
	if(haveSprOpt && !spr) { std::cerr << "--spr-radius, --spr-rounds, --spr-min-gain and --spr-log go with --spr" << std::endl; return EXIT_FAILURE; }
	if(spr) {
		if(sprRadius < 1 || sprRadius > HU_SPR_MAX_RADIUS) { std::cerr << "--spr-radius must be 1 to " << HU_SPR_MAX_RADIUS << std::endl; return EXIT_FAILURE; }
		if(sprRounds < 1) { std::cerr << "--spr-rounds must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(!(sprMinGain > 0) || !std::isfinite(sprMinGain)) { std::cerr << "--spr-min-gain must be above 0" << std::endl; return EXIT_FAILURE; }
	}
	if(support && !mlLengths) { std::cerr << "--support goes with --ml-lengths" << std::endl; return EXIT_FAILURE; }
	if(haveSupportOpt && !support) { std::cerr << "--support-seed and --support-out go with --support" << std::endl; return EXIT_FAILURE; }
	if(support && (supportN < 1 || supportN > HU_SUPPORT_MAX_REPLICATES)) { std::cerr << "--support must be 1 to " << HU_SUPPORT_MAX_REPLICATES << " replicates" << std::endl; return EXIT_FAILURE; }
	if(gamma && !mlLengths) { std::cerr << "--gamma goes with --ml-lengths" << std::endl; return EXIT_FAILURE; }
	if(haveGammaOpt && !gamma) { std::cerr << "--gamma-alpha, --gamma-rounds, --gamma-eps and --gamma-log go with --gamma" << std::endl; return EXIT_FAILURE; }
	if(gamma) {
		if(gammaK < 2 || gammaK > 16) { std::cerr << "--gamma must be 2 to 16 rate categories" << std::endl; return EXIT_FAILURE; }
		if(haveGammaAlpha && (!(gammaAlpha >= HU_GAMMA_ALPHA_MIN) || !(gammaAlpha <= HU_GAMMA_ALPHA_MAX))) { std::cerr << "--gamma-alpha must be " << HU_GAMMA_ALPHA_MIN << " to " << HU_GAMMA_ALPHA_MAX << std::endl; return EXIT_FAILURE; }
		if(gammaRounds < 1) { std::cerr << "--gamma-rounds must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(!(gammaEps > 0) || !std::isfinite(gammaEps)) { std::cerr << "--gamma-eps must be above 0" << std::endl; return EXIT_FAILURE; }
	}
	if(nni) {
		if(nniRounds < 1) { std::cerr << "--nni-rounds must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(!(nniMinGain > 0) || !std::isfinite(nniMinGain)) { std::cerr << "--nni-min-gain must be above 0" << std::endl; return EXIT_FAILURE; }
	}
	if(mlLengths) {
		if(smFn.empty()) { std::cerr << "--ml-lengths fits the branch lengths under a substitution model: -sm is required" << std::endl; return EXIT_FAILURE; }
		if(!(mlEps > 0) || !std::isfinite(mlEps)) { std::cerr << "--ml-eps must be positive" << std::endl; return EXIT_FAILURE; }
		if(mlEps < 100 * HU_BLEN_TAU) { std::cerr << "--ml-eps must be at least " << 100 * HU_BLEN_TAU << ": 100 times the tolerance of a branch's own step" << std::endl; return EXIT_FAILURE; }
		if(!(maxLen > 0) || !std::isfinite(maxLen)) { std::cerr << "--max-len must be positive" << std::endl; return EXIT_FAILURE; }
		if(!(minLen >= 0)) { std::cerr << "--min-len must not be negative" << std::endl; return EXIT_FAILURE; }
		if(!(minLen < maxLen)) { std::cerr << "--min-len must be below --max-len" << std::endl; return EXIT_FAILURE; }
		if(mlRounds < 1) { std::cerr << "--ml-rounds must be at least 1" << std::endl; return EXIT_FAILURE; }
		if(!startFn.empty() && !distFn.empty()) { std::cerr << "--dist-out: with --start-tree no distances are computed" << std::endl; return EXIT_FAILURE; }
	}
	static const char* const names[] = {"pdist", "JC69", "K80", "F81", "HKY85", "TN93"};
	int type = -1;
	if(!distName.empty()) {
		for(int m = 0; m < 6; ++m) if(distName == names[m]) type = m;
		if(type < 0) { std::cerr << "Unsupported distance '" << distName << "': pdist, JC69, K80, F81, HKY85 or TN93 (GTR distances are not offered)" << std::endl; return EXIT_FAILURE; }
		if(type >= HU_DIST_F81 && smFn.empty()) { std::cerr << "--dist " << distName << " reads the base frequencies of a model: -sm is required" << std::endl; return EXIT_FAILURE; }
	}
	/* the model: its type is the default distance, its pi the base frequencies */
	double pi[4] = {0.25, 0.25, 0.25, 0.25};
	hu_model_desc md;
	memset(&md, 0, sizeof(md));
	if(!smFn.empty()) {
		std::string text;
		if(!read_file(smFn, text)) { std::cerr << "Unable to open '" << smFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		/* the type is the word behind "Type:", as hmmufotu-amd-build reads the file (src/hmmufotu-build.cpp:393-405) */
		std::istringstream in(text);
		std::string tag, mtype, line;
		while(in >> tag) { if(tag[0] == '#') { std::getline(in, line); continue; } if(tag == "Type:") { in >> mtype; break; } }
		const std::string withType = mtype + "\n" + text;
		if(mtype.empty()) { std::cerr << "Unable to load DNA Substitution Model '" << smFn << "': no Type: line" << std::endl; return EXIT_FAILURE; }
		if(hu_model_parse_text(withType.data(), (int64_t) withType.size(), &md) != HU_OK) { std::cerr << "Unable to load DNA Substitution Model '" << smFn << "': " << hu_last_error() << std::endl; return EXIT_FAILURE; }
		/* hu_model_desc.type: GTR TN93 HKY85 F81 K80 JC69 in the order of hmmufotu-amd-train-sm */
		static const int ofModel[6] = {HU_DIST_TN93, HU_DIST_TN93, HU_DIST_HKY85, HU_DIST_F81, HU_DIST_K80, HU_DIST_JC69};
		if(md.type < 0 || md.type > 5) { std::cerr << "Unknown model type in '" << smFn << "'" << std::endl; return EXIT_FAILURE; }
		md.dg_k = 0;                                                       /* the fixed-rate model, as hmmufotu-amd-train-sm trained it */
		if(type < 0) {
			type = ofModel[md.type];
			if(md.type == 0) info("The model is GTR, whose distance is not offered: TN93 with the model's base frequencies is used");
		}
		for(int b = 0; b < 4; ++b) pi[b] = md.pi[b];
		if(type >= HU_DIST_F81) for(int b = 0; b < 4; ++b) if(!(pi[b] > 0)) { std::cerr << "The model of '" << smFn << "' has a base frequency that is not positive" << std::endl; return EXIT_FAILURE; }
	}
	if(type < 0) type = HU_DIST_JC69;
	info(std::string("Distance: ") + names[type]);

	LineIn seqIn;
	if(!seqIn.open(seqFn)) { std::cerr << "Unable to open MSA file '" << seqFn << "' " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	HuBuildInputs inp;
	if(!hu_load_msa(seqIn, seqFn, seqFn, inp, info)) return EXIT_FAILURE;
	if(inp.nSeq < 3) { std::cerr << "A tree needs at least 3 sequences, '" << seqFn << "' has " << inp.nSeq << std::endl; return EXIT_FAILURE; }
	/* MSA::prune: the columns without a residue go */
	int8_t enc[256];
	hu_msa_encode_table(enc);
	{
		std::vector<char> any(inp.L0, 0);
		for(size_t i = 0; i < inp.nSeq; ++i) { const char* src = inp.msa.data() + i * inp.L0; for(size_t j = 0; j < inp.L0; ++j) if(enc[(unsigned char) src[j]] >= 0) any[j] = 1; }
		for(size_t j = 0; j < inp.L0; ++j) if(any[j]) inp.keep.push_back((uint32_t) j);
		inp.L = (int32_t) inp.keep.size();
		info("MSA pruned: " + std::to_string(inp.nSeq) + " X " + std::to_string(inp.L) + " aligned sequences");
	}
	if(inp.L < 1) { std::cerr << "Unable to build a tree: the MSA has no column with a residue" << std::endl; return EXIT_FAILURE; }
	if(inp.L > 65535) { std::cerr << "The pruned MSA has " << inp.L << " columns: 65535 at the most are taken" << std::endl; return EXIT_FAILURE; }
	const size_t n = inp.nSeq, L = (size_t) inp.L;
	std::vector<int8_t> rows(n * L);
	for(size_t i = 0; i < n; ++i) hu_encode_row(inp, enc, i, rows.data() + i * L);
	std::vector<char>().swap(inp.msa);
	for(size_t i = 0; i < n; ++i) {
		const std::string& s = inp.rowName[i];
		for(unsigned char c : s) if(c == '\'' || c < 0x20 || c == 0x7f) { std::cerr << "Sequence name '" << s << "' holds a quote or a byte that does not print: no Newick label" << std::endl; return EXIT_FAILURE; }
	}

	/* the tree of the fit: one parse, of --start-tree here or of the joins' text below, whose handle also writes the result.
	 * --start-tree is read and joined to the MSA by name before anything is computed */
	std::string text;
	std::unique_ptr<hu_newick, void (*)(hu_newick*)> nw(nullptr, hu_newick_free);
	std::vector<int32_t> parent, childOff, childIdx; std::vector<double> blen;
	int32_t nn = 0;
	std::vector<std::string> nodeNames;                       /* of the parsed tree, and of the leaves --add appends */
	std::vector<size_t> queryRow;                             /* --add: the rows of the MSA that are no leaf of --start-tree, ascending */
	auto parse_tree = [&](const std::string& from) {
		hu_newick* t = nullptr;
		if(hu_newick_parse(text.data(), (int64_t) text.size(), &t) != HU_OK) { std::cerr << "Unable to read Newick tree in '" << from << "': " << hu_last_error() << std::endl; return false; }
		nw.reset(t);
		hu_newick_size(t, &nn);
		parent.resize(nn); childOff.resize((size_t) nn + 1); childIdx.resize((size_t) std::max(nn - 1, 1)); blen.resize(nn);
		hu_newick_get(t, parent.data(), blen.data(), childOff.data(), childIdx.data());
		nodeNames.resize((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) nodeNames[i] = hu_newick_name(t, i);
		return true;
	};
	int64_t fitNodes = 2 * (int64_t) n - 2;                    /* the joins' tree: n leaves, n - 3 joins, the top node */
	if(!startFn.empty()) {
		if(!read_file(startFn, text)) { std::cerr << "Unable to open '" << startFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		if(!parse_tree(startFn)) return EXIT_FAILURE;
		info("Newick Tree read: " + std::to_string(nn) + " nodes");
		std::unordered_map<std::string, int32_t> seen;
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) {
			const std::string leaf = nodeNames[i].c_str();
			if(!seen.insert({leaf, i}).second) { std::cerr << "Non-unique leaf name '" << leaf << "' found in the tree '" << startFn << "'" << std::endl; return EXIT_FAILURE; }
			if(!inp.name2row.count(leaf)) { std::cerr << "Unmatched MSA and Tree: leaf '" << leaf << "' of '" << startFn << "' is no sequence of the MSA" << std::endl; return EXIT_FAILURE; }
		}
		for(size_t i = 0; i < n; ++i) if(!seen.count(inp.rowName[i])) { if(add) { queryRow.push_back(i); continue; } std::cerr << "Unmatched MSA and Tree: sequence '" << inp.rowName[i] << "' is no leaf of '" << startFn << "'" << std::endl; return EXIT_FAILURE; }
		if(nn < 2) { std::cerr << "The tree '" << startFn << "' has one node: no branch to fit" << std::endl; return EXIT_FAILURE; }
		fitNodes = (int64_t) nn + 2 * (int64_t) queryRow.size();
		if(fitNodes > INT32_MAX) { std::cerr << "--add: " << queryRow.size() << " new sequences give a tree of too many nodes" << std::endl; return EXIT_FAILURE; }
	}
	if(mlLengths && haveMem) {
		const int64_t need = support ? hu_support_need((int32_t) fitNodes, (int32_t) L, (int32_t) supportN) : nni ? hu_nni_need((int32_t) fitNodes, (int32_t) L) : hu_blen_need((int32_t) fitNodes, (int32_t) L), have = (int64_t)(memGB * 1e9);
		const int64_t addNeed = queryRow.empty() ? 0 : hu_add_need((int32_t) fitNodes, (int32_t) L, (int32_t) queryRow.size());
		if(addNeed > have) { std::cerr << "--add: " << fitNodes << " nodes of " << L << " columns after " << queryRow.size() << " insertions need " << addNeed << " bytes (64 bytes per node and column for the messages), --mem allows " << have << " bytes" << std::endl; return EXIT_FAILURE; }
		const int64_t sprNeed = spr ? hu_spr_need((int32_t) fitNodes, (int32_t) L, sprRadius) : 0;
		if(sprNeed > have && sprNeed >= need) { std::cerr << "--spr: " << fitNodes << " nodes of " << L << " columns at radius " << sprRadius << " need " << sprNeed << " bytes (64 bytes per node and column for the messages), --mem allows " << have << " bytes" << std::endl; return EXIT_FAILURE; }
		const int64_t gammaNeed = gamma ? hu_gamma_need((int32_t) fitNodes, (int32_t) L, gammaK) : 0;
		if(gammaNeed > have && gammaNeed >= need) { std::cerr << "--gamma: " << fitNodes << " nodes of " << L << " columns in " << gammaK << " rate categories need " << gammaNeed << " bytes (64 bytes per node, column and category for the messages), --mem allows " << have << " bytes" << std::endl; return EXIT_FAILURE; }
		if(need > have) { std::cerr << (support ? "--support: " : nni ? "--nni: " : "--ml-lengths: ") << fitNodes << " nodes of " << L << " columns need " << need << " bytes (64 bytes per node and column for the messages), --mem allows " << have << " bytes" << std::endl; return EXIT_FAILURE; }
	}

	hu_nj_opts o;
	hu_nj_default_opts(&o);
	o.host = host ? 1 : 0;
	if(haveMem) o.mem_budget = (int64_t)(memGB * 1e9);
	if(!host && hu_device_count() <= device) { std::cerr << "Error: device " << device << " asked for, " << hu_device_count() << " gfx950 device(s) visible; --host runs without one" << std::endl; return EXIT_FAILURE; }
	std::vector<const char*> nm(n);
	for(size_t i = 0; i < n; ++i) nm[i] = inp.rowName[i].c_str();
	std::vector<double> D;
	if(startFn.empty()) {
		if(!distFn.empty()) D.resize(n * n);
		std::vector<int32_t> join(2 * (n - 3) + 1); std::vector<double> len(2 * (n - 3) + 1);
		int32_t last3[3]; double lastLen3[3]; int64_t nSat = 0;
		if(hu_msa_tree(host ? -1 : device, (int64_t) n, (int64_t) L, rows.data(), type, pi, sat, &o, distFn.empty() ? nullptr : D.data(), &nSat, join.data(), len.data(), last3, lastLen3) != HU_OK) {
			std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		if(nSat > 0) std::cerr << "Warning: " << nSat << " pair(s) of sequences are saturated under " << names[type] << ": given "
			<< (haveSat ? "the distance of --sat" : "twice the largest finite distance") << std::endl;
		if(verbose && !host) {
			double s[4];
			hu_nj_timing(s);
			std::cerr << "copies up and encoding " << s[0] << " s, distances " << s[1] << " s, joins " << s[2] << " s, copies back " << s[3] << " s" << std::endl;
		}
		const int64_t tl = hu_nj_newick((int64_t) n, nm.data(), join.data(), len.data(), last3, lastLen3, nullptr, 0);
		if(tl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) tl + 1, '\0');
		hu_nj_newick((int64_t) n, nm.data(), join.data(), len.data(), last3, lastLen3, &text[0], tl + 1);
		text.resize((size_t) tl);
		if(mlLengths && !parse_tree("the joins")) return EXIT_FAILURE;
	}
	/* --add: the sequences that are no leaf of --start-tree are inserted first; the arrays grow by two nodes per sequence, and whatever
	 * follows (the fit, --nni, --spr, --support) runs on the grown tree.  Without such a sequence the run is the run without the flag */
	bool grown = false;
	if(add && (!queryRow.empty() || !addLogFn.empty())) {
		const size_t q = queryRow.size(), N = (size_t) nn + 2 * q;
		std::vector<int8_t> seq(N * L, (int8_t) -2), qrows(std::max<size_t>(q, 1) * L);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		for(size_t k = 0; k < q; ++k) memcpy(qrows.data() + k * L, rows.data() + queryRow[k] * L, L);
		std::vector<int32_t> par(parent), off(childOff), idx(childIdx), qnode(std::max<size_t>(q, 1), -1);
		std::vector<double> bl(blen);
		par.resize(N, -1); bl.resize(N, 0.0); off.resize(N + 1, 0); idx.resize(std::max<size_t>(N - 1, 1), 0);
		for(int32_t i = 0; i < nn; ++i) if(par[i] >= 0 && std::isfinite(bl[i])) bl[i] = std::min(std::max(bl[i], minLen), maxLen);
		hu_add_opts ao;
		hu_add_default_opts(&ao);
		std::vector<hu_add_round> arounds(std::max<size_t>(q, 1));
		std::vector<hu_add_insert> ains(std::max<size_t>(q, 1));
		ao.blen.eps = mlEps; ao.blen.min_len = minLen; ao.blen.max_len = maxLen; ao.blen.max_rounds = mlRounds; ao.blen.host = host ? 1 : 0; ao.blen.device = device;
		ao.blen.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0;
		ao.rounds = arounds.data(); ao.rounds_cap = (int32_t) arounds.size(); ao.inserts = ains.data(); ao.inserts_cap = (int64_t) ains.size();
		if(hu_tree_add_search(&ao, nn, (int32_t) L, (int32_t) q, par.data(), bl.data(), seq.data(), off.data(), idx.data(), qrows.data(), qnode.data(), &md) != HU_OK) {
			std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		if(verbose) {
			char line[240];
			snprintf(line, sizeof(line), "Sequences inserted: %d in %d round(s), log-likelihood %.17g of the start tree, %.17g of the grown tree of %zu nodes", ao.n_inserted, ao.n_rounds, ao.ll_start, ao.ll_final, N);
			std::cerr << line << std::endl;
			for(int32_t r = 0; r < ao.n_rounds; ++r) {
				snprintf(line, sizeof(line), "round %d: %d scored, %d inserted, log-likelihood %.17g", r + 1, arounds[r].scored, arounds[r].inserted, arounds[r].ll);
				std::cerr << line << std::endl;
			}
			double s[4];
			hu_add_timing(s);
			std::cerr << "insertion sweeps " << s[0] << " s, scoring " << s[1] << " s, fits " << s[2] << " s, the rest " << s[3] << " s" << std::endl;
		}
		if(!addLogFn.empty()) {
			FILE* f = fopen(addLogFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << addLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
			fprintf(f, "round\tll\tscored\tinserted\n0\t%.17g\t0\t0\n", ao.ll_start);
			for(int32_t r = 0; r < ao.n_rounds; ++r) fprintf(f, "%d\t%.17g\t%d\t%d\n", r + 1, arounds[r].ll, arounds[r].scored, arounds[r].inserted);
			for(int32_t k = 0; k < ao.n_inserted; ++k) fprintf(f, "# insert: %d\t%s\t%d\t%d\t%.17g\t%.17g\n", ains[k].round, inp.rowName[queryRow[(size_t) ains[k].query]].c_str(), ains[k].v, ains[k].w, ains[k].t, ains[k].f);
			fprintf(f, "# stop: all inserted\n");
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << addLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		}
		if(q > 0) {
			parent.swap(par); blen.swap(bl); childOff.swap(off); childIdx.swap(idx);
			nodeNames.resize(N);
			for(size_t k = 0; k < q; ++k) nodeNames[(size_t) qnode[k]] = inp.rowName[queryRow[k]];
			nn = (int32_t) N;
			grown = true;
		}
	}
	/* --ml-lengths: the parsed tree's arrays go into the fit, and its handle writes them back */
	hu_blen_opts bo;
	hu_blen_default_opts(&bo);
	std::vector<hu_blen_round> rounds;
	/* --spr: the search on the arrays in place, its report and its log; the moves applied, or -1 after an error */
	auto run_spr = [&](const std::vector<int8_t>& seq) -> long long {
		hu_spr_opts so;
		hu_spr_default_opts(&so);
		std::vector<hu_spr_round> srounds((size_t) sprRounds);
		std::vector<int32_t> moves((size_t) sprRounds * (size_t) nn * 5);
		so.blen.eps = mlEps; so.blen.min_len = minLen; so.blen.max_len = maxLen; so.blen.max_rounds = mlRounds; so.blen.host = host ? 1 : 0; so.blen.device = device;
		so.blen.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0;
		so.radius = sprRadius; so.spr_rounds = sprRounds; so.min_gain = sprMinGain; so.rounds = srounds.data(); so.rounds_cap = sprRounds;
		so.moves = moves.data(); so.moves_cap = (int64_t) sprRounds * nn;
		if(hu_tree_spr_search(&so, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), childOff.data(), childIdx.data(), &md) != HU_OK) { std::cerr << hu_last_error() << std::endl; return -1; }
		static const char* const why[] = {"local optimum", "no improving move", "max rounds"};
		if(verbose) {
			char line[240];
			snprintf(line, sizeof(line), "SPR search: log-likelihood %.17g -> %.17g, %lld move(s) applied in %d round(s) at radius %d, stop: %s", so.ll_start, so.ll_final, (long long) so.n_moves, so.n_rounds, sprRadius, why[so.stop]);
			std::cerr << line << std::endl;
			for(int64_t k = 0; k < so.n_moves && k < so.moves_cap; ++k) {
				const int32_t* mv = moves.data() + k * 5;
				snprintf(line, sizeof(line), "round %d: the subtree of node %d from the edge of node %d into the edge of node %d, distance %d", mv[0], mv[1], mv[2], mv[3], mv[4]);
				std::cerr << line << std::endl;
			}
			if(so.skipped > 0) std::cerr << so.skipped << " node(s) were not pruned: their parent is the top node or a polytomy" << std::endl;
			double s[4];
			hu_spr_timing(s);
			std::cerr << "SPR fits " << s[0] << " s, scoring " << s[1] << " s, trials " << s[2] << " s, the rest " << s[3] << " s" << std::endl;
		}
		if(!sprLogFn.empty()) {
			FILE* f = fopen(sprLogFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << sprLogFn << "': " << strerror(errno) << std::endl; return -1; }
			fprintf(f, "round\tll\tpruned\ttargets\tcandidates\ttaken\tapplied\n0\t%.17g\t0\t0\t0\t0\t0\n", so.ll_start);
			for(int32_t r = 0; r < so.n_rounds; ++r) fprintf(f, "%d\t%.17g\t%d\t%lld\t%d\t%d\t%d\n", r + 1, srounds[r].ll, srounds[r].pruned, (long long) srounds[r].targets, srounds[r].candidates, srounds[r].taken, srounds[r].applied);
			fprintf(f, "# stop: %s\n# skipped: %lld nodes\n", why[so.stop], (long long) so.skipped);
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << sprLogFn << "': " << strerror(errno) << std::endl; return -1; }
		}
		return (long long) so.n_moves;
	};
	if(mlLengths && nni) {
		std::vector<int8_t> seq((size_t) nn * L, (int8_t) -2);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		for(int32_t i = 0; i < nn; ++i) if(parent[i] >= 0 && std::isfinite(blen[i])) blen[i] = std::min(std::max(blen[i], minLen), maxLen);
		hu_nni_opts no;
		hu_nni_default_opts(&no);
		std::vector<hu_nni_round> nrounds((size_t) nniRounds);
		no.blen.eps = mlEps; no.blen.min_len = minLen; no.blen.max_len = maxLen; no.blen.max_rounds = mlRounds; no.blen.host = host ? 1 : 0; no.blen.device = device;
		no.blen.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0;
		no.nni_rounds = nniRounds; no.min_gain = nniMinGain; no.rounds = nrounds.data(); no.rounds_cap = nniRounds;
		if(hu_tree_nni_search(&no, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), childOff.data(), childIdx.data(), &md) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		static const char* const why[] = {"local optimum", "no improving swap", "max rounds"};
		if(verbose) {
			char line[240];
			snprintf(line, sizeof(line), "NNI search: log-likelihood %.17g -> %.17g, %lld swap(s) applied in %d round(s), stop: %s", no.ll_start, no.ll_final, (long long) no.n_swaps, no.n_rounds, why[no.stop]);
			std::cerr << line << std::endl;
			if(no.skipped > 0) std::cerr << no.skipped << " edge(s) at polytomies were not scored" << std::endl;
			double s[4];
			hu_nni_timing(s);
			std::cerr << "fits " << s[0] << " s, scoring " << s[1] << " s, trials " << s[2] << " s, the rest " << s[3] << " s" << std::endl;
		}
		if(spr) {
			const long long moved = run_spr(seq);
			if(moved < 0) return EXIT_FAILURE;
			if(moved > 0) {
				/* the interchanges once more, on the tree the moves left; --nni-log holds the first search */
				hu_nni_opts no2;
				hu_nni_default_opts(&no2);
				no2.blen = no.blen; no2.nni_rounds = nniRounds; no2.min_gain = nniMinGain;
				if(hu_tree_nni_search(&no2, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), childOff.data(), childIdx.data(), &md) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
				if(verbose) {
					char line[240];
					snprintf(line, sizeof(line), "NNI search after the moves: log-likelihood %.17g -> %.17g, %lld swap(s) applied in %d round(s), stop: %s", no2.ll_start, no2.ll_final, (long long) no2.n_swaps, no2.n_rounds, why[no2.stop]);
					std::cerr << line << std::endl;
				}
			}
		}
		std::vector<const char*> nodeName((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) nodeName[i] = nodeNames[i].c_str();
		const int64_t wl = hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), nullptr, 0);
		if(wl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) wl + 1, '\0');
		hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), &text[0], wl + 1);
		text.resize((size_t) wl);
		if(!nniLogFn.empty()) {
			FILE* f = fopen(nniLogFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << nniLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
			fprintf(f, "round\tll\tscored\tcandidates\ttaken\tapplied\n0\t%.17g\t0\t0\t0\t0\n", no.ll_start);
			for(int32_t r = 0; r < no.n_rounds; ++r) fprintf(f, "%d\t%.17g\t%d\t%d\t%d\t%d\n", r + 1, nrounds[r].ll, nrounds[r].scored, nrounds[r].candidates, nrounds[r].taken, nrounds[r].applied);
			fprintf(f, "# stop: %s\n# skipped: %lld edges at polytomies\n", why[no.stop], (long long) no.skipped);
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << nniLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		}
	}
	else if(mlLengths && spr) {
		std::vector<int8_t> seq((size_t) nn * L, (int8_t) -2);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		for(int32_t i = 0; i < nn; ++i) if(parent[i] >= 0 && std::isfinite(blen[i])) blen[i] = std::min(std::max(blen[i], minLen), maxLen);
		if(run_spr(seq) < 0) return EXIT_FAILURE;
		std::vector<const char*> nodeName((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) nodeName[i] = nodeNames[i].c_str();
		const int64_t wl = hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), nullptr, 0);
		if(wl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) wl + 1, '\0');
		hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), &text[0], wl + 1);
		text.resize((size_t) wl);
	}
	else if(mlLengths) {
		std::vector<int8_t> seq((size_t) nn * L, (int8_t) -2);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		/* a start outside the interval, a negative length of the joins' last node among them, begins at its nearer end */
		for(int32_t i = 0; i < nn; ++i) if(parent[i] >= 0 && std::isfinite(blen[i])) blen[i] = std::min(std::max(blen[i], minLen), maxLen);
		rounds.resize((size_t) mlRounds);
		bo.eps = mlEps; bo.min_len = minLen; bo.max_len = maxLen; bo.max_rounds = mlRounds; bo.host = host ? 1 : 0; bo.device = device;
		bo.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0; bo.rounds = rounds.data(); bo.rounds_cap = mlRounds;
		if(hu_tree_optimize_lengths(&bo, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), &md) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		static const char* const why[] = {"converged", "no improving step", "max rounds"};
		if(verbose) {
			char line[200];
			snprintf(line, sizeof(line), "Branch lengths fitted: log-likelihood %.17g -> %.17g in %d round(s), stop: %s", bo.ll_start, bo.ll_final, bo.n_rounds, why[bo.stop]);
			std::cerr << line << std::endl;
			if(bo.n_capped > 0) std::cerr << "Warning: " << bo.n_capped << " branch step(s) hit the cap of " << HU_BLEN_MAX_NEWTON << " Newton steps" << std::endl;
			double s[4];
			hu_blen_timing(s);
			std::cerr << "sweeps " << s[0] << " s, steps " << s[1] << " s, trial sweeps " << s[2] << " s, the rest " << s[3] << " s" << std::endl;
		}
		/* the handle knows the start tree alone: a grown tree is written from its arrays */
		std::vector<const char*> nodeName((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) nodeName[i] = nodeNames[i].c_str();
		const int64_t wl = grown ? hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), nullptr, 0) : hu_newick_write(nw.get(), blen.data(), nullptr, 0);
		if(wl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) wl + 1, '\0');
		if(grown) hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), &text[0], wl + 1);
		else hu_newick_write(nw.get(), blen.data(), &text[0], wl + 1);
		text.resize((size_t) wl);
		if(!mlLogFn.empty()) {
			FILE* f = fopen(mlLogFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << mlLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
			fprintf(f, "round\tll\ts\tdelta\tcapped\n0\t%.17g\t0\t0\t0\n", bo.ll_start);
			for(int32_t r = 0; r < bo.n_rounds; ++r) fprintf(f, "%d\t%.17g\t%.17g\t%.17g\t%lld\n", r + 1, rounds[r].ll, rounds[r].s, rounds[r].delta, (long long) rounds[r].n_capped);
			fprintf(f, "# stop: %s\n", why[bo.stop]);
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << mlLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		}
	}
	/* --support: the supports of the final tree's eligible edges become the labels of their lower ends */
	std::vector<std::string> finalLabel;                      /* of the tree as written, when --support has set labels */
	if(support) {
		std::vector<int8_t> seq((size_t) nn * L, (int8_t) -2);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		hu_support_opts so;
		hu_support_default_opts(&so);
		so.blen.min_len = minLen; so.blen.max_len = maxLen; so.blen.host = host ? 1 : 0; so.blen.device = device; so.blen.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0;
		so.replicates = (int32_t) supportN; so.seed = supportSeed;
		const int32_t cap = std::max((nn - 1) / 2, 1);
		std::vector<int32_t> eNode((size_t) cap), eCount((size_t) cap); std::vector<double> eT((size_t) cap * 3), eF((size_t) cap * 3);
		int32_t nE = 0; int64_t skipped = 0;
		if(hu_tree_nni_support(&so, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), &md, cap, &nE, &skipped, eNode.data(), eT.data(), eF.data(), eCount.data(), nullptr) != HU_OK) {
			std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		if(verbose) {
			std::cerr << "Local supports: " << nE << " edge(s) scored over " << supportN << " replicate(s), " << skipped << " edge(s) at polytomies skipped" << std::endl;
			double s[4];
			hu_support_timing(s);
			std::cerr << "sweep " << s[0] << " s, scoring " << s[1] << " s, weights " << s[2] << " s, supports " << s[3] << " s" << std::endl;
		}
		int32_t root = 0;
		for(int32_t i = 0; i < nn; ++i) if(parent[i] < 0) root = i;
		/* a root-spanning edge is scored from the smaller of the root's two children: the other one carries the label too */
		auto other_end = [&](int32_t u) -> int32_t {
			if(parent[u] != root || childOff[root + 1] - childOff[root] != 2) return -1;
			const int32_t c0 = childIdx[childOff[root]], c1 = childIdx[childOff[root] + 1];
			return c0 == u ? c1 : c0;
		};
		std::vector<std::string> label((size_t) nn);
		std::vector<const char*> nodeName((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) label[i] = nodeNames[i];
		for(int32_t e = 0; e < nE; ++e) {
			char num[32];
			snprintf(num, sizeof(num), "%.3f", (double) eCount[e] / (double) supportN);
			const int32_t u = eNode[e], s = other_end(u);
			if(label[u].empty()) label[u] = num;
			if(s >= 0 && label[s].empty()) label[s] = num;
		}
		finalLabel = label;
		for(int32_t i = 0; i < nn; ++i) nodeName[i] = label[i].c_str();
		const int64_t wl = hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), nullptr, 0);
		if(wl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) wl + 1, '\0');
		hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), &text[0], wl + 1);
		text.resize((size_t) wl);
		if(!supportFn.empty()) {
			/* the leaves below every node, counted upwards from every leaf */
			std::vector<int32_t> leaves((size_t) nn, 0);
			for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) for(int32_t v = i; v >= 0; v = parent[v]) leaves[v]++;
			FILE* f = fopen(supportFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << supportFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
			fprintf(f, "node\tname\tkind\tleaves\tt0\talrt\tcount\treplicates\tsupport\n");
			for(int32_t e = 0; e < nE; ++e) {
				const int32_t u = eNode[e], s = other_end(u);
				const bool root3 = parent[u] == root && s < 0;
				const double t0 = s >= 0 ? blen[u] + blen[s] : blen[u], alrt = 2.0 * (eF[(size_t) e * 3] - std::max(eF[(size_t) e * 3 + 1], eF[(size_t) e * 3 + 2]));
				fprintf(f, "%d\t%s\t%s\t%d\t%.17g\t%.17g\t%d\t%lld\t%.17g\n", u, nodeNames[u].c_str(), s >= 0 ? "root2" : root3 ? "root3" : "inner", leaves[u], t0, alrt,
					eCount[e], supportN, (double) eCount[e] / (double) supportN);
			}
			fprintf(f, "# skipped: %lld edges at polytomies\n# seed: %llu\n", (long long) skipped, supportSeed);
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << supportFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		}
	}
	/* --gamma: the last stage.  The lengths of the tree as it stands and the shape under the discrete Gamma of rates; the topology, the
	 * names, the order of children and the top node stay, and so do the labels of --support, which were computed on the lengths before */
	if(gamma) {
		std::vector<int8_t> seq((size_t) nn * L, (int8_t) -2);
		for(int32_t i = 0; i < nn; ++i) if(childOff[i] == childOff[i + 1]) memcpy(seq.data() + (size_t) i * L, rows.data() + (size_t) inp.name2row.at(nodeNames[i]) * L, L);
		hu_gamma_opts go;
		hu_gamma_default_opts(&go);
		std::vector<hu_gamma_pass> passes((size_t) gammaRounds);
		go.blen.eps = mlEps; go.blen.min_len = minLen; go.blen.max_len = maxLen; go.blen.max_rounds = mlRounds; go.blen.host = host ? 1 : 0; go.blen.device = device;
		go.blen.mem_budget = haveMem ? (int64_t)(memGB * 1e9) : 0;
		go.k = gammaK; go.alpha = haveGammaAlpha ? gammaAlpha : 0.0; go.max_outer = gammaRounds; go.eps_ll = gammaEps; go.passes = passes.data(); go.passes_cap = gammaRounds;
		if(hu_tree_gamma_fit(&go, nn, (int32_t) L, parent.data(), blen.data(), seq.data(), &md) != HU_OK) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		static const char* const why[] = {"converged", "max passes", "fixed alpha"};
		if(verbose) {
			char line[240];
			snprintf(line, sizeof(line), "Discrete Gamma of %d rates fitted: alpha %.17g, log-likelihood %.17g -> %.17g in %d pass(es), stop: %s", gammaK, go.alpha_fit, go.ll_start, go.ll_final, go.n_outer, why[go.stop]);
			std::cerr << line << std::endl;
			std::cerr << "rates:";
			for(int c = 0; c < gammaK; ++c) { snprintf(line, sizeof(line), " %.6g", go.rates[c]); std::cerr << line; }
			std::cerr << std::endl;
			for(int32_t r = 0; r < go.n_outer; ++r) {
				snprintf(line, sizeof(line), "pass %d: alpha %.17g, log-likelihood %.17g, %d round(s)", r + 1, passes[r].alpha, passes[r].ll, passes[r].n_rounds);
				std::cerr << line << std::endl;
			}
			if(go.n_capped > 0) std::cerr << "Warning: " << go.n_capped << " branch step(s) hit the cap of " << HU_BLEN_MAX_NEWTON << " Newton steps" << std::endl;
			double s[5];
			hu_gamma_timing(s);
			std::cerr << "shape searches " << s[0] << " s, sweeps " << s[1] << " s, steps " << s[2] << " s, trial sweeps " << s[3] << " s, the rest " << s[4] << " s" << std::endl;
		}
		/* written as the stage before wrote it: by the handle of the parsed tree, or from the arrays with the labels it gave */
		const bool fromArrays = grown || nni || spr || support;
		std::vector<const char*> nodeName((size_t) nn);
		for(int32_t i = 0; i < nn; ++i) nodeName[i] = finalLabel.empty() ? nodeNames[i].c_str() : finalLabel[i].c_str();
		const int64_t wl = fromArrays ? hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), nullptr, 0) : hu_newick_write(nw.get(), blen.data(), nullptr, 0);
		if(wl < 0) { std::cerr << hu_last_error() << std::endl; return EXIT_FAILURE; }
		text.assign((size_t) wl + 1, '\0');
		if(fromArrays) hu_newick_from_arrays(nn, parent.data(), childOff.data(), childIdx.data(), nodeName.data(), blen.data(), &text[0], wl + 1);
		else hu_newick_write(nw.get(), blen.data(), &text[0], wl + 1);
		text.resize((size_t) wl);
		if(!gammaLogFn.empty()) {
			FILE* f = fopen(gammaLogFn.c_str(), "w");
			if(!f) { std::cerr << "Unable to write to '" << gammaLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
			fprintf(f, "pass\talpha\tll\trounds\n0\t%.17g\t%.17g\t0\n", haveGammaAlpha ? gammaAlpha : 1.0, go.ll_start);
			for(int32_t r = 0; r < go.n_outer; ++r) fprintf(f, "%d\t%.17g\t%.17g\t%d\n", r + 1, passes[r].alpha, passes[r].ll, passes[r].n_rounds);
			fprintf(f, "# rates:");
			for(int c = 0; c < gammaK; ++c) fprintf(f, "%c%.17g", c ? '\t' : ' ', go.rates[c]);
			fprintf(f, "\n# stop: %s\n", why[go.stop]);
			if(fclose(f) != 0) { std::cerr << "Unable to write to '" << gammaLogFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		}
	}
	if(!distFn.empty()) {
		FILE* f = fopen(distFn.c_str(), "w");
		if(!f) { std::cerr << "Unable to write to '" << distFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		fprintf(f, "%zu\n", n);
		for(size_t i = 0; i < n; ++i) {
			fputs(nm[i], f);
			for(size_t j = 0; j < n; ++j) fprintf(f, "\t%.17g", D[i * n + j]);
			fputc('\n', f);
		}
		if(fclose(f) != 0) { std::cerr << "Unable to write to '" << distFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	}
	if(outFn.empty()) { std::cout << text; std::cout.flush(); }
	else {
		std::ofstream of(outFn, std::ios::binary);
		if(!of.is_open()) { std::cerr << "Unable to write to '" << outFn << "': " << strerror(errno) << std::endl; return EXIT_FAILURE; }
		of << text; of.flush();
		if(!of) { std::cerr << "Unable to write tree: " << strerror(errno) << std::endl; return EXIT_FAILURE; }
	}
	info("Tree written");
	return EXIT_SUCCESS;
}
