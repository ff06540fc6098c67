// hmmufotu-amd-train-hmm: a banded profile HMM (.hmm) trained on a reference MSA with Dirichlet priors — hmmufotu-train-hmm
// (src/hmmufotu-train-hmm.cpp:87-228, BandedHMMP7::build of src/BandedHMMP7.cpp:386-541), whose output is the <DB>.hmm that stands
// beside the <DB>.ptu of hmmufotu-amd-build --no-hmm.  The host reads the MSA exactly as the build program does (hu_build_inputs.h)
// and the prior file (hu_hmm_prior_read); the wide loops, the MSA statistics and the weighted counts over all cells, run on the device
// (hu_msa_stats, hu_hmm_counts); the effective sequence number and the probabilities are a few million lgamma calls on the host
// (hu_hmm_estimate).  Options, the prior file and the MSA are checked before a device is asked for.  DESIGN.md §15.
//   hmmufotu-amd-train-hmm <MSA-FILE> -dm FILE [-o FILE] [--fmt fasta] [-f|--symfrac DOUBLE] [--device N] [-v]
#include <algorithm>
#include <cstdlib>
#include <ctime>
#include "hu_build_inputs.h"

/* the parts of hu_build_inputs.h that need a tree are for the other programs */
static const auto unused_tree [[maybe_unused]] = &hu_load_tree;
static const auto unused_join [[maybe_unused]] = &hu_join_msa_tree;
static const auto unused_newick [[maybe_unused]] = &hu_is_newick_name;
static const auto unused_encode [[maybe_unused]] = &hu_encode_row;
static const auto unused_file [[maybe_unused]] = &read_file;

static const double DEFAULT_SYMFRAC = 0.5;     /* src/hmmufotu-train-hmm.cpp:50 */
static const size_t MAX_CS = 65535;            /* kMaxCS - 1, src/BandedHMMP7.h:279 */

static void usage(const char* p) {
	std::cerr << "Train a Banded-HMM model with customized data\n"
		"Usage:    " << p << "  <MSA-FILE> -dm FILE [options]\n"
		"MSA-FILE  FILE                   : a multiple-alignment sequence file, support .gz or .bz2 compressed file\n"
		"Options:    -dm FILE             : the trained Dirichlet Model (prior) file; required, there is no built-in one\n"
		"            -o FILE              : write output to FILE instead of stdout\n"
		"            --fmt  STR           : MSA format, supported format: 'fasta'\n"
		"            -f|--symfrac DOUBLE  : conservation threshold for considering a site as a Match state in HMM [" << DEFAULT_SYMFRAC << "]\n"
		"            --device  INT        : device index [0]\n"
		"            -v  FLAG             : enable verbose information\n"
		"            --version            : show program version and exit\n"
		"            -h|--help            : print this message and exit\n";
}

int main(int argc, char** argv) {
	std::vector<std::string> pos; std::string outFn, fmt, dmFn;
	double symfrac = DEFAULT_SYMFRAC;
	int device = 0, verbose = 0;
	if(argc == 1) { usage(argv[0]); return EXIT_SUCCESS; }
	for(int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto val = [&]() -> const char* { if(i + 1 >= argc) { std::cerr << "Error: option " << a << " needs a value\n"; exit(EXIT_FAILURE); } return argv[++i]; };
		if(a == "-h" || a == "--help") { usage(argv[0]); return EXIT_SUCCESS; }
		else if(a == "--version") { std::cerr << argv[0] << ": v1.5.1\nPackage: HmmUFOtu v1.5.1 (file formats and training semantics; hmmufotu_amd engine for gfx950)" << std::endl; return EXIT_SUCCESS; }
		else if(a == "-o") outFn = val(); else if(a == "--fmt") fmt = val();
		else if(a == "-dm") dmFn = val();
		else if(a == "-f" || a == "--symfrac") symfrac = atof(val());
		else if(a == "--device") device = atoi(val());
		else if(a.size() > 1 && a[0] == '-' && a.find_first_not_of('v', 1) == std::string::npos) verbose += (int) a.size() - 1;
		else if(a[0] == '-' && a.size() > 1) { std::cerr << "Error: unknown option " << a << std::endl; usage(argv[0]); return EXIT_FAILURE; }
		else pos.push_back(a);
	}
	if(pos.size() != 1) { std::cerr << "Error:" << std::endl; usage(argv[0]); return EXIT_FAILURE; }
	const HuInfo info = [&](const std::string& s) { if(verbose) std::cerr << s << std::endl; };
	const std::string seqFn = pos[0];
	/* main() lets 0 and 1 through (src/hmmufotu-train-hmm.cpp:129) and build() then throws (src/BandedHMMP7.cpp:390-391) */
	if(!(symfrac > 0 && symfrac < 1)) { std::cerr << "-f|--symfrac must between 0 and 1, both excluded" << std::endl; return EXIT_FAILURE; }
	if(dmFn.empty()) { std::cerr << "-dm FILE is required: no Dirichlet Model file is built in" << std::endl; return EXIT_FAILURE; }
	if(device < 0) { std::cerr << "--device must be non-negative" << std::endl; return EXIT_FAILURE; }
	/* guess input format (src/hmmufotu-train-hmm.cpp:149-163) */
	if(fmt.empty() && ends_with(seqFn, ".msa")) fmt = "msa";
	hu_guess_seq_format(seqFn, fmt);
	if(fmt == "msa") { std::cerr << "MSA format 'msa': the reference's binary .msa database is not read here; pass the alignment as FASTA" << std::endl; return EXIT_FAILURE; }
	if(fmt != "fasta") { std::cerr << "Unsupported sequence format '" << fmt << "'" << std::endl; return EXIT_FAILURE; }

	/* the prior, then the MSA */
	hu_hmm_prior prior;
	if(hu_hmm_prior_read(dmFn.c_str(), &prior) != HU_OK) { std::cerr << "Failed to read in the HMM Prior file: " << hu_last_error() << std::endl; return EXIT_FAILURE; }
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
		if(kept > MAX_CS) { std::cerr << "Unable to train the profile: the MSA has " << kept << " columns after pruning, the profile's index arrays end at " << MAX_CS << std::endl; return EXIT_FAILURE; }
		if(kept == 0) { std::cerr << "Unable to train the profile: the MSA has no column with a residue" << std::endl; return EXIT_FAILURE; }
	}

	/* the device: MSA::prune and the weighted counts of the MSA (one call on the text as read), then the match columns */
	if(hu_device_count() <= device) { std::cerr << "Error: device " << device << " asked for, " << hu_device_count() << " gfx950 device(s) visible" << std::endl; return EXIT_FAILURE; }
	std::string err;
	if(!hu_prune_msa(device, inp, info, err)) { std::cerr << "Error: " << err << std::endl; return EXIT_FAILURE; }
	const size_t L = (size_t) inp.L;
	std::vector<double> wres(4 * L), wgap(L);
	std::vector<int32_t> newCol(L0, -1);
	for(size_t j = 0; j < L; ++j) {
		const size_t c = inp.keep[j];
		newCol[c] = (int32_t) j;
		for(int b = 0; b < 4; ++b) wres[b * L + j] = inp.wres[b * L0 + c];
		wgap[j] = inp.wgap[c];
	}
	std::vector<uint8_t> mask(L); std::vector<int32_t> map(L); std::vector<char> cons(L); std::vector<double> ident(L);
	int32_t K = 0;
	if(hu_hmm_match_columns((int64_t) L, (int64_t) nSeq, wres.data(), wgap.data(), symfrac, mask.data(), &K, map.data(), cons.data(), ident.data()) != HU_OK) {
		std::cerr << "Unable to train the profile: " << hu_last_error() << std::endl; return EXIT_FAILURE;
	}
	info("Profile size: " + std::to_string(K) + " match columns of " + std::to_string(L));
	/* the pruned text; first and last residue in its columns (a column with a residue is always kept) */
	std::vector<char> text(nSeq * L);
	for(size_t i = 0; i < nSeq; ++i) { const char* src = inp.msa.data() + i * L0; char* dst = text.data() + i * L; for(size_t j = 0; j < L; ++j) dst[j] = src[inp.keep[j]]; }
	std::vector<char>().swap(inp.msa);
	std::vector<int32_t> st(nSeq), en(nSeq);
	for(size_t i = 0; i < nSeq; ++i) { st[i] = inp.start[i] < 0 ? -1 : newCol[(size_t) inp.start[i]]; en[i] = inp.end[i] < 0 ? -1 : newCol[(size_t) inp.end[i]]; }
	const size_t K1 = (size_t) K + 1;
	std::vector<double> em(K1 * 4), ei(K1 * 4), t(K1 * 9), pm(K1 * 4), pi(K1 * 4), pt(K1 * 9);
	if(hu_hmm_counts(device, (int64_t) nSeq, (int64_t) L, text.data(), inp.weight.data(), st.data(), en.data(), mask.data(), K, em.data(), ei.data(), t.data()) != HU_OK) {
		std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE;
	}
	double effN = 0; int32_t passes = 0;
	if(hu_hmm_estimate(K, em.data(), ei.data(), t.data(), (int64_t) nSeq, &prior, pm.data(), pi.data(), pt.data(), &effN, &passes) != HU_OK) {
		std::cerr << "Error: " << hu_last_error() << std::endl; return EXIT_FAILURE;
	}
	info("Effective sequence number: " + std::to_string(effN) + " of " + std::to_string(nSeq) + " after " + std::to_string(passes) + " bisection passes");
	info("Banded HMM profile trained");

	/* output: NAME is the input as given (MSA::setName(inFn), src/hmmufotu-train-hmm.cpp:205), DATE %c of the local time (src/BandedHMMP7.cpp:533-538) */
	char date[128];
	const time_t now = time(nullptr);
	strftime(date, sizeof(date), "%c", localtime(&now));
	if(hu_hmm_write(outFn.empty() ? "-" : outFn.c_str(), "hmmufotu-amd-train-hmm-v1.5.1", seqFn.c_str(), K, (int32_t) L, pm.data(), pi.data(), pt.data(), map.data(), cons.data(),
			(int64_t) nSeq, effN, date) != HU_OK) { std::cerr << "Unable to write to " << (outFn.empty() ? "stdout" : outFn) << ": " << hu_last_error() << std::endl; return EXIT_FAILURE; }
	info("Banded HMM profile written");
	return EXIT_SUCCESS;
}
