/*
 * hmmufotu_amd — C ABI of the MI355X-native per-read assignment engine.
 *
 * The reference (HmmUFOtu v1.5.1) has no plugin/FFI layer; its seam for this path is the C++
 * free-function API of src/HmmUFOtu_main.h:70-113 called once per read from the OpenMP task in
 * src/hmmufotu.cpp:603-751.  This header is the batched, POD-only replacement of that seam:
 * every entry point names the reference function(s) it stands in for.  Host code that keeps
 * the per-read reference signatures lives in hmmufotu_amd/csrc/hu_reference_api.hpp.
 *
 * Conventions: all pointers are HOST pointers unless a field says "device"; the caller owns
 * every in/out buffer; functions return HU_OK (0) or a negative hu_status and never abort;
 * hu_last_error() returns a thread-local message.  One hu_batch is driven by one host thread
 * (it owns a HIP stream); several batches may share one hu_db concurrently (the DB is
 * immutable after creation, like the const BandedHMMP7 / PTUnrooted objects of the reference).
 */
#ifndef HMMUFOTU_AMD_H_
#define HMMUFOTU_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
	HU_OK = 0,
	HU_ERR_ARG = -1,      /* invalid argument (reference: assert / invalid_argument)            */
	HU_ERR_DEVICE = -2,   /* no gfx950 device / HIP failure: the engine has NO CPU fallback      */
	HU_ERR_IO = -3,       /* unreadable or malformed database file                                */
	HU_ERR_NOMEM = -4,
	HU_ERR_STATE = -5,    /* stage called out of order                                            */
	HU_ERR_NUMERIC = -6   /* an iteration that did not converge, or an answer the input does not have */
} hu_status;

/* align_mode of src/BandedHMMP7.h:168-173 */
enum { HU_MODE_GLOBAL = 0, HU_MODE_LOCAL = 1, HU_MODE_NGCL = 2, HU_MODE_CGNL = 3 };
/* DNA substitution models of src/DNASubModelFactory.cpp:38-53 */
enum { HU_GTR = 0, HU_TN93 = 1, HU_HKY85 = 2, HU_F81 = 3, HU_K80 = 4, HU_JC69 = 5 };
/* PTUnrooted::PRIOR_TYPE */
enum { HU_PRIOR_UNIFORM = 0, HU_PRIOR_HEIGHT = 1 };

/* per-read status flags (replace the reference's assert(aln.isValid()) aborts, src/hmmufotu.cpp:622) */
enum {
	HU_READ_OK = 1,
	HU_READ_INVALID = 0,      /* bad base code or no finite Viterbi path                            */
	HU_READ_CHIMERA = 2,      /* PE orientation check failed (src/hmmufotu.cpp:629-637)             */
	HU_READ_NEEDS_FULL = 4,   /* internal: banded DP found no path, full DP scheduled              */
	HU_READ_OUT_OF_WINDOW = 16 /* aligned, but its CS region leaves the column window the database keeps messages for
	                            * (hu_tree_desc.win_*): not placed, no TSV line; the rest of the batch goes on   */
};

/* capacity of the per-read seed lists: max_nseed <= HU_MAX_SEEDS, and the per-seed result arrays of
 * hu_batch_get_seeds / hu_batch_get_estimates / hu_seed_batch_given have this ROW STRIDE whatever max_nseed is */
#define HU_MAX_SEEDS 64

typedef struct hu_db hu_db;        /* profile + pre-evaluated tree packed once into HBM             */
typedef struct hu_batch hu_batch;  /* device workspace + stream for one batch of reads in flight    */

/* BandedHMMP7 profile fields as operator>> leaves them (src/BandedHMMP7.cpp:100-246,
 * src/BandedHMMP7.h:499-548): costs are -ln p, '*' == +inf.  hu_db_create runs the post-load
 * chain itself (extend_index, adjustProfileLocalMode, wingRetract; :104-109, :1083-1120). */
typedef struct {
	int32_t K;                /* profile length (LENG)                                             */
	int32_t L;                /* consensus length (MAXL)                                           */
	const double* EM;         /* [K+1][4] match emission costs, row 0 = COMPO                      */
	const double* EI;         /* [K+1][4] insert emission costs                                    */
	const double* T;          /* [K+1][7] transition costs m->m m->i m->d i->m i->i d->m d->d      */
	const int32_t* p2cs;      /* [K+1] MAP: 1-based CS column of profile column k; [0] ignored     */
} hu_profile_desc;

/* DNASubModel + DiscreteGammaModel parameters (src/GTR.cpp:43-81, src/TN93.cpp:40-77, ...;
 * src/DiscreteGammaModel.cpp:57-72).  par: GTR R[16] row-major | TN93 kr,ky,beta |
 * HKY85 kappa,beta | F81 beta | K80 kappa | JC69 -.  pi is ignored for K80/JC69. */
typedef struct {
	int32_t type;
	double pi[4];
	double par[16];
	int32_t dg_k;             /* 0 = no discrete Gamma                                             */
	double dg_rate[16];       /* r[k] exactly as stored in the .ptu (NOT multiplied by K)          */
} hu_model_desc;

/* PTUnrooted as loaded from a .ptu (src/PhyloTreeUnrooted.cpp:496-535): node i is id2node[i].
 * up[i] is the cached message of branch i -> parent(i), down[i] that of parent(i) -> i
 * (Matrix4Xd 4 x csLen, column-major == [site][4]); for the root, up[root] holds the root
 * message.  Messages may be given for a column window only (win_len < cs_len). */
typedef struct {
	int32_t n_nodes;
	int32_t cs_len;
	const int32_t* parent;    /* [n] -1 for the root                                               */
	const double* blen;       /* [n] length of the branch to the parent                            */
	const int8_t* seq;        /* [n][cs_len] DigitalSeq codes: 0..3, gap -2                        */
	const double* up;         /* [n][win_len][4]                                                   */
	const double* down;       /* [n][win_len][4]                                                   */
	const double* height;     /* [n] node2height                                                   */
	const int32_t* anno_id;   /* [n] class of the node's taxon annotation string (may be NULL)     */
	const double* anno_dist;  /* [n] annoDist (may be NULL)                                        */
	int64_t win_start;        /* first CS column (0-based) covered by up/down                      */
	int64_t win_len;          /* 0 = all cs_len columns                                            */
	int32_t msgs_on_device;   /* up/down are DEVICE pointers the DB adopts: not copied, not freed, and
	                           * REWRITTEN IN PLACE into the engine's packed linear form             */
} hu_tree_desc;

/* CLI defaults of src/hmmufotu.cpp:37-57 */
typedef struct {
	int32_t align_mode;       /* HU_MODE_GLOBAL for assembled/PE reads, HU_MODE_NGCL for --single  */
	int32_t max_nseed;        /* -N  [50]                                                          */
	double max_diff;          /* -d  [inf]                                                         */
	double max_height;        /* -H  [inf]                                                         */
	double max_error;         /* -e  [20]                                                          */
	int32_t weighted;         /* -m  0 'unweighted' [default], 1 'weighted'                        */
	int32_t only_ml;          /* --ML                                                              */
	int32_t prior;            /* --prior                                                           */
	int32_t ignore_orient;    /* -i                                                                */
	int32_t fix_root_loglik;  /* 0 [default]: placeSeq's loglik as the reference computes it — the constant
	                           * (end - start + 1) log(sum_i pi_i e) of SURVEY.md F4 (src/PhyloTreeUnrooted.cpp:918-922), so every
	                           * candidate ties and the pick follows the estimated order.  1 (--fix-root-loglik): the value evidently
	                           * intended, sum_j log pi . exp(loglik(r, j)) at the optimised branch lengths; candidates are then
	                           * ranked by it (q-values, --ML sort, chimera log-odds all become informative).  A documented
	                           * deviation from the reference, off by default                                          */
	int32_t seed_order;       /* which of the nodes that TIE at the cut-off distance getSeed keeps, and in which order the seeds reach estimateSeq:
	                           * HU_SEED_ORDER_LIBSTDCXX (1, the default of hu_default_opts): the reference's own — the first max_nseed elements of
	                           * std::sort(locs) on dist ALONE (src/HmmUFOtu_main.cpp:139, src/hmmufotu.cpp:646-647), i.e. the tie permutation of
	                           * libstdc++'s introsort over all ~n_nodes PTLocs in node order.  Reproduced ON THE DEVICE (full (d, N) pair scan +
	                           * k_seed_refsort: data-parallel Hoare partitions restricted to the ranges that reach the first max_nseed places).
	                           * The host restatement (hu_sort_prefix_libstdcxx) finishes only the reads the kernel lists: a row that reaches
	                           * introsort's heap-sort branch, level tables that overflow, and every read of a tree whose sort tables exceed
	                           * 150 KB of LDS (its index of every 64th table entry: above ~9 M nodes; reported once on stderr and in hu_batch_refsort_stats).  A read with a NaN
	                           * distance (a node sharing no column with it: std::sort is undefined) takes (dist, node id) with NaN last.
	                           * HU_SEED_ORDER_STABLE (0): ascending (dist, node id) — independent of any library's tie permutation, selected by
	                           * the distance-only scan + top-k; ~25 % faster, differs from a g++-built reference wherever nodes tie at the
	                           * cut-off distance.  NOTE: a zero-filled hu_opts selects STABLE; call hu_default_opts. */
} hu_opts;
enum { HU_SEED_ORDER_STABLE = 0, HU_SEED_ORDER_LIBSTDCXX = 1 };

/* BandedHMMP7::HmmAlignment minus the string (src/BandedHMMP7.h:74-130) */
typedef struct {
	int32_t seq_start, seq_end, hmm_start, hmm_end, cs_start, cs_end; /* all 1-based */
	int32_t status;           /* HU_READ_*                                                          */
	int32_t used_full;        /* 1 if the full-DP fallback ran (src/HmmUFOtu_main.cpp:89-93)        */
	double cost;
} hu_align_rec;

/* PTUnrooted::PTPlacement (src/PhyloTreeUnrooted.h:410-510) with node ids instead of pointers */
typedef struct {
	int32_t c_node, p_node, a_node;
	int32_t n_cand;           /* candidates that survived filterPlacements                          */
	double wuv, ratio, wnr, loglik, height, q_place, q_taxon, anno_dist, est_loglik;
	double root_loglik;       /* with fix_root_loglik: the intended root log-likelihood (== loglik then); NaN otherwise.  The
	                           * reference's constant is (cs_end - cs_start + 1) * log(sum_i pi_i e) either way           */
} hu_place_rec;

void hu_default_opts(hu_opts* o);
const char* hu_last_error(void);
/* number of usable gfx950 devices (0 => every compute entry point fails with HU_ERR_DEVICE) */
int hu_device_count(void);

/* ---- database ---------------------------------------------------------------------------
 * replaces: hmmIn >> hmm, ptu.load(ptuIn), hmm.setSequenceMode/wingRetract
 * (src/hmmufotu.cpp:457-498) */
int hu_db_create(const hu_profile_desc* prof, const hu_tree_desc* tree, const hu_model_desc* model,
		int device, hu_db** out);
/* same from the reference's on-disk formats (.hmm text, .ptu binary) */
int hu_db_load(const char* hmm_path, const char* ptu_path, int device, hu_db** out);
/* the same keeping only the messages of the CS columns [win_start, win_start + win_len) on the device (win_len 0: all) — one shard of a database
 * held as column windows, see "column-window sharding" below */
int hu_db_load_window(const char* hmm_path, const char* ptu_path, int device, int64_t win_start, int64_t win_len, hu_db** out);
/* The reference's own TEXT forms, from memory — for a caller that holds loaded reference objects: BandedHMMP7 keeps its cost
 * matrices private and has no accessors for them (src/BandedHMMP7.h:497-548), but operator<<(ostream&, const BandedHMMP7&)
 * (src/BandedHMMP7.cpp:324-378) writes exactly what hu_profile_desc wants; likewise DNASubModel::write (src/GTR.cpp:83-104 and
 * friends).  hu_profile_parse_text: first call with NULL arrays for K and L, then with EM/EI [K+1][4], T [K+1][7], p2cs [K+1].
 * hu_model_parse_text fills type, pi and par; dg_k / dg_rate are the caller's (DiscreteGammaModel::getK / rate(k)). */
int hu_profile_parse_text(const char* text, int64_t len, int32_t* K, int32_t* L, double* EM, double* EI, double* T, int32_t* p2cs);
int hu_model_parse_text(const char* text, int64_t len, hu_model_desc* out);
/* host-only parse of the two database files (no device needed): sizes with fill = 0, then the arrays a non-NULL pointer names;
 * up / down [n][cs_len][4] are the whole message set (use it on test-sized files) */
int hu_files_parse(const char* hmm_path, const char* ptu_path, int32_t* K, int32_t* L, int32_t* n_nodes, int32_t* root,
		double* EM, double* EI, double* T, int32_t* p2cs, double* entry_cost, double* exit_cost,
		int32_t* parent, double* blen, int8_t* seq, double* height, double* up, double* down, hu_model_desc* model, int fill);
/* host-only: the spectral form P(t) = U diag(exp(lam t)) U1 the kernels use for a model (U, U1 [16] row-major, lam [4]) */
int hu_model_spectral(const hu_model_desc* model, double* U, double* lam, double* U1);
void hu_db_destroy(hu_db* db);
int hu_db_info(const hu_db* db, int32_t* K, int32_t* cs_len, int32_t* n_nodes, int32_t* root, int64_t* hbm_bytes);
/* host copies of what the readers parsed (for format tests); any pointer may be NULL */
int hu_db_get_profile(const hu_db* db, double* EM, double* EI, double* T, int32_t* p2cs,
		double* entry_cost, double* exit_cost);
int hu_db_get_tree(const hu_db* db, int32_t* parent, double* blen, int8_t* seq, double* height);
int hu_db_get_model(const hu_db* db, hu_model_desc* out);
/* PTUNode::getAnno() of a node of a database loaded with hu_db_load ("" otherwise) */
const char* hu_db_get_annotation(const hu_db* db, int32_t node);
/* device-side DNASubModel::Pr(t) (src/GTR.h:116-121 and friends), for parity tests */
int hu_db_model_pr(const hu_db* db, int n, const double* t, double* P /* [n][16] row-major */);

/* ---- tree pre-evaluation (the core of hmmufotu-build) ---------------------
 * Messages of every directed edge by a post-order and a pre-order sweep, equivalent to the reference's
 * "setRoot(i); evaluate()" loop over all nodes (src/hmmufotu-build.cpp:454-459), with the discrete
 * Gamma averaging of src/PhyloTreeUnrooted.cpp:320-346; ancestral sequences by per-site argmax
 * (src/PhyloTreeUnrooted.cpp:1085-1093), node heights (:274-287).  seq [n][cs_len] holds the leaf
 * rows on entry; inner rows are filled inside the column window.  up_dev/down_dev are DEVICE buffers
 * [n][win_len][4] (log space, the .ptu convention; up[root] = root message) that can be handed to
 * hu_db_create with msgs_on_device = 1. */
int hu_tree_evaluate(int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, int8_t* seq,
		const hu_model_desc* model, int device, int64_t win_start, int64_t win_len, double* up_dev, double* down_dev, double* height);

/* PTUnrooted::save (src/PhyloTreeUnrooted.cpp:537-567): writes the .ptu database file hmmufotu and hu_db_load read, from the arrays of a
 * hu_tree_desc (whole messages: win_len 0; up / down may be DEVICE buffers as hu_tree_evaluate leaves them — msgs_on_device = 1 — and are
 * then streamed to the file edge by edge).  names / annos: n C strings each (NULL: "n<i>" / "").  model_text: the model block as the
 * reference writes it (DNASubModel::write), or NULL to have it generated from `model`.  dg_alpha, dg_breaks [dg_k + 1]: what
 * DiscreteGammaModel::save stores beside the rates (the engine itself reads only the rates). */
int hu_ptu_write(const char* path, const hu_tree_desc* tree, const char* const* names, const char* const* annos, const hu_model_desc* model,
		const char* model_text, double dg_alpha, const double* dg_breaks);

/* ---- build statistics (the MSA and mutation-count loops of hmmufotu-build) -------------------------
 * MSA statistics on the device: MSA::updateRawCounts, updateSeqWeight and updateWeightedCounts (src/MSA.cpp:226-293) of the loaded
 * alignment, msa = n_seq rows of cs_len bytes, row-major, as read (case kept).  Every byte is classified by encode(toupper(c)) of the
 * MSA's IUPACNucl alphabet: hu_msa_encode_table gives that table (0..3 residue, a degenerate letter as the first base of its expansion,
 * -2 gap, -1 anything else).  Outputs, all host:
 *   res_count [4][cs_len], gap_count [cs_len]: raw counts; the columns with no residue are the ones MSA::prune drops (src/MSA.cpp:87-138);
 *   start / end / len [n_seq]: first / last residue column (-1 if none), in the input's columns, and the residue count;
 *   seq_weight [n_seq]: position-specific weights, each summed over columns in serial j order on the device, then scaled to sum n_seq
 *     on the host with a serial sum (the reference's seqWeight.sum() is an Eigen reduction);
 *   res_wcount [4][cs_len], gap_wcount [cs_len]: weighted counts, each summed over sequences in serial i order.
 * Dropping columns without residues changes none of these for the columns that stay (pruned columns add no weight), so one call on the
 * unpruned alignment gives the values the reference computes after prune(). */
int hu_msa_encode_table(int8_t* out /* [256] */);
int hu_msa_stats(int device, int64_t n_seq, int64_t cs_len, const char* msa, int32_t* res_count, int32_t* gap_count,
		int32_t* start, int32_t* end, int32_t* len, double* seq_weight, double* res_wcount, double* gap_wcount);
/* PhyloTreeUnrooted::estimateNumMutations (src/PhyloTreeUnrooted.cpp:1008-1016) for every column: the non-root nodes whose inferState
 * differs from their parent's.  inferState is the first maximum (Eigen maxCoeff) of the node's own message, up[node], leaves included;
 * a gap leaf's message is log pi (src/PhyloTreeUnrooted.h:1431-1437), so its state is the first maximum of pi.  up_dev: DEVICE [n_nodes][cs_len][4], the whole-column up buffer of hu_tree_evaluate with a
 * fixed-rate model.  counts: host [cs_len].  Needs n_nodes x cs_len bytes of device scratch. */
int hu_tree_count_mutations(int device, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* up_dev, int32_t* counts);
/* DiscreteGammaModel::setBreaks / setRates (src/DiscreteGammaModel.cpp:40-55), host only: breaks [K + 1] (last +inf), rates [K] (sum 1) */
int hu_dg_model(int32_t K, double alpha, double* breaks, double* rates);
/* DiscreteGammaModel::estimateShapeMoment (src/DiscreteGammaModel.cpp:92-98): mean^2 / (var - mean), sums in serial order; +inf when
 * n < 2; <= 0 (or NaN) means near-invariant rates, which hmmufotu-build answers with the fixed-rate model (src/hmmufotu-build.cpp:437-446) */
double hu_dg_estimate_shape(int64_t n, const double* X);

/* ---- the rest of hmmufotu-build --no-hmm (src/hmmufotu-build.cpp:346-503 without the csfm, hmm and msa parts) ----
 * Newick reader, host only: the grammar of src/NewickTree.h:186-215 as NewickTree::read applies it (src/NewickTree.cpp:37-59:
 * phrase_parse with a white-space skipper, and the whole text must be consumed).  subtree = [ '(' subtree (',' subtree)* ')' ] [label]
 * [':' double]; tree = subtree ';'.  An unquoted label is a run of printable characters without blanks and ( ) [ ] ' : ; ,  — a quoted
 * one is '...' with no quote inside (blanks inside are kept), and its name is the text between the quotes.  Node ids are those of
 * PTUnrooted(const NewickTree&) (src/PhyloTreeUnrooted.cpp:131-154): depth-first from the root (id 0) with an explicit stack, children
 * pushed in file order, so the LAST child of a node gets the smallest id among its siblings.
 * Refused with HU_ERR_IO and a message that names the byte offset: unbalanced brackets, a missing ';', text after the closing ';',
 * a ':' without a number, an empty tree (no token before the end).
 * hu_newick_get: parent [n] (-1 for the root), blen [n] (a missing length is 0, and so is the root's: the reference never reads it),
 * child_off [n + 1] / child_idx [n - 1]: every node's children IN FILE ORDER, the order of addEdge (:170-179) and so of the node's
 * neighbour list behind its parent in a reference-built .ptu.  Any pointer may be NULL. */
typedef struct hu_newick hu_newick;
int hu_newick_parse(const char* text, int64_t len, hu_newick** out);
void hu_newick_free(hu_newick* t);
int hu_newick_size(const hu_newick* t, int32_t* n_nodes);
int hu_newick_get(const hu_newick* t, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx);
const char* hu_newick_name(const hu_newick* t, int32_t node);   /* "" for an unnamed node; lives as long as t */

/* The annotation steps of the build, host only, on a tree whose branch lengths are final (after fixBranchLength):
 *   loadAnnotation (src/PhyloTreeUnrooted.cpp:223-240) when anno_text is not NULL: lines "name<TAB>annotation"; a node whose NAME is
 *     a key takes the annotation as its new name (a later line for the same key wins; a line without a TAB keeps the annotation of the
 *     line before it, as the reference's getline on an exhausted stream does);
 *   formatName / formatTaxonName (:974-986): the name split at any of ";: " (TAXON_SEP, adjacent separators as one), the fields
 *     isCanonicalName accepts (longer than 3 bytes and starting with one of d__ k__ p__ c__ o__ f__ g__ s__, src/PhyloTreeUnrooted.h:1564-1574)
 *     joined with ";";
 *   annotate (:988-1006): from the node towards the root until a node whose name isFullCanonicalName (field i starts with the prefix of
 *     level i: k p c o f g s, :956-963) or the root; the branch lengths walked are added to anno_dist in that order, partially canonical
 *     names (:965-972) on the way are collected, and the annotation is their join with ";" from the root's side, or root_name
 *     (NULL: "cellular_organisms") when there is none.
 * Results through the handle: names and annotations per node, anno_dist [n]. */
typedef struct hu_tree_anno hu_tree_anno;
int hu_tree_annotate(int32_t n_nodes, const int32_t* parent, const double* blen, const char* const* names, const char* anno_text,
		int64_t anno_len, const char* root_name, hu_tree_anno** out);
void hu_tree_anno_free(hu_tree_anno* a);
const char* hu_tree_anno_name(const hu_tree_anno* a, int32_t node);
const char* hu_tree_anno_anno(const hu_tree_anno* a, int32_t node);
int hu_tree_anno_dist(const hu_tree_anno* a, double* anno_dist /* [n] */);

/* PTUnrooted::treeLoglik() (src/PhyloTreeUnrooted.cpp:707-712, src/PhyloTreeUnrooted.h:1341-1343): per column
 * dot_product_scaled(pi, up[root][:, j]) (:1505-1510) = log(pi . exp(v + s)) - s with s = -510 - max(v) when max(v) is finite and below
 * -510 (MIN_LOGLIK_EXP), else 0 — on the device, one lane per column, from the root message hu_tree_evaluate leaves at up_dev[root]
 * (up_dev: DEVICE [n_nodes][cs_len][4], whole columns).  per_col: host [cs_len] (may be NULL); *sum: their sum in serial j order on
 * the host, so it depends on no reduction tree. */
int hu_tree_loglik(int device, int32_t n_nodes, int32_t cs_len, int32_t root, const hu_model_desc* model, const double* up_dev,
		double* per_col, double* sum);

/* Device memory for a caller of hu_tree_evaluate that holds no HIP runtime of its own (hmmufotu-amd-build): free and total bytes of the
 * device, and a buffer on it.  hu_device_malloc: HU_ERR_NOMEM when the device cannot back it. */
int hu_device_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes);
int hu_device_malloc(int device, int64_t bytes, void** out);
void hu_device_free(int device, void* p);

/* hu_ptu_write for a real build.  The same arguments, and
 *   child_off [n + 1] / child_idx [n - 1]: every node's children in the order to write them behind its parent (hu_newick_get gives the
 *     reference's: file order); NULL: ascending id, as hu_ptu_write;
 *   msa_row_of_leaf [n]: the MSA row of every leaf (other nodes: -1); the MSA index block then holds (row, node id) in ascending row as
 *     PTUnrooted::saveMSAIndex writes its map (src/PhyloTreeUnrooted.cpp:569-578); NULL: the k-th leaf in node order, as hu_ptu_write;
 *   staging_bytes: size of each of the two staging buffers (0: 256 MB); rounded down to whole messages, at least one.
 * With msgs_on_device the payloads of a run of consecutive directed edges (and the root row, last) are packed by k_ptu_gather into a
 * device staging buffer, copied with ONE hipMemcpyAsync into page-locked memory and written from there, header and payload
 * alternately, while the next run is gathered and copied on the other stream (hu_ptu_write: one blocking copy per edge).  up / down
 * must then be 16-byte aligned.  Host-resident messages take the plain loop.  The stream is checked after every run: a short write
 * ends the call with HU_ERR_IO.  With NULL child order and NULL rows the file is byte for byte hu_ptu_write's. */
int hu_ptu_write_stream(const char* path, const hu_tree_desc* tree, const char* const* names, const char* const* annos, const hu_model_desc* model,
		const char* model_text, double dg_alpha, const double* dg_breaks, const int32_t* child_off, const int32_t* child_idx,
		const int32_t* msa_row_of_leaf, int64_t staging_bytes);

/* ---- column-windowed builds: a database whose messages do not fit one device (hmmufotu-amd-build --col-window) ----
 * Felsenstein's recursion (src/PhyloTreeUnrooted.cpp:315-374) treats every column on its own, so the sweep, the mutation counts
 * (hu_tree_count_mutations with cs_len = win_len), the log-likelihoods (hu_tree_loglik with cs_len = win_len) and the file's payloads can be
 * made a window of columns at a time; every value is bit-equal to the whole-width entries' for the same column.
 *
 * hu_tree_sweep_*: hu_tree_evaluate held across windows.  create sends the topology, the level order and the branch lengths to the device
 * once (28 n bytes; the tree is checked before a device is asked for); window sends the [n_nodes][win_len] bytes of seq's columns
 * [win_start, win_start + win_len), runs the level kernels with the window's stride, and puts the inferred inner rows of these columns back
 * into seq (host [n_nodes][cs_len], leaf rows on entry, as hu_tree_evaluate).  Nothing on the device is sized by n_nodes x cs_len: beside the
 * caller's up_dev / down_dev (DEVICE [n_nodes][win_len][4]) the handle keeps n_nodes x (the widest win_len seen) bytes.  down_dev NULL: the
 * post-order levels only, which is all hu_tree_count_mutations reads (pass 1 of -V, src/hmmufotu-build.cpp:431-447).  heights: calcNodeHeight
 * (:274-287), host only. */
typedef struct hu_tree_sweep hu_tree_sweep;
int hu_tree_sweep_create(int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, int device, hu_tree_sweep** out);
int hu_tree_sweep_window(hu_tree_sweep* s, const hu_model_desc* model, int8_t* seq, int64_t win_start, int64_t win_len, double* up_dev, double* down_dev);
int hu_tree_sweep_heights(const hu_tree_sweep* s, double* height);
void hu_tree_sweep_destroy(hu_tree_sweep* s);

/* hu_ptu_writer_*: PTUnrooted::save (src/PhyloTreeUnrooted.cpp:537-567) fed a window at a time; the file is byte for byte hu_ptu_write_stream's.
 * The format keeps every directed edge's [cs_len][4] payload contiguous, so the layout is computed first: 32 header bytes, the node section
 * (per node 49 + 2 |name| + cs_len + |annotation| bytes: known without the inner rows), 8 bytes of edge count, 2 (n - 1) edge records of
 * 33 + 32 cs_len bytes in hu_ptu_write_stream's order, the root row of 8 + 32 cs_len bytes, the tail.
 *   open: tree gives n_nodes, cs_len, parent, blen and anno_dist (its other fields are not read); names, annos, child_off / child_idx,
 *     msa_row_of_leaf and staging_bytes as hu_ptu_write_stream.  Sizes the file up to the tail and writes every record's header.  Needs no device.
 *   window: up / down [n_nodes][win_len][4] of the columns [win_start, win_start + win_len), in any order of windows.  on_device = 1: DEVICE
 *     buffers on the current device, 16-byte aligned; runs of consecutive records' 32 win_len-byte pieces are packed by k_ptu_gather (pieces =
 *     2 win_len) into one of two staging buffers, copied on one of two streams and placed by the host at record offset + 33 + 32 win_start
 *     (root row: + 8) with positioned writes, while the next run is gathered.  on_device = 0: host buffers, no device needed.
 *   close: writes the node section from seq [n_nodes][cs_len] (all inner rows are known now) and the tail (height, model, model_text, dg_alpha,
 *     dg_breaks as hu_ptu_write).  HU_ERR_STATE unless the windows given tile [0, cs_len) exactly once.  Frees the handle in every case.
 *   abort: frees the handle and removes the file.
 * Every write's result is checked; a failed write, a failed close and abort leave no file behind. */
typedef struct hu_ptu_writer hu_ptu_writer;
int hu_ptu_writer_open(const char* path, const hu_tree_desc* tree, const char* const* names, const char* const* annos, const int32_t* child_off,
		const int32_t* child_idx, const int32_t* msa_row_of_leaf, int64_t staging_bytes, hu_ptu_writer** out);
int hu_ptu_writer_window(hu_ptu_writer* w, int64_t win_start, int64_t win_len, const double* up, const double* down, int on_device);
int hu_ptu_writer_close(hu_ptu_writer* w, const int8_t* seq, const double* height, const hu_model_desc* model, const char* model_text,
		double dg_alpha, const double* dg_breaks);
void hu_ptu_writer_abort(hu_ptu_writer* w);

/* The window width of a build, host only.  hu_build_window_need: the device bytes a windowed build of n nodes holds at width W,
 *   need(W) = 64 n W                           up and down of the second pass, the wider one (the first holds up alone)
 *           + n W                              the sweep's sequence bytes
 *           + (with_var ? n W + 4 W + 4 n : 0)  hu_tree_count_mutations: states, counts, parents
 *           + 8 W                              hu_tree_loglik's column values
 *           + 2 stage(W) + 8 n                 the writer's two staging buffers and its record codes,
 *                                              stage(W) = max(32 W, min(2^28, (2 n - 1) 32 W))
 *           + 28 n + 64                        the sweep's per-node arrays
 * which grows with W.  hu_build_window_plan: the largest W <= cs_len with need(W) <= budget_bytes, rounded down to a multiple of 256 when it is
 * 256 or more (whole workgroups of the level kernels), and need(W) in *need_bytes.  HU_ERR_NOMEM when not even one column fits: *win_len = 0,
 * *need_bytes = need(1), and the message names both numbers. */
int64_t hu_build_window_need(int32_t n_nodes, int32_t win_len, int with_var);
int hu_build_window_plan(int32_t n_nodes, int32_t cs_len, int with_var, int64_t budget_bytes, int32_t* win_len, int64_t* need_bytes);

/* ---- the tree of a .ptu without its messages (host only, no device): what the consumers of an assignment file need of the database —
 * hmmufotu-sum the nodes' taxon annotations (src/hmmufotu-sum.cpp:378-383), hmmufotu-jplace the topology, branch lengths and the order of
 * every node's children as PTUnrooted::load leaves it (src/hmmufotu-jplace.cpp:197, src/PhyloTreeUnrooted.cpp:1135-1157).  The 4 x csLen
 * doubles of every directed edge are read past, never kept. */
typedef struct hu_tree_info hu_tree_info;
int hu_tree_info_load(const char* ptu_path, hu_tree_info** out);
void hu_tree_info_free(hu_tree_info* t);
int hu_tree_info_get(const hu_tree_info* t, int32_t* n_nodes, int32_t* cs_len, int32_t* root, hu_model_desc* model);
/* node i: parent (-1: root), length of the branch to it, annotation distance, leaf flag; the strings live as long as t */
int hu_tree_info_node(const hu_tree_info* t, int32_t i, int32_t* parent, double* blen, double* anno_dist, int32_t* is_leaf,
		const char** name, const char** anno);
/* children of node i in the order of PTUNode::neighbors (the order their parent -> child edges stand in the file); returns the count */
int hu_tree_info_children(const hu_tree_info* t, int32_t i, const int32_t** children);

/* BandedHMMP7::buildAlignPath (src/BandedHMMP7.cpp:894-941): the CSLoc of a CSFM hit (1-based CS
 * start/end + the gapped CS string, src/CSLoc.h) and the seed's 1-based read range -> the
 * ViterbiAlignPath row {start,end,from,to,nIns,nDel} hu_batch_set_reads takes.  Host only. */
int hu_build_align_path(const hu_db* db, int cs_start, int cs_end, const char* cs, int cs_from, int cs_to, int32_t* out6);

/* ---- host seed lookup -----------------------------------------------------
 * CSFMIndex::locateOne + BandedHMMP7::buildAlignPath as alignSeq uses them (src/HmmUFOtu_main.cpp:50-84), over the same
 * text as the reference's FM-index (the gap-free leaf sequences, src/CSFMIndex.cpp:288-330), indexed here by a position
 * array sorted on the 32 symbols that follow (a depth-32 suffix array) with a 12-base directory.  The hit taken is the
 * FIRST of the suffix-ordered range (the reference's locateFirst, :92-119; its locateOne draws a random member of the same
 * range with rand(), src/CSFMIndex.cpp:139).  seed_len in 12..31 (CLI: 15..25).  Host only. */
typedef struct hu_seed_index hu_seed_index;
int hu_seed_index_create(int32_t n_nodes, int32_t cs_len, const int32_t* parent, const int8_t* seq,
		int32_t K, const int32_t* p2cs, int32_t seed_len, hu_seed_index** out);
/* The same index from the reference's own <DB>.csfm (CSFMIndex::load, src/CSFMIndex.cpp:200-230: libcds BitSequenceRRR +
 * WaveletTreeNoptrs): the sequences are recovered from the BWT, the sampled suffix array and concat2CS, and the seeds are kept in
 * the file's own suffix order, so the first hit of a seed is CSFMIndex::locateFirst's (src/CSFMIndex.cpp:92-119).
 * p2cs / K: the profile's map (hu_db_info / the .hmm), as for hu_seed_index_create. */
int hu_seed_index_load_csfm(const char* path, int32_t K, const int32_t* p2cs, int32_t seed_len, hu_seed_index** out);
void hu_seed_index_destroy(hu_seed_index* ix);
int64_t hu_seed_index_size(const hu_seed_index* ix);          /* distinct seed_len-mers */
int64_t hu_seed_index_bytes(const hu_seed_index* ix, int64_t* positions /* indexed k-mer starts; may be NULL */);   /* resident bytes */
/* every occurrence of one seed in index (suffix) order — the range locateOne draws from: sequence number (leaves in node-id
 * order), residue offset inside it, 0-based CS column of its first base.  Returns the count; at most cap entries are written */
/* CSFMIndex::locateFirst + count for one seed of the index's length: 1-based CS columns of the first hit's first and last base */
int hu_seed_index_locate_first(const hu_seed_index* ix, const char* kmer, int32_t* cs_start, int32_t* cs_end, int64_t* count);
int64_t hu_seed_index_occurrences(const hu_seed_index* ix, const char* kmer, int32_t* seq_no, int32_t* offset, int32_t* cs_col, int64_t cap);
/* Host only, no device: what std::sort (libstdc++: introsort — median-of-3 Hoare partitions down to 16 elements, heap sort past a depth of
 * 2 lg n, one final insertion sort) leaves in the first k places of n PTLocs compared on dist alone, given in node order — the computation
 * behind HU_SEED_ORDER_LIBSTDCXX, exposed for its parity test.  dist must hold no NaN (std::sort is undefined on them).  out_idx [min(k, n)]:
 * indices into dist. */
int hu_sort_prefix_libstdcxx(const double* dist, int64_t n, int64_t k, int32_t* out_idx);
/* The same on the device (k_seed_refsort, the kernel behind HU_SEED_ORDER_LIBSTDCXX), exposed for its parity test: rows x n (d, N) pairs
 * (d << 16 | N, d <= N, N >= 1; pair16 != 0: held as 16-bit pairs, d, N <= 255), one sort per row.  out_idx [rows][k]; out_cnt [rows] =
 * min(k, n), or -1 for a row the kernel left to the host path (heap-sort branch of introsort). */
int hu_sort_prefix_device(int device, const uint32_t* pairs, int rows, int64_t n, int k, int pair16, int32_t* out_idx, int32_t* out_cnt);
/* The same with the root of the test tree at place root_place (0 .. n) of node order instead of behind the last node: the kernel's level 0 is
 * the pair row WITHOUT the root's entry, read in aligned vectors that are one element off from the root on. */
int hu_sort_prefix_device_at(int device, const uint32_t* pairs, int rows, int64_t n, int k, int pair16, int64_t root_place, int32_t* out_idx, int32_t* out_cnt);
/* The device routine behind filterPlacements and the final sort (hu_kern_rank.h), exposed for its parity test: rows x n doubles (n <= HU_MAX_SEEDS),
 * order [rows][n] = for every place the index of the element that std::sort(rbegin, rend, less) — libstdc++'s introsort incl. its heap-sort
 * branch — leaves there (descending; equal keys as the library leaves them). */
int hu_sort_desc_device(int device, const double* keys, int rows, int n, int32_t* order);
/* the 5' and (GLOBAL mode) 3' seed scans for n reads -> vpaths [n][2][6] for hu_batch_set_reads */
int hu_seed_index_lookup(const hu_seed_index* ix, int n, const char* bases, const int64_t* offs, int seed_region,
		int align_mode, int32_t* vpaths);

/* The same with CSFMIndex::locateOne's hit choice (src/CSFMIndex.cpp:121-147; `hmmufotu -S <seed>`): each seed takes a pseudo-random member
 * of its hit range instead of the first.  The reference draws with rand() from ONE global stream, seeded by -S (default: the time) and
 * raced on by its OpenMP tasks, so its own runs only repeat with -p 1; here the draw is a hash of (seed, number of the read
 * in the input = first_read + its index, seed position): the same reads get the same hits whatever the batching or thread count. */
int hu_seed_index_lookup_random(const hu_seed_index* ix, int n, const char* bases, const int64_t* offs, int seed_region,
		int align_mode, uint64_t seed, int64_t first_read, int32_t* vpaths);

/* ---- batch ------------------------------------------------------------------------------ */
int hu_batch_create(hu_db* db, int max_reads, hu_batch** out);
void hu_batch_destroy(hu_batch* b);

/* reads after the host seed lookup (the boundary of SURVEY.md F7): bases are the read
 * characters (upper-case IUPAC; anything PrimarySeq::encodeAt maps to <0 marks the read
 * invalid), vpaths the ViterbiAlignPath {start,end,from,to,nIns,nDel} of the <=2 CSFM seeds
 * (src/HmmUFOtu_main.cpp:52-84, src/BandedHMMP7.cpp:894-941), rows with start==0 unused.
 * mates (already reverse-complemented, src/hmmufotu.cpp:609) may be NULL for SE. */
int hu_batch_set_reads(hu_batch* b, int n, const char* bases, const int64_t* offs, const int32_t* vpaths,
		const char* mates, const int64_t* moffs, const int32_t* mvpaths);
/* alternative entry after alignment: DigitalSeq codes [n][cs_len] and 0-based inclusive
 * regions, as getSeed/estimateSeq/placeSeq receive them (src/hmmufotu.cpp:641-645) */
int hu_batch_set_aligned(hu_batch* b, int n, const int8_t* codes, const int32_t* start, const int32_t* end);

/* alignSeq(hmm, csfm, read, ...) minus the CSFM lookup, + PE merge + DigitalSeq encoding
 * (src/HmmUFOtu_main.cpp:86-104, src/hmmufotu.cpp:621-641) */
int hu_align_batch(hu_batch* b, const hu_opts* o);
/* getSeed + truncation to max_nseed (src/HmmUFOtu_main.cpp:127-152, src/hmmufotu.cpp:645-647);
 * order is (dist, node id) — the reference's std::sort order is unspecified among ties */
int hu_seed_batch(hu_batch* b, const hu_opts* o);
/* the segment form of the seed stage (src/hmmufotu.cpp:662-665, 682, 686): the node ids are GIVEN
 * (ids [n][stride], n_seeds[r] <= HU max_nseed of them used) and only their distance is measured over the
 * batch's current regions — against dist_ids[r][s] when dist_ids is not NULL (the alt-placement PTLoc
 * takes the distance to another node than the branch it names), else against ids[r][s] */
int hu_seed_batch_given(hu_batch* b, const int32_t* n_seeds, const int32_t* ids, const int32_t* dist_ids, int stride);
/* estimateSeq over the seeds (src/HmmUFOtu_main.cpp:154-160, src/PhyloTreeUnrooted.cpp:849-877) */
int hu_estimate_batch(hu_batch* b, const hu_opts* o);
/* filterPlacements (src/HmmUFOtu_main.cpp:162-173) — host, literally std::sort */
int hu_filter_batch(hu_batch* b, const hu_opts* o);
/* placeSeq over the survivors (src/HmmUFOtu_main.cpp:175-180, src/PhyloTreeUnrooted.cpp:879-954) */
int hu_place_batch(hu_batch* b, const hu_opts* o);
/* The candidates of every read GIVEN by the caller instead of produced by hu_filter_batch — for callers that keep the reference's
 * per-stage functions (estimateSeq -> filterPlacements -> placeSeq -> calcQValues on a vector<PTPlacement>, src/HmmUFOtu_main.h:91-107)
 * and may drop, reorder or edit placements between the stages (hmmufotu_amd/csrc/hu_reference_api.hpp does).  offs [n + 1]; recs
 * [offs[n]] in the order the later stages are to see them, at most HU_MAX_SEEDS per read, none for a read that is not HU_READ_OK.
 * Read from a record: c_node (a non-root node), ratio, wnr, est_loglik; with placed != 0 also loglik, height, a_node — records as
 * hu_batch_get_candidate_places returns them — and the batch then counts as placed (hu_finish_batch may follow); with placed == 0 it
 * counts as filtered (hu_place_batch may follow).  The batch must be aligned (hu_align_batch or hu_batch_set_aligned). */
int hu_batch_set_candidates(hu_batch* b, const int64_t* offs, const hu_place_rec* recs, int placed);
/* calcQValues + final sort + bestPlace (src/HmmUFOtu_main.cpp:182-216, src/hmmufotu.cpp:725-733) */
int hu_finish_batch(hu_batch* b, const hu_opts* o);
/* the whole per-read task body for the batch (src/hmmufotu.cpp:621-733) */
int hu_assign_batch(hu_batch* b, const hu_opts* o);

/* ---- chimera check (-C; src/hmmufotu.cpp:653-691) ------------------------------------------
 * hu_chimera_opts mirrors --num-segment / --chimera-err / --chimera-lod (src/hmmufotu.cpp:145-149, 249-256,
 * 325-340): num_seg even in [2,6]; max_chimera_error > 0 (CLI default max_error / num_seg);
 * min_chimera_lod >= 0 */
typedef struct {
	int32_t num_seg;
	int32_t reserved;
	double max_chimera_error;
	double min_chimera_lod;
} hu_chimera_opts;
/* per read: the best 5' and 3' segment placements and the log-odds against each other's branch.
 * checked = 0 (and ids -1, lod NaN) for reads that are not HU_READ_OK, have no seed, or whose region is
 * shorter than num_seg columns — the reference indexes an empty vector there */
typedef struct {
	int32_t checked, is_chimera;
	int32_t seg5_start, seg5_end, seg3_start, seg3_end;   /* 0-based inclusive segment of each winner */
	int32_t n_seg5, n_seg3;                               /* pooled placements per half               */
	hu_place_rec seg5, seg3;                              /* a_node = getTaxonId()                    */
	double alt5_loglik, alt3_loglik;
	double lod;
} hu_chimera_rec;
void hu_default_chimera_opts(const hu_opts* o, hu_chimera_opts* co);
/* b: a batch that is at least seeded (hu_seed_batch done; it is left untouched and can go on to
 * hu_estimate_batch ... for the reads that are not chimeric).  work: a second batch on the same database
 * with max_reads >= b's read count; its contents are overwritten (num_seg + 2 passes of the segment
 * seed/estimate/filter/place stages run in it).  out [n] */
int hu_chimera_batch(hu_batch* b, hu_batch* work, const hu_opts* o, const hu_chimera_opts* co, hu_chimera_rec* out);

/* Kernel-selection / diagnostic knobs of a batch (which Viterbi kernel, node-ordered launches, split placement slots ...;
 * the list with defaults is HuKnobs in hmmufotu_amd/csrc/hu_engine.hip).  A batch reads its defaults from the environment
 * (HU_<NAME>) once, in hu_batch_create; this call changes one of them afterwards.  Results do not depend on any knob
 * beyond the documented tolerances — the parity tests force each alternative kernel through here.  HU_ERR_ARG: no such knob. */
int hu_batch_set_knob(hu_batch* b, const char* name, int value);

/* wait for everything queued on the batch's stream */
int hu_batch_sync(hu_batch* b);

/* ---- results (device -> caller's host buffers; any pointer may be NULL) ----------------- */
int hu_batch_get_alignments(hu_batch* b, hu_align_rec* recs, char* align /* [n][cs_len] */, char* trace, int trace_stride);
int hu_batch_get_codes(hu_batch* b, int8_t* codes /* [n][cs_len] */, int32_t* start, int32_t* end);
int hu_batch_get_pdist(hu_batch* b, int read, int32_t* d /* [n_nodes] */, int32_t* N);
/* n_seeds [n]; ids, d, N: [n][HU_MAX_SEEDS] — every row is written in full (entries past n_seeds[r]: id -1, d = N = 0) */
int hu_batch_get_seeds(hu_batch* b, int32_t* n_seeds, int32_t* ids, int32_t* d, int32_t* N);
/* ratio, wnr, loglik: [n][HU_MAX_SEEDS], NaN past the read's seed count */
int hu_batch_get_estimates(hu_batch* b, double* ratio, double* wnr, double* loglik);
/* the same with a caller-chosen row stride (>= 1): min(stride, HU_MAX_SEEDS) entries are written per read, nothing beyond;
 * for callers that size their buffers [n][max_nseed] */
int hu_batch_get_seeds_strided(hu_batch* b, int32_t* n_seeds, int32_t* ids, int32_t* d, int32_t* N, int stride);
int hu_batch_get_estimates_strided(hu_batch* b, double* ratio, double* wnr, double* loglik, int stride);
/* all candidates after placement, in filterPlacements order: offs [n+1]; arrays sized offs[n] */
int hu_batch_get_candidates(hu_batch* b, int64_t* offs, int32_t* c_node, double* ratio, double* wnr, double* est_loglik, int32_t* iters);
int hu_batch_get_placements(hu_batch* b, hu_place_rec* best /* [n] */);
/* every candidate's PTPlacement after hu_finish_batch, in filterPlacements order (offs as above) */
int hu_batch_get_candidate_places(hu_batch* b, hu_place_rec* recs /* [offs[n]] */);

/* One TSV line per read exactly as the main loop prints it (src/hmmufotu.cpp:736-739: id, description,
 * HmmAlignment operator<< src/BandedHMMP7.cpp:1215-1221, PTPlacement::write
 * src/PhyloTreeUnrooted.h:1611-1617; doubles at the default 6-significant-digit ostream precision).
 * ids/descs: n C strings; annos: taxon annotation per NODE (may be NULL -> empty column).  Reads whose
 * status is not HU_READ_OK produce no line, like the reference.  Writes into buf (capacity cap) and
 * returns the number of bytes needed (call again with a larger buffer if > cap). */
int64_t hu_batch_format_tsv(hu_batch* b, const char* const* ids, const char* const* descs, const char* const* annos,
		char* buf, int64_t cap);
/* the same with -C: which = 0 writes the assignment file's lines (HU_READ_OK reads the check did not flag), which = 1 the
 * --chimera-out lines (bad PE orientation, or flagged; placement columns of a default PTPlacement, src/hmmufotu.cpp:693-706).
 * which = 2 is the assignment file of --align-only: as 0 for a batch that is only aligned, default placement columns.
 * chimera_info != 0 inserts the --chimera-info columns before the placement (src/hmmufotu.cpp:57, 742-746).  chi [n] from
 * hu_chimera_batch (NULL: nothing was checked) */
int64_t hu_batch_format_tsv_chimera(hu_batch* b, const char* const* ids, const char* const* descs, const char* const* annos,
		const hu_chimera_rec* chi, int chimera_info, int which, char* buf, int64_t cap);
/* the same without a copy: *text points at the batch's own buffer holding the lines (valid until the next format call on this
 * batch); returns their length.  One pass — the (buf, cap) forms above format once per call, so "ask for the size, then fetch" costs
 * two.  The lines of a batch are formatted on the host thread pool of the calling thread. */
int64_t hu_batch_format_tsv_ptr(hu_batch* b, const char* const* ids, const char* const* descs, const char* const* annos,
		const hu_chimera_rec* chi, int chimera_info, int which, const char** text);
/* the bytes each read's line takes in the text of the LAST format call on this batch, newline included (0: the read has no line there): lens [n].
 * For callers that reassemble lines from several batches in read order (the column-window mode of the CLI) */
int hu_batch_tsv_line_lengths(hu_batch* b, int64_t* lens);
/* header with the --chimera-info columns (src/hmmufotu.cpp:592-594 with CHIMERA_TSV_HEADER) */
const char* hu_tsv_header_chimera(void);
/* the header line of the assignment file (src/hmmufotu.cpp:592-594) */
const char* hu_tsv_header(void);

/* ---- column-window sharding (last row) -------------------------------
 * PTUnrooted::load keeps the messages of EVERY column of every directed edge in one address space (src/PhyloTreeUnrooted.cpp:496-535); a database whose
 * messages exceed one GPU's HBM (72 bytes per node and column once packed: 28.8 MB per column at 399,999 nodes) is held as W column WINDOWS instead,
 * one hu_db per window (hu_db_load_window, or hu_tree_desc.win_*), usually one per device.  A read's placement touches only the columns of its
 * alignment region, so it runs unchanged on any window that holds the region; the seed scan runs on the node sequences, which every window holds whole.
 * Reads are ROUTED by where their seeds say they lie, before the alignment; a read that comes back HU_READ_OUT_OF_WINDOW (aligned, region known
 * exactly, not placed) is routed once more by its region.  No window exchanges anything with another: still no data-path collective.
 *   hu_windows_plan      W windows of equal width that cover [0, cs_len) and overlap their neighbours by `overlap` columns (choose it >= the widest
 *                        alignment region to be expected, so that every region lies inside at least one window)
 *   hu_route_by_seeds    per read the window to try first: the CS interval the read is expected to cover — from the profile positions of its
 *                        seed paths (vpaths [n][2][6] as for hu_batch_set_reads), extended by the bases left and right of the seeds; the window
 *                        that contains it with the widest margin, else the one that overlaps it most.  A read without a seed goes to window 0.
 *                        lens [n]: bases of each read (of the merged pair: pass the forward read's and the mate's through lens / mate_lens)
 *   hu_route_by_region   the same from exact 1-based inclusive CS regions (hu_align_rec.cs_start / cs_end); -1 when no window contains the region */
typedef struct { int64_t win_start, win_len; } hu_window;
int hu_windows_plan(int64_t cs_len, int n_win, int64_t overlap, hu_window* out /* [n_win] */);
int hu_route_by_seeds(const hu_db* db, int n_win, const hu_window* win, int n, const int32_t* lens, const int32_t* vpaths,
		const int32_t* mate_lens, const int32_t* mate_vpaths, int32_t* window_of_read /* [n] */);
int hu_route_by_region(int n_win, const hu_window* win, int n, const int32_t* cs_start, const int32_t* cs_end, int32_t* window_of_read /* [n] */);

/* ---- measurement ------------------------------------------------------------------------
 * per-kernel device time of the LAST call of each stage, measured with HIP events on the
 * batch's stream: ms[HU_T_*]; and the algorithmic work it covered */
enum { HU_T_VITERBI = 0, HU_T_ALIGN_BUILD = 1, HU_T_SEED_PDIST = 2, HU_T_SEED_TOPK = 3,
	HU_T_ESTIMATE = 4, HU_T_PLACE = 5, HU_T_COUNT = 8 };
int hu_batch_timings(hu_batch* b, float* ms /* [HU_T_COUNT] */);
/* enable/disable event recording around kernels (off by default: zero overhead) */
int hu_batch_profile(hu_batch* b, int enable);
/* host wall-clock (ms) of the last hu_assign_batch: align | seed+estimate+filter | place | finish */
int hu_batch_wall(hu_batch* b, double* ms4);
/* the last hu_seed_batch under HU_SEED_ORDER_LIBSTDCXX: reads the device sort (k_seed_refsort) handed to the host restatement (heap-sort branch, table
 * overflow; the NaN-distance reads of a database with partial sequences are counted too), and whether the WHOLE batch took the host path (a tree beyond
 * the kernel's LDS index, ~9 M nodes: said once on stderr) — so that a rate quoted for the mode is never silently a host-path rate */
int hu_batch_refsort_stats(hu_batch* b, int32_t* left_to_host, int32_t* whole_batch_on_host);

/* ---- primer coverage (hmmufotu-anneal) --------------------------------------------------
 * The node scan of src/hmmufotu-anneal.cpp:246-290: for each primer, the nodes (all of them, the root included) whose sequence is within
 * max_dist of the primer's alignment, SeqUtils::pDist(aln.align, node seq, csStart - 1, csEnd - 1) (src/SeqUtils.cpp:77-85): the share
 * of the region's columns, gaps included, where DegenAlphabet::isMatch(align char, node code) fails.  Among them the leaves, nodes with
 * one neighbour (a root with a single child is one).
 * Runs on a batch that hu_align_batch has aligned: the caller aligns each primer (GLOBAL mode, no vpaths: alignSeq(hmm, read),
 * src/HmmUFOtu_main.cpp:107-125), and for the reverse strand its reverse complement as another row, and chooses the strand on the host
 * from the rows' costs (the reverse one only when its cost is strictly lower, :253-265).  row_of_primer[i] is the chosen row of primer i;
 * a negative row skips the primer (both outputs -1).  as_read (may be NULL) gives per primer the text of its chosen row in the case the
 * primer was read (for the reverse row: reversed and complemented case by case, IUPACNucl::getComplementSymbol); the row's bases must
 * be that text upper-cased.  The reference writes a matched base into the alignment as read, so a lower-case one is an invalid symbol
 * there: the batch's rows take the text's case before the scan, and hu_batch_get_alignments returns them so afterwards.
 * HU_ERR_ARG: a row that is not an aligned row of the batch, a text that is not its bases, max_dist < 0, or a database that keeps a
 * column window (hu_db_load_window). */
int hu_anneal_batch(hu_batch* b, const int32_t* row_of_primer, int n, const char* const* as_read, double max_dist, int64_t* hit_nodes, int64_t* hit_leaves);
/* the hit threshold of a region of len columns: the largest d with (double) d / len <= max_dist, -1 if none */
int64_t hu_anneal_max_mismatch(double max_dist, int32_t len);
/* the match rule per alignment byte: bit 0..3 = node code 0..3 (A C G T), bit 4 = node code -2 (gap), bit 5 = node code -1 */
int hu_anneal_match_table(uint8_t* out /* [256] */);
/* ANNEAL_HEADER of src/hmmufotu-anneal.cpp:52: the first line of an anneal report */
const char* hu_anneal_header(void);
/* PTUnrooted::numLeaves: nodes with one neighbour (src/PhyloTreeUnrooted.h:199) */
int hu_db_num_leaves(const hu_db* db, int64_t* n_leaves);

/* ---- OTU consensus sequences (hmmufotu-sum -c) ---------------------------
 * What src/hmmufotu-sum.cpp:383-397 and :437-457 do with the accepted records of assignment files: per OTU (the node of a record's
 * taxon_id) the column counts of its reads' alignments, then one consensus sequence per OTU from those counts and the node's message
 * as a Dirichlet prior (PTUnrooted::inferPostCS, src/PhyloTreeUnrooted.cpp:1111-1125).  The counts stay on the device.  A handle is
 * bound to a loaded database; several handles (and batches) may share one.  Calls on one handle are not concurrent.
 * hu_otucs_create: HU_ERR_ARG for a database that keeps a column window (hu_db_load_window), and for one whose stored root is not
 * node 0: the reference re-roots at node 0 first (ptu.setRoot(0), src/hmmufotu-sum.cpp:337), recomputing that node's message from its
 * children, which is not provided; hmmufotu-build stores root 0. */
typedef struct hu_otucs hu_otucs;
int hu_otucs_create(hu_db* db, hu_otucs** out);
void hu_otucs_free(hu_otucs* h);
/* the loop of src/hmmufotu-sum.cpp:391-397 for n_rows accepted records: rows [n_rows][cs_len] bytes, the records' alignment strings as
 * read; node_of_row [n_rows] their taxon_id.  Byte c of column j adds 1 to freq(b, j) of the row's OTU when b = encode(toupper(c)) of
 * IUPACNucl (hu_msa_encode_table) is a residue, else to gap(j): gap symbols and every invalid byte alike.  May be called any number of
 * times; the counts equal those of one call with all rows.  HU_ERR_ARG, before anything reaches the device, for a node outside
 * [0, n_nodes); a failed call changes nothing. */
int hu_otucs_add(hu_otucs* h, int64_t n_rows, const int32_t* node_of_row, const char* rows);
/* the counts of one OTU: freq [4][cs_len] (A C G T), gap [cs_len]; all zero for a node no row has named */
int hu_otucs_counts(hu_otucs* h, int32_t node, uint32_t* freq, uint32_t* gap);
/* PTUnrooted::inferPostCS(node, freq, gap, effN) for n OTUs: out [n][cs_len] characters of ACGT and '-', no terminator.  Per column:
 * pri = the node's message towards its parent (for node 0 the root message of the .ptu) as weights summing to 1 (inferWeight,
 * src/PhyloTreeUnrooted.h:1590-1593), post = eff_n * pri + freq, post /= sum(post), and the symbol is '-' when sum(freq) < gap, else
 * the first maximum of post.  eff_n = 0 turns the prior off.  HU_ERR_ARG for a node outside [0, n_nodes) or eff_n < 0. */
int hu_otucs_infer(hu_otucs* h, int32_t n, const int32_t* nodes, double eff_n, char* out);
/* host only: the description of an OTU's FASTA record (src/hmmufotu-sum.cpp:448-452),
 *   DBName=<db_name>;Taxonomy="<taxonomy>";AnnoDist=<anno_dist>;ReadCount=<read_count>;SampleHits=<sample_hits>
 * anno_dist as boost::lexical_cast<string>(double) writes it: 17 significant digits in ostream's general format, i.e. %.17g.  Returns
 * the length (without the terminator) and writes at most cap bytes, terminator included; HU_ERR_ARG (negative) on a null argument. */
int64_t hu_otucs_description(const char* db_name, const char* taxonomy, double anno_dist, int64_t read_count, int64_t sample_hits, char* out, int64_t cap);
/* the annotation distance of a node (PTUNode::getAnnoDist), beside hu_db_get_annotation */
int hu_db_get_anno_dist(const hu_db* db, int32_t node, double* out);

/* ---- the summary of a run from its own batches (hmmufotu-amd --otu-table / --otu-cs) ----------------
 * What hmmufotu-amd-sum and hmmufotu-amd-otu-cs would read back from the batch's assignment lines, without the lines.
 * hu_batch_get_summary, for a finished batch of reads (hu_finish_batch done; HU_ERR_STATE otherwise): per read
 *   in_main       1 when the read's line stands in the main assignment output (hu_batch_format_tsv_chimera, which = 0, with the same chi:
 *                 HU_READ_OK and not flagged as a chimera), else 0
 *   taxon         the line's taxon_id column: a_node of the best placement, -1 when the read has none
 *   q_taxon       Q_taxon of the best placement as the engine holds it (NaN when the read has none)
 *   n_cols        CS_end - CS_start + 1
 *   n_sym         bytes of the columns CS_start - 1 .. CS_end - 1 of the read's alignment row that are symbols (upper-case IUPAC codes)
 *   n_match       those of the columns that are match columns of the profile
 *   n_match_sym   the bytes that are both
 * The four integers are counted on the device, where the rows are (no row crosses to the host), and are 0 for a read that is not
 * HU_READ_OK.  chi [n] from hu_chimera_batch, or NULL. */
typedef struct {
	int32_t in_main, taxon;
	double q_taxon;
	int32_t n_cols, n_sym, n_match, n_match_sym;
} hu_sum_rec;
int hu_batch_get_summary(hu_batch* b, const hu_chimera_rec* chi, hu_sum_rec* out /* [n] */);
/* host only: accept[i] = 1 when record i is "a valid assignment" for hmmufotu-amd-sum reading the read's line (hu_tsv::accepted), else 0:
 * in_main, taxon >= 0, Q_taxon >= min_q where Q_taxon is q_taxon through the line's six significant digits and back, and, each unless
 * its threshold is 0, n_sym / n_cols >= min_aln and n_match_sym / n_match >= min_hmm (0 / 0 rejects). */
int hu_sum_accept(const hu_sum_rec* recs, int n, double min_q, double min_aln, double min_hmm, uint8_t* accept /* [n] */);
/* hu_otucs_add for the reads i of a finished batch with accept[i] != 0, each under the taxon of its best placement; the rows are read
 * where they lie on the device.  The call waits for the batch's stream first and returns when the batch may be reused.  HU_ERR_STATE: the
 * batch is not finished; HU_ERR_ARG: the batch is of another database than the handle, or an accepted read has no alignment or no
 * taxon.  A failed call changes nothing. */
int hu_otucs_add_batch(hu_otucs* h, hu_batch* b, const uint8_t* accept /* [n] */);
/* the inverse of hu_otucs_counts: freq [4][cs_len] and gap [cs_len] are added to the counts of the OTU `node` (merging the handles of
 * several replicas).  HU_ERR_ARG for a node outside [0, n_nodes). */
int hu_otucs_add_counts(hu_otucs* h, int32_t node, const uint32_t* freq, const uint32_t* gap);

/* ---- the seed index file <DB>.csfm (hmmufotu-build's csfm.build(msa) + csfm.save) -------------------------------
 * hu_suffix_array: what divsufsort(concatSeq, SA, N) returns in CSFMIndex::buildBWT (src/CSFMIndex.cpp:327-335), built on the device by
 * prefix doubling over a radix sort.  text: n bytes of 0 (separator, terminator) and 1..4 (bases), 1 <= n < 2^31; sa [n]: the start
 * positions of the suffixes in ascending order, a suffix that is a proper prefix of another first.  rounds (may be NULL): doubling rounds
 * taken; device_seconds (may be NULL): time on the device without the copies.  HU_ERR_ARG for n out of range (before the text is read)
 * or a symbol above 4, both before a device is asked for; HU_ERR_NOMEM with the bytes needed and the bytes free when the device cannot
 * hold the sort (about 29.3 bytes per symbol).  hu_suffix_array_tile: the pairs one wave sorts per pass, for tests of the tile edges. */
int hu_suffix_array(int device, const uint8_t* text, int64_t n, int32_t* sa, int32_t* rounds, double* device_seconds);
int32_t hu_suffix_array_tile(void);
/* CSFMIndex::save (src/CSFMIndex.cpp:176-198) of the index CSFMIndex::build makes (buildBasic, buildConcatSeq, buildBWT, :275-368), behind
 * the 20-byte head saveProgInfo puts in front of it (src/hmmufotu-build.cpp:479-480).  rows: n_seq rows of cs_len bytes, row-major, as read
 * (case kept): the pruned alignment, ALL its rows in file order.  A byte is a gap or a residue by hu_msa_encode_table, a residue's symbol is
 * encode(toupper(c)) + 1; any other byte is refused with its row and column (HU_ERR_ARG; the reference refuses such an alignment when it
 * loads it).  cs_seq: the cs_len characters of MSA::calculateCS, zero-terminated (the file's leading blank is added here); cs_identity
 * [cs_len]: MSA::identityAt of every column (the file's leading 0 is added here).
 * hu_csfm_encode: host only, from a GIVEN suffix array sa [N] of the concatenated text, N = residues + n_seq + 1 (HU_ERR_ARG when it is no
 * permutation of 0 .. N - 1; its order is not checked).  hu_csfm_write: the suffix array, the BWT, the marks of the sampled rows and the
 * sampled values come from the device (hu_suffix_array's construction); the file is encoded and written on up to 16 host threads.
 * Both refuse cs_len > 65535 and N >= 2^31 before anything is allocated.  hu_csfm_write_timing: of this thread's last hu_csfm_write,
 * seconds [4] = text, device (with copies), encode + write, suffix array alone; rounds = doubling rounds. */
int hu_csfm_encode(const char* path, int64_t n_seq, int64_t cs_len, const char* rows, const char* cs_seq, const double* cs_identity, const int32_t* sa);
int hu_csfm_write(const char* path, int64_t n_seq, int64_t cs_len, const char* rows, const char* cs_seq, const double* cs_identity, int device);
int hu_csfm_write_timing(double* seconds /* [4] */, int32_t* rounds);

/* ---- training a substitution model (hmmufotu-train-sm) -------------------------------------------------------
 * model->trainParams(tree.getModelTransitionSet(method), tree.getModelFreqEst()) of src/hmmufotu-train-sm.cpp:232-233 in four steps:
 * which rows are compared (host), the counts over their columns (device), the closed-form trainers (host), the model file (host).
 *
 * hu_sm_training_set: PTUnrooted::getModelTraningSetGojobori / getModelTraningSetGoldman (src/PhyloTreeUnrooted.cpp:449-486) up to the
 * point where sequences are read, on the arrays of hu_newick_get; row_of [n]: the MSA row of every leaf, -1 for the other nodes.  A
 * node's neighbour list is "parent, then children in file order"; isLeaf / isTip / firstChild / lastChild are those of
 * src/PhyloTreeUnrooted.h:199-267 (a leaf has ONE neighbour, so a root with a single child is one).  Nodes are visited in id order.
 *   HU_SM_GOJOBORI: a node with exactly two children, one of them a tip, gives (row0, row1, row2) = (randomLeaf(the other child), the
 *     tip's first child, its last child).  randomLeaf (src/PhyloTreeUnrooted.h:1480-1486) steps to children[rand() % size] until a
 *     leaf: rand() is the C library's and is never seeded here, so an unseeded process draws what the reference's program draws.
 *   HU_SM_GOLDMAN: a tip with more than two neighbours gives (-1, first child's row, last child's row).
 * Every candidate is returned; whether it is used is decided from the distances hu_sm_counts measures (hu_sm_item_pass).
 * items: [n_nodes][3] int32 of room; *n_items: how many were written.  No counting, no device. */
enum { HU_SM_GOJOBORI = 0, HU_SM_GOLDMAN = 1 };
int hu_sm_training_set(int32_t n_nodes, const int32_t* parent, const int32_t* child_off, const int32_t* child_idx, const int32_t* row_of,
		int method, int32_t* items, int64_t* n_items);
/* The column loops, on the device (k_sm_counts, one workgroup per item and per row).  rows [n_rows][cs_len]: codes as hu_msa_encode_table
 * gives them (0..3 residue, negative: gap or invalid).  items [n_items][3] as above, rows checked against n_rows before a device is
 * asked for.  Outputs, all host, all integer and therefore exact:
 *   counts [n_items][16], row-major from, to.  A triple is DNASubModel::calcTransFreq3Seq(row0, row1, row2) (src/DNASubModel.cpp:75-104):
 *     per column with three residues the ancestor is b0 if b0 == b1 or b0 == b2, else b1 if b1 == b2, else the column is skipped; one
 *     is added to (anc, b0), (anc, b1), (anc, b2).  A pair is calcTransFreq2Seq(row1, row2) (:52-62).
 *   dn [n_items][4]: d, N of SeqUtils::pDist (src/SeqUtils.cpp:37-54; N = columns where both are residues, d = those that differ) for
 *     (row0, row1) and (row0, row2); for a pair for (row1, row1) — the reference's Goldman test compares the row with itself — and
 *     (row1, row2).
 *   base [n_rows][4]: DNASubModel::calcBaseFreq of every row (:106-112).
 * n_items may be 0.  HU_ERR_NOMEM with the bytes needed and the bytes free when the device cannot hold the rows (each padded to a
 * multiple of 16 bytes) and the outputs.  hu_sm_counts_timing: of this thread's last call, seconds [3] = allocation and copies to
 * the device, the kernel, the copies back. */
int hu_sm_counts(int device, int64_t n_rows, int64_t cs_len, const int8_t* rows, int64_t n_items, const int32_t* items,
		int32_t* counts, int32_t* dn, int32_t* base);
int hu_sm_counts_timing(double* seconds /* [3] */);
/* pass [n_items]: SeqUtils::pDist(...) <= DNASubModel::MAX_PDIST (0.15, src/DNASubModel.cpp:39) as the two training-set loops apply
 * it: (double) d / N, both distances of a triple, the first of a pair; N == 0 gives NaN, which fails. */
int hu_sm_item_pass(int64_t n_items, const int32_t* items, const int32_t* dn, int32_t* pass);
/* trainParams of the six models (src/GTR.cpp:92-122, src/TN93.cpp:88-102, src/HKY85.cpp:86-98, src/F81.cpp:84-89, src/K80.cpp:81-89,
 * src/JC69.h:79-80).  mats [n_items][16] row-major in item order, of which those with pass != 0 are the reference's vector; base [4]:
 * getModelFreqEst (src/PhyloTreeUnrooted.cpp:488-494), the base counts summed over the leaf rows.  Fills type, pi and par of *out
 * (dg_k = 0).  GTR: constrainedQfromP (src/DNASubModel.cpp:147-164) of every matrix, those that pass isValidRate
 * (src/DNASubModel.h:200-206) scaled by minus their TRACE (scale's default pi = Ones, src/DNASubModel.cpp:123-126) and averaged, then
 * R(i, j) = Q(i, j) / pi(j), symmetrised.  n_used (may be NULL): the matrices that entered — for GTR the valid ones.
 * Where the reference would print NaN this entry refuses with HU_ERR_ARG and says so: no valid matrix (GTR), Tv == 0 (TN93, HKY85,
 * K80), base counts that sum to 0 (every model with a pi). */
int hu_sm_train(int type, int64_t n_items, const double* mats, const int32_t* pass, const int64_t* base, hu_model_desc* out, int64_t* n_used);
/* DNASubModel::write of the model (src/GTR.cpp:83-90 and friends): the lines of the model block hu_ptu_write generates, every number as
 * %.17g, so hu_model_parse_text returns pi and par bit for bit; GTR's "Q:" lines hold setQfromParams' matrix scaled by minus its
 * trace, as the reference computes it (both readers skip them).  Returns the length without the terminator and writes at most cap
 * bytes, terminator included; negative on a bad argument. */
int64_t hu_sm_write_text(const hu_model_desc* model, char* buf, int64_t cap);

/* ---- simulated reads with a known answer (hmmufotu-sim) --------------------------------------------------------
 * The loop of src/hmmufotu-sim.cpp:351-424 in three steps: which branch, branch point and columns every read takes (host), the
 * sites of all reads (device), the description of a record (host).  Random numbers are Philox4x32-10 words keyed by the seed,
 * key = (seed & 0xffffffff, seed >> 32); a uniform of [0, 1) is ((hi >> 5) * 2^26 + (lo >> 6)) * 2^-53 of two words.  The reference
 * draws from Boost's mt11213b: the distributions are the reference's, the streams are not.
 *
 * hu_sim_philox: out [4] = Philox4x32-10(counter [4], key [2]), the code host and device share; for known-answer tests. */
int hu_sim_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out);
/* The options of the rejection loop: -d, -m, -s, -l, -u and the (start, end) pairs of the -R BED file as read (columns 2 and 3). */
typedef struct {
	double max_dist;            /* a read's point is at most this far above a leaf; +inf: anywhere */
	double mean_size, sd_size;  /* amplicon size ~ normal(mean, sd) */
	double min_size, max_size;  /* clamps; max_size 0: none */
	int64_t n_regions;          /* 0: reads start anywhere on the consensus */
	const int32_t* regions;     /* [n_regions][2] */
} hu_sim_opts;
void hu_sim_default_opts(hu_sim_opts* o);     /* src/hmmufotu-sim.cpp:56-60: inf, 500, 30, 0, 0; no regions */
/* whether a BED line (s, e) gives a region: 0 <= s < e < cs_len.  The reference (:303) also takes e == cs_len and then reads one
 * column past the alignment; here that line is dropped like the others outside the consensus. */
int hu_sim_region_ok(int32_t s, int32_t e, int32_t cs_len);
/* The rejection loop of src/hmmufotu-sim.cpp:351-380 for n reads, on the arrays of hu_db_get_tree (or of any tree: no device).
 * A node is drawn uniformly among those with height <= max_dist (node_dist, :337-344) and the branch point rc uniformly in [0, 1);
 * the attempt is dropped when the node is the root, when height[c] + blen[c] * rc > max_dist, or when end >= cs_len.  Without
 * regions start is uniform on [0, cs_len - 1], len = (int) normal(mean, sd) (Box-Muller), raised to (int) min_size, cut to
 * (int) max_size when that is above 0, and end = start + len: len + 1 columns, as the reference's inclusive loop walks them.  With
 * regions a uniformly chosen accepted line (s, e) gives start = s + 1, end = e (the reference's own off-by-one), and when no line is
 * accepted the reads start anywhere, as in the reference.  One deviation: a negative len (end < start, an empty record in the
 * reference) is dropped too.
 * Attempt number a draws from the counters (b, a & 0xffffffff, a >> 32, 1): block b = 0 gives the node (words 0, 1) and rc (2, 3),
 * b = 1 the start or the region (0, 1), b = 2 the two uniforms of the normal.  *attempt: in, the first attempt number (0 for a new
 * plan); out, the next one: a plan made in pieces is the plan made at once, so it depends on (seed, options) alone.
 * HU_ERR_ARG: sizes the reference's option checks refuse, no node below the root within max_dist, min_size >= cs_len without
 * regions, or ten million attempts in a row without a read. */
int hu_sim_plan(int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const double* height, const hu_sim_opts* o,
		uint64_t seed, int64_t* attempt, int64_t n, int32_t* node, double* rc, int32_t* start, int32_t* end);
/* MSA::gapWFrac(j) = gapWCount(j) / (resWCount.col(j).sum() + gapWCount(j)) (src/MSA.cpp:71-75) of every column, from hu_msa_stats on
 * the database's device; the four weighted residue counts are summed as (A + G) + (C + T).  gap_frac: [cs_len].
 * msa: n_seq rows of msa_len bytes as read, restricted to the columns MSA::prune keeps (at least one residue); their number must be
 * the database's cs_len (HU_ERR_ARG otherwise).  msa == NULL: the database's own leaf rows (nodes with one neighbour) in node-id
 * order, rewritten as text (a residue as its letter, any other code as '-'), every column kept: a column without a residue, which
 * only a database made from arrays can have, gets the fraction 1.  A .ptu keeps the leaf rows of the .msa it was built
 * with, so the second form differs from the reference's <DB>.msa only in the order of the rows, i.e. in the order the weighted
 * counts are summed. */
int hu_sim_gap_frac(const hu_db* db, int64_t n_seq, int64_t msa_len, const char* msa, double* gap_frac);
/* The per-site loop of src/hmmufotu-sim.cpp:393-409 for n reads at once (k_sim_reads, one workgroup per read).  Read r lies on the
 * branch above node[r], blen * rc[r] above the node, and covers the columns start[r] .. end[r].  At column j
 *   w = Philox(counter (j, g & 0xffffffff, g >> 32, 0)), g = read0 + r;   u_gap from words 0, 1;   u_base from words 2, 3;
 *   a gap when u_gap <= gap_frac[j] (:394); else q = exp(rLoglik - max) of :401-405, computed from the packed messages as
 *   q_i = max((Pr(v rc) msg(c -> p))_i (Pr(v (1 - rc)) msg(p -> c))_i, 0) with the plain model's Pr (no discrete-Gamma rates, as in
 *   the reference), S = q0 + q1 + q2 + q3 summed in that order, t = u_base * S, and the base is the first i with
 *   t < q0 + ... + q_i, else 3.
 * Outputs (host).  off[r] = the columns of the reads before r.  aligned: at off[r] the end - start + 1 characters "ACGT-" of the
 * read; seq: at off[r] the same without '-', seq_len[r] of them, the rest of the read's room zeroed; mate (want_mate != 0, else
 * ignored): likewise the reverse complement of seq.  Each needs the sum of all reads' columns in bytes.
 * The same (seed, read0 + r) gives the same read in any call.  hu_sim_timing: of this thread's last call, seconds [3] = allocation
 * and copies to the device, the kernel, the copies back.
 * HU_ERR_ARG, with the outputs untouched and before anything reaches the device: a node outside [0, n_nodes) or the root, columns
 * that are not 0 <= start <= end < cs_len, an rc outside [0, 1], a database that keeps a column window (hu_db_load_window). */
int hu_sim_reads(const hu_db* db, int64_t n, const int32_t* node, const double* rc, const int32_t* start, const int32_t* end,
		const double* gap_frac, uint64_t seed, uint64_t read0, int want_mate, char* aligned, char* seq, char* mate, int32_t* seq_len);
int hu_sim_timing(double* seconds /* [3] */);
/* host only: the description of a read's FASTA record (src/hmmufotu-sim.cpp:384-386, 413-416),
 *   branchID=<c>-><p>;taxonID=<id>;taxonName="<name>";branchPoint=<rc>;csStart=<start>;csEnd=<end>;seqLen=<seq_len>;
 * id and name are those of c when rc <= 0.5, else of p; taxon_c / taxon_p: PTUNode::getTaxon() of the two nodes, which is
 * hu_db_get_annotation (with ";Other" appended when hu_db_get_anno_dist is NaN: getTaxon's maxDist is inf).  rc as
 * boost::lexical_cast<string>(double) writes it, %.17g.  seq_len: the length of the record's sequence before -r cuts it.  Returns the
 * length (without the terminator) and writes at most cap bytes, terminator included; HU_ERR_ARG (negative) on a null argument. */
int64_t hu_sim_description(int32_t c, int32_t p, const char* taxon_c, const char* taxon_p, double rc, int32_t start, int32_t end, int64_t seq_len,
		char* out, int64_t cap);

/* ---- training the profile HMM (hmmufotu-train-hmm) --------------------------------------------------------------
 * BandedHMMP7::build (src/BandedHMMP7.cpp:386-541) in five steps: the prior file (host), which columns are match columns (host),
 * the weighted counts over all cells (device), the effective sequence number and the probabilities (host), the file (host).
 * All arrays are row-major; E_M / E_I are [K + 1][4] (row 0 of E_M: COMPO), T is [K + 1][3][3] indexed (from, to) with M = 0, I = 1,
 * D = 2 (p7_state, src/BandedHMMP7.h:157).
 *
 * hu_hmm_prior_read: operator>> of BandedHMMP7Prior (src/BandedHMMP7Prior.cpp:39-62) with DirichletMixture::read
 * (src/math/DirichletMixture.cpp:254-285) and DirichletDensity::read (src/math/DirichletDensity.cpp:135-162): five blocks, each a
 * head line ("Match emission:", "Insert emission:", "Match transition:", "Insert transition:", "Delete transition:") followed by a
 * model.  Stricter than the reference, which reads whatever sscanf and operator>> leave: every label line must be there, every
 * number must parse and be finite, alpha > 0, q >= 0, the five blocks must all be present with dimensions 4 (L components, 1 <= L <=
 * HU_HMM_MAX_MIX) / 4 / 3 / 2 / 2.  HU_ERR_IO with the block and the reason otherwise. */
#define HU_HMM_MAX_MIX 32
typedef struct {
	int32_t me_L, pad0;                        /* components of the match-emission mixture */
	double me_q[HU_HMM_MAX_MIX];               /* mixture coefficients */
	double me_alpha[4][HU_HMM_MAX_MIX];        /* alpha(i, j): residue i, component j, as the file lays it out */
	double ie_alpha[4], mt_alpha[3], it_alpha[2], dt_alpha[2];
} hu_hmm_prior;
int hu_hmm_prior_read(const char* path, hu_hmm_prior* out);
/* The match columns (src/BandedHMMP7.cpp:405-411, :517-530), host only, from the weighted counts of hu_msa_stats restricted to the
 * pruned columns: res_wcount [4][cs_len], gap_wcount [cs_len].  Column j is a match column when MSA::symWFrac(j) >= symfrac
 * (src/MSA.cpp:77-81), numRes / (numRes + gapWCount) with numRes = (A + G) + (C + T); a column without weight (NaN) is none.
 * Outputs: mask [cs_len] (1 = match); *K; for k = 1 .. K at index k - 1: map (the 1-based column, the MAP tag), cons (MSA::CSBaseAt,
 * the first maximum of the weighted counts, lower-case when wIdentityAt < CONS_THRESHOLD = 0.9) and identity (MSA::wIdentityAt,
 * :65-67, the maximum / n_seq); each has cs_len entries of room.  HU_ERR_ARG: symfrac outside the open interval (0, 1) as build()
 * throws (:390-391), more than 65,535 columns (kMaxCS, src/BandedHMMP7.h:279: the reference's index arrays end there), or K = 0. */
int hu_hmm_match_columns(int64_t cs_len, int64_t n_seq, const double* res_wcount, const double* gap_wcount, double symfrac,
		uint8_t* mask, int32_t* K, int32_t* map, char* cons, double* identity);
/* The counting loops of src/BandedHMMP7.cpp:424-477 on the device (k_hmm_states, k_hmm_counts: hu_kern_hmm.h).  msa: n_seq rows of
 * cs_len bytes, the pruned text as read; weight / start / end [n_seq]: seq_weight, start and end of hu_msa_stats, the columns
 * renumbered after the prune; mask [cs_len] and K of hu_hmm_match_columns.  Outputs, host, raw weighted counts: e_m, e_i [K + 1][4],
 * t [K + 1][9].  Per cell (i, j) with state sm (determineMatchingState, src/BandedHMMP7.h:713-716; a byte is a residue when
 * hu_msa_encode_table gives >= 0) and k = the match columns at or before j: M adds w to e_m(k, b) and to COMPO, I to e_i(k, b), and
 * t(k)(sm, smN) gets w where smN is the state of the nearest non-P cell right of j on the row, if there is one and the pair is
 * neither I->D nor D->I (the reference reads an unassigned variable there).  Then every row adds w to
 * t(0)(M, state at start) and to t(K)(state at end, M); a row with start < 0 (no residue) adds nothing anywhere.
 * Every column has its own sums in ascending i; the host adds the columns of one k up in ascending j.  Needs 2 n_seq cs_len bytes of
 * device memory: HU_ERR_NOMEM with the bytes needed and the bytes free.  HU_ERR_ARG, before a device is asked for: cs_len above
 * 65,535, a mask that does not hold K match columns, a weight that is negative or not finite, a start / end outside the row or on a
 * byte that is no residue.  hu_hmm_counts_timing: of this thread's last call, seconds [4] = allocation and copies to the device,
 * k_hmm_states, k_hmm_counts, the copy back and the host's sums; *peak_bytes: device memory in use during the call beyond what was
 * in use before it, by hipMemGetInfo. */
int hu_hmm_counts(int device, int64_t n_seq, int64_t cs_len, const char* msa, const double* weight, const int32_t* start, const int32_t* end,
		const uint8_t* mask, int32_t K, double* e_m, double* e_i, double* t);
int hu_hmm_counts_timing(double* seconds /* [4] */, int64_t* peak_bytes);
/* effN and the probabilities (src/BandedHMMP7.cpp:479-494), host only.  e_m, e_i, t: the counts above; n_seq: the rows of the MSA.
 * effN is RootFinder::rootBisection (src/math/RootFinder.cpp:22-76; absEps = relEps = 1e-10, resEps = 0, no iteration limit) on
 * [0, n_seq] of RelativeEntropyTargetFunc (src/BandedHMMP7.cpp:1122-1135): the counts scaled by x / n_seq (scale, :248-257),
 * estimateParams (:280-315) with DirichletMixture::meanPostP (src/math/DirichletMixture.cpp:45-61) on the match emissions and
 * DirichletDensity::meanPostP (src/math/DirichletDensity.cpp:25-27) on the rest, then meanRelativeEntropy (:317-322) in bits
 * (src/math/LinearAlgebraBasic.h:90-98) against the uniform background, minus DEFAULT_ERE = 1.  The function is pure, so the two
 * evaluations at the bracket's ends that the reference repeats on every pass are not repeated.  No sign change: effN = n_seq.
 * Then the counts are scaled by effN / n_seq and estimated once more, specials included (T[0](D,M) = 1, T[0](D,D) = 0, T[K](M,D) = 0,
 * T[K](D,M) = 1, T[K](D,D) = 0; T[K].row(M) is not renormalised).  Outputs: probabilities in the layout of the inputs (which they
 * may not alias), *eff_n, *passes = the bisection passes taken (0 without a sign change).  Sums of 4 are (x0 + x2) + (x1 + x3), of
 * 3 (x0 + x1) + x2. */
int hu_hmm_estimate(int32_t K, const double* e_m, const double* e_i, const double* t, int64_t n_seq, const hu_hmm_prior* prior,
		double* p_m, double* p_i, double* p_t, double* eff_n, int32_t* passes);
/* operator<< of BandedHMMP7 (src/BandedHMMP7.cpp:324-378) for a trained profile: HMMER3/f <version>, NAME, LENG, ALPH DNA, the tags
 * MAXL RF MM CONS CS MAP NSEQ EFFN DATE in the order build() sets them (:497-538; EFFN as %g, date: the DATE value, written as
 * given), the HMM header, then per k the match line (k = 0: COMPO) with MAP, CONS and "-" for RF, MM and CS, the insert line and the
 * transition line m->m m->i m->d i->m i->i d->m d->d.  Every number is the cost -log p at 6 significant digits (%g, the stream's
 * default); infinity is "*" on the insert and transition lines and "inf" on the match line, as Eigen prints it.  map, cons: as
 * hu_hmm_match_columns returns them.  path "-": the standard output.  Returns HU_ERR_IO when the file cannot be written. */
int hu_hmm_write(const char* path, const char* version, const char* name, int32_t K, int32_t cs_len, const double* p_m, const double* p_i,
		const double* p_t, const int32_t* map, const char* cons, int64_t n_seq, double eff_n, const char* date);

/* ---- training the prior file (hmmufotu-train-dm) ----------------------------------------------------------------
 * src/hmmufotu-train-dm.cpp:236-373 in five steps: the training sets (device), the shuffle and the moment fit that start a model
 * (host), the gradient ascent of a batch of models (device), the file (host).  A training set is [M][K]: the K values of a data
 * column lie together.  A model's alpha is [K][L], residue or transition i, component j; a density is a model with L = 1.
 *
 * hu_dm_training_data: the double loop of src/hmmufotu-train-dm.cpp:253-333 on the pruned alignment (msa, n_seq rows of cs_len bytes,
 * and weight [n_seq] as hu_msa_stats returns it).  The weights are scaled by (1 / pri_rate) / n_seq (MSA::sclaleWeight, :236-237), the
 * weighted counts are summed again from the scaled weights (MSA::updateWeightedCounts, src/MSA.cpp:280-293), a column is a match
 * column where symWFrac(j) >= symfrac (src/MSA.cpp:81-85; symfrac in [0, 1]), and the states are determineMatchingState's as in
 * hu_hmm_counts (k_hmm_states), I->D and D->I not counted.  As in the reference, the search for the next cell steps past the cell it
 * found before it tests for the end (:287-294), so a transition into the last column is dropped like one into nothing.  Outputs: mask
 * [cs_len]; data_me, data_ie [.][4] (weighted base counts of the match / other columns), data_mt [.][3] (M->M M->I M->D), data_it
 * [.][2] (I->M I->I), data_dt [.][2] (D->M D->D), each with room for cs_len columns and holding, in ascending j, the columns
 * j < cs_len - 1 with a non-zero entry (the emissions: every column); n_cols [5] their numbers of columns.  Every value is a serial
 * sum over the rows in ascending order: the reference's bit for bit.  hu_dm_training_data_timing: of this thread's last call, seconds
 * [4] = allocation and copies to the device, the weighted counts and the mask, k_hmm_states and k_dm_drop, k_dm_counts; *peak_bytes
 * as hu_hmm_counts_timing. */
int hu_dm_training_data(int device, int64_t n_seq, int64_t cs_len, const char* msa, const double* weight, double pri_rate, double symfrac,
		uint8_t* mask, double* data_me, double* data_ie, double* data_mt, double* data_it, double* data_dt, int64_t* n_cols /* [5] */);
int hu_dm_training_data_timing(double* seconds /* [4] */, int64_t* peak_bytes);
/* host only: std::random_shuffle of 0 .. M - 1 as DirichletMixture::momentInit calls it (src/math/DirichletMixture.cpp:215-218):
 * libstdc++'s loop, for i = 1 .. M - 1 swap(idx[i], idx[rand() % (i + 1)]), on the C library's rand().  seed non-NULL: srand(*seed)
 * first (src/hmmufotu-train-dm.cpp:184); NULL: the stream goes on, which is what a further seed of -n does. */
int hu_dm_shuffle(int64_t M, const uint32_t* seed, int32_t* idx);
/* host only: momentInit of a density (L = 1; src/math/DirichletDensity.cpp:105-133; idx unused) or of a mixture (L >= 2;
 * src/math/DirichletMixture.cpp:208-252; idx [M]: the order hu_dm_shuffle gave).  alpha [K][L] comes back as 1 where the reference
 * leaves the model untouched: M < 2 (density) or M < 2 L (mixture), and a density or a block of M / L columns in which no i gives
 * alphaNorm > 0. */
int hu_dm_moment_init(int32_t K, int32_t L, int64_t M, const double* data, const int32_t* idx, double* alpha);
/* trainML of src/math/DirichletDensity.cpp:46-77 and src/math/DirichletMixture.cpp:92-146 without their momentInit, for n independent
 * problems on the device: k_dm_train, one workgroup per problem, at most `chunk` iterations per launch; the host launches until no
 * problem is running and calls progress(user, iterations of the furthest problem, problems still running) after every launch.  What
 * a problem carries between launches is complete: the result is the same bit for bit for every chunk and for every batch the problem
 * is part of.  K 2 .. 4; L 1 (density) or 2 .. 10 (mixture); alpha0 [K][L] > 0 (w starts as its logarithm); q0 [L], NULL: 1 / L.
 * status: HU_DM_CONVERGED the reference's stop test (isApprox on alpha at abs_eps_params + rel_eps_params |alpha_old|, and
 * 0 <= deltaC < abs_eps_cost + rel_eps_cost cOld); HU_DM_MAXIT max_iter iterations done (0: no limit); HU_DM_NAN_OVERFIT an alpha
 * became 0 and HU_DM_NAN_UNUSED a mixture coefficient fell below 1 / M, the reference's two NaN returns (cost: NaN);
 * HU_DM_NOT_FINITE the cost is NaN or infinite, where the reference would not end.  M = 0: nothing is trained, alpha0 comes back with
 * cost 0 and HU_DM_CONVERGED after 0 iterations. */
#define HU_DM_CONVERGED 1
#define HU_DM_MAXIT 2
#define HU_DM_NAN_OVERFIT 3
#define HU_DM_NAN_UNUSED 4
#define HU_DM_NOT_FINITE 5
typedef struct { int32_t K, L; int64_t M; const double* data; const double* alpha0; const double* q0; } hu_dm_problem;
typedef struct { double eta, abs_eps_cost, rel_eps_cost, abs_eps_params, rel_eps_params; int64_t max_iter; int32_t chunk, pad0; } hu_dm_opts;
typedef struct { double alpha[4][10]; double q[10]; double cost; int64_t iterations; int32_t status, pad0; } hu_dm_result;
typedef void (*hu_dm_progress)(void* user, int64_t iterations, int32_t running);
void hu_dm_default_opts(hu_dm_opts* o);     /* eta 0.001 (src/math/DirichletModel.cpp:15); epsilons 0, 1e-6, 0, 1e-4 (src/BandedHMMP7Prior.cpp:32-35); max_iter 0; chunk 64 */
int hu_dm_train(int device, int32_t n, const hu_dm_problem* prob, const hu_dm_opts* opts, hu_dm_result* out, hu_dm_progress progress, void* user);
/* test probe: the kernels' lgamma (the device library's) and digamma (hu_kern_dm.h) at n points x > 0 */
int hu_dm_special(int device, int64_t n, const double* x, double* lgamma_out, double* digamma_out);
/* host only: operator<< of BandedHMMP7Prior (src/BandedHMMP7Prior.cpp:62-69) with DirichletMixture::print
 * (src/math/DirichletMixture.cpp:197-206) and DirichletDensity::print (src/math/DirichletDensity.cpp:96-103): the training costs cost
 * [5] (ME IE MT IT DT) at the stream's 6 digits, q and alpha under Eigen's FullPrecision format, 16 significant digits, every entry
 * right-aligned to the widest of its matrix.  path "-": the standard output. */
int hu_dm_write(const char* path, const hu_hmm_prior* prior, const double* cost /* [5] */);

/* ---- OTU tables: hmmufotu-merge, hmmufotu-subset, hmmufotu-norm ----
 * The reference's "table" format (OTUTable::loadTable / saveTable, src/OTUTable.cpp:123-164, behind readProgInfo / writeProgInfo,
 * src/util/ProgEnv.cpp:101-135): a first line "# HmmUFOtu <version> <info>", a header "otuID <TAB> sample ... <TAB> taxonomy", then per
 * OTU its id, one number per sample and the rest of the line as taxonomy.  All of hu_otu_table_* is host code.
 * hu_otu_table_read: HU_ERR_IO with the reference's message when the first line does not scan as "# <name> <version>", names another
 * program, or carries a version above v1.5.1; a second row with an id already seen is dropped (addOTU returns the first).  Refused
 * here and not by the reference: a value line before the header (it would add a row of no columns), a second header, a row that has
 * fewer numbers than the header has samples.  Blank lines are passed over.
 * hu_otu_table_new: a table from arrays, counts [n_otu][n_sample] row-major; a repeated id is dropped as the reader drops it.
 * hu_otu_table_write: "# HmmUFOtu v1.5.1<info>", the header, one row per OTU; numbers at ostream's precision 15 as hmmufotu-amd-sum
 * writes them.  path "-": the standard output.
 * hu_otu_table_merge: dst += src (src/OTUTable.cpp:211-240): new samples, then new OTUs with src's taxonomy, appended in first-seen
 * order; counts of a sample name both have are added; an empty dst becomes a copy of src.
 * hu_otu_table_prune_samples: drops the columns whose sum is < min (min 0: none); hu_otu_table_prune_otus: the rows whose sum is 0.
 * hu_otu_table_normalize (normalizeConst, :110-121): Z 0 = the largest column sum; every cell becomes cell / (colsum / Z), column sums
 * taken in ascending row order; an empty or all-zero table is left alone.  A column whose sum is 0 stays 0 and is counted in
 * *zero_columns (may be NULL) — the reference divides by 0 there and prints NaN.  HU_ERR_ARG for Z < 0 or NaN.
 * The pointers the getters return stay valid until the table is changed or freed; hu_otu_table_counts is writable. */
typedef struct hu_otu_table hu_otu_table;
int hu_otu_table_read(const char* path, hu_otu_table** out);
int hu_otu_table_new(int64_t n_otu, int64_t n_sample, const char* const* otu_ids, const char* const* taxa, const char* const* samples, const double* counts,
		hu_otu_table** out);
void hu_otu_table_free(hu_otu_table* t);
int hu_otu_table_dims(const hu_otu_table* t, int64_t* n_otu, int64_t* n_sample);
const char* hu_otu_table_otu(const hu_otu_table* t, int64_t i);
const char* hu_otu_table_taxon(const hu_otu_table* t, int64_t i);
const char* hu_otu_table_sample(const hu_otu_table* t, int64_t j);
double* hu_otu_table_counts(hu_otu_table* t);     /* [n_otu][n_sample], row-major */
int hu_otu_table_write(const hu_otu_table* t, const char* path, const char* info);
int hu_otu_table_merge(hu_otu_table* dst, const hu_otu_table* src);
int hu_otu_table_prune_samples(hu_otu_table* t, uint64_t min);
int hu_otu_table_prune_otus(hu_otu_table* t);
int hu_otu_table_normalize(hu_otu_table* t, double Z, int64_t* zero_columns);

/* hu_otu_subset: every sample (column) of counts [n_otu][n_sample] rarefied to `size` reads into out (same shape; may not alias counts),
 * OTUTable::subsetUniform / subsetMultinom (src/OTUTable.cpp:166-209).  A sample with T_j <= size reads is returned untouched, as there.
 * device < 0: the host path; otherwise the kernels of hu_kern_draw.h (uniform) or hu_kern_otu.h (multinomial) on that device.  Both give the same integers.
 * The distributions are the reference's, the streams are not (it draws from Boost's mt11213b): the generator is Philox4x32-10
 * (hu_sim_philox) under the key (seed & 0xffffffff, seed >> 32), and a result is defined by names, not by the order of execution.
 * HU_OTU_UNIFORM, without replacement: the reads of sample j are numbered t = 0 .. T_j - 1 in row order, OTU i owns [P_i, P_i+1), P the
 * exclusive prefix sum of column j.  Read t has the key k = (w0 << 32 | w1) >> (64 - key_bits), w the output of the counter
 * (t & 0xffffffff, t >> 32, j, 2).  The `size` reads smallest in (key, t) order are kept; an OTU's new count is how many lie in its range.
 * HU_OTU_MULTINOMIAL, with replacement: draw m = 0 .. size - 1 takes r = w0 << 32 | w1 of the counter (m & 0xffffffff, m >> 32, j, 3)
 * and counts for the OTU that owns read t = (r * T_j) >> 64 (the high half of the 128-bit product; the bias is below T_j / 2^64).
 * opts NULL: the defaults.  chunk: reads (draws) per workgroup, > 0, device path only — the result does not depend on it.  key_bits:
 * 1 .. 64; below 64 it makes keys tie, so that the tie rule can be tested; the programs do not offer it.
 * HU_ERR_ARG with the reason, before anything reaches a device: a cell that is negative, not finite or not an integer (the reference
 * truncates fractions silently), a column total of 2^32 or more, size 0, an unknown method, chunk or key_bits out of range.
 * hu_otu_subset_timing: of this thread's last device call, seconds [3] = copies to the device, kernels, copy back. */
#define HU_OTU_UNIFORM 0
#define HU_OTU_MULTINOMIAL 1
typedef struct {
	int32_t chunk;        /* 16384 */
	int32_t key_bits;     /* 64 */
} hu_otu_opts;
void hu_otu_default_opts(hu_otu_opts* o);
int hu_otu_subset(int device, int64_t n_otu, int64_t n_sample, const double* counts, uint64_t size, int method, uint64_t seed, const hu_otu_opts* opts,
		double* out);
int hu_otu_subset_timing(double* seconds /* [3] */);

/* ---- hmmufotu-amd-unifrac: the distances between the samples of an OTU table on the database's tree ----
 * The tree is the .ptu's, rooted at its stored root.  Branch v is the edge from node v to its parent, of length b_v (hu_tree_info_node's
 * blen); the root has none.  HmmUFOtu places reads on inner nodes as well as on leaves: a read of OTU u lies below every branch on the
 * path from u to the root, u's own branch included (what zero-length pseudo-leaves would give).  An OTU that is the root lies below no
 * branch but counts in its sample's total.  With c_uj the table's cell and T_j the column sum,
 *     p_vj = (sum of c_uj over the OTUs u in the subtree of v) / T_j,
 * and every sum below runs over the branches with p_vi + p_vj > 0:
 *   HU_UF_UNWEIGHTED    sum b_v |[p_vi > 0] - [p_vj > 0]| / sum b_v max([p_vi > 0], [p_vj > 0])
 *   HU_UF_WEIGHTED      sum b_v |p_vi - p_vj| / sum b_v (p_vi + p_vj)
 *   HU_UF_WEIGHTED_RAW  sum b_v |p_vi - p_vj|
 *   HU_UF_GENERALIZED   sum b_v s^alpha |p_vi - p_vj| / s / sum b_v s^alpha, s = p_vi + p_vj, 0 <= alpha <= 1
 *   HU_UF_BRAY_CURTIS, HU_UF_JACCARD: WEIGHTED and UNWEIGHTED on the identity tree, where every OTU row is its own branch of length 1;
 *                       tree must be NULL, otu_node is not read.
 * A denominator of 0 (both samples on the root alone) gives 0; d(i,i) is exactly 0; d(j,i) is the stored copy of d(i,j).  pd (may be
 * NULL) [n_sample]: Faith's PD, sum b_v [p_vj > 0].
 * hu_unifrac: counts [n_otu][n_sample] row-major, otu_node [n_otu] the node of every row (two rows may name one node), dist
 * [n_sample][n_sample].  Only the branches on a path from some row's node to the root are kept, B of them, numbered in depth-first
 * order (children in ascending node number); the device fills P [B][n_sample] from one column scan of the rows in that order and one
 * gather (integer counts below 2^53 come out exact), then k_unifrac_pairs (hu_kern_unifrac.h) adds the terms: branches in ascending
 * order within slabs of `slab` consecutive branches, the slabs then in ascending order.  The order is a function of the table, the tree
 * and the slab alone, so a result does not depend on the run, the grid or the device, and the host path (opts->host) gives the same
 * bits for every method but HU_UF_GENERALIZED with 0 < alpha < 1, where the two pow / sqrt differ.
 * slab 0: hu_unifrac_default_slab(n_sample, B) = B when the nt (nt + 1) / 2 tiles, nt = ceil(n_sample / 64), number 1024 or more;
 * otherwise max(256, 32 ceil(ceil(B / ceil(1024 / tiles)) / 32)).
 * HU_ERR_ARG with the reason, before a device is asked for: n_sample < 1, an unknown method, alpha outside [0, 1] or given (not 0.5)
 * without HU_UF_GENERALIZED, slab < 0, a tree with an identity method or none with a tree method, a node outside [0, n_nodes), a
 * parent array that is no rooted tree, a kept branch whose length is negative or not finite, a cell that is negative or not finite, a
 * sample without reads.  HU_ERR_NOMEM with the bytes needed and the bytes free (mem_budget, when > 0 and smaller) when the device
 * cannot hold P, the scan and the partial sums.
 * hu_unifrac_embed: *n_branch = B; with P == NULL nothing else is done (no device).  Otherwise cap_branch >= B, and branch_node [B]
 * (may be NULL), branch_len [B] (may be NULL) and P [B][n_sample] are filled.
 * hu_unifrac_timing: of this thread's last device call, seconds [4] = copies up, embedding, pair kernels, copy back. */
#define HU_UF_UNWEIGHTED 0
#define HU_UF_WEIGHTED 1
#define HU_UF_WEIGHTED_RAW 2
#define HU_UF_GENERALIZED 3
#define HU_UF_BRAY_CURTIS 4
#define HU_UF_JACCARD 5
typedef struct {
	int32_t method;       /* HU_UF_WEIGHTED */
	int32_t host;         /* 0; 1: the host path, no device needed */
	double alpha;         /* 0.5 */
	int64_t slab;         /* 0: hu_unifrac_default_slab */
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_unifrac_opts;
typedef struct {
	int32_t n_nodes;
	const int32_t* parent;   /* [n_nodes], -1: the root */
	const double* blen;      /* [n_nodes], the length of the branch to the parent */
} hu_unifrac_tree;
void hu_unifrac_default_opts(hu_unifrac_opts* o);
int64_t hu_unifrac_default_slab(int64_t n_sample, int64_t n_branch);
int hu_unifrac(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, double* dist, double* pd);
int hu_unifrac_embed(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		const hu_unifrac_opts* opts, int64_t* n_branch, int64_t cap_branch, int32_t* branch_node, double* branch_len, double* P);
int hu_unifrac_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-permanova: do the sample groups differ on a distance matrix? (PERMANOVA, Anderson 2001) ----
 * dist [n][n] row-major: symmetric, non-negative, finite, zero on the diagonal.  group [n]: a label in 0 .. a-1 per sample, n_g the
 * group sizes.  With D2_ij = d_ij * d_ij (one rounded product):
 *     SS_T = (1/n) sum_{i<j} D2_ij,  SS_W = sum_{i<j, g_i == g_j} D2_ij / n_{g_i},  SS_A = SS_T - SS_W,
 *     F = (SS_A / (a-1)) / (SS_W / (n-a)),  R2 = SS_A / SS_T,  p = (1 + #{pi : SS_W(pi) <= SS_W(observed)}) / (perms + 1).
 * The order of every sum is a function of n alone: the samples in tiles of 64, the tiles (I, J), I <= J, in ascending row-major order;
 * in a tile, for i ascending, r_i = the matching D2_ij of the tile, j ascending, j > i, by plain adds from +0, then s = fma(1/n_{g_i},
 * r_i, s) over i ascending from +0; the tile sums then by plain adds in tile order from +0.  SS_T: the same with every pair matching
 * and plain adds of r_i, divided by n at the end.  So relabellings that induce one partition give the same bits, the result depends
 * on neither chunk nor the device, and the host path (opts->host, or device < 0: one thread, no device needed) gives the same bits.
 * Permutation p (0-based) is a Fisher-Yates shuffle of the observed labels, for i = n-1 down to 1: w = Philox4x32-10 (hu_sim_philox) of
 * the counter (i & 0xffffffff, i >> 32, p & 0xffffffff, p >> 32) under the key (seed & 0xffffffff, seed >> 32), x = w[1] << 32 | w[0],
 * j = the high 64 bits of x (i + 1), swap g[i] and g[j].  No rejection: j is off the uniform by (i + 1) / 2^64 at the most.
 * hu_permanova: ssw_perm (may be NULL) [perms] receives SS_W of every permutation.  chunk: permutations per launch (0: as many as the
 * memory holds, 16,384 at the most); the device works on chunks padded to whole workgroups of 256.
 * HU_ERR_ARG with the reason, before a device is asked for: n < 3, a negative label, labels not dense in 0 .. a-1, a < 2, a > n-1,
 * a > 65,535, perms < 1 or > 10^7, chunk < 0, a cell that is negative, not finite or above 2^511 (its square
 * would not be finite), d_ij != d_ji (with both indices), a non-zero
 * diagonal, every distance 0.  HU_ERR_NOMEM with the bytes needed and the bytes free when hu_permanova_need exceeds mem_budget (checked
 * before a device is asked for) or what the device reports free.  SS_W == 0 gives F = +inf; p still comes from the SS_W comparison.
 * hu_permanova_labels: host only, out [count][n] the labellings of permutations first .. first + count - 1.
 * hu_permanova_need: the bytes on the device for a chunk: 8 n^2 for the matrix, and with c = chunk rounded up to 256 and t the tiles,
 * 2 n c for the labels, 8 t c for the partial sums, 8 c for the outputs, 8 a + 2 n for the tables and 1 MB of slack; -1 on a bad argument.
 * hu_permanova_timing: of this thread's last device call, seconds [4] = copies up, shuffles, pair kernel, finish and copy back.
 * hu_dist_matrix_read: the file hmmufotu-amd-unifrac -o writes: a first line of names, each after a tab, then per sample its name and n
 * numbers, tab-separated.  HU_ERR_IO with the line otherwise.  The pointers the getters return stay valid until the matrix is freed. */
typedef struct {
	int64_t perms;        /* 999 */
	uint64_t seed;        /* 1 */
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t reserved;
	int64_t chunk;        /* 0: chosen from n and the memory */
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_permanova_opts;
typedef struct {
	int64_t n, a, perms;
	double ss_total, ss_within, ss_among, F, R2;
	int64_t count_le;
	double p;
} hu_permanova_result;
void hu_permanova_default_opts(hu_permanova_opts* o);
int hu_permanova(int device, int64_t n, const double* dist, const int32_t* group, const hu_permanova_opts* opts, hu_permanova_result* out,
		double* ssw_perm /* [perms] or NULL */);
int hu_permanova_labels(int64_t n, const int32_t* group, uint64_t seed, int64_t first, int64_t count, int32_t* out /* [count][n] */);
int64_t hu_permanova_need(int64_t n, int64_t a, int64_t chunk);
int hu_permanova_timing(double* seconds /* [4] */);
typedef struct hu_dist_matrix hu_dist_matrix;
int hu_dist_matrix_read(const char* path, hu_dist_matrix** out);
void hu_dist_matrix_free(hu_dist_matrix* m);
int hu_dist_matrix_dims(const hu_dist_matrix* m, int64_t* n);
const char* hu_dist_matrix_sample(const hu_dist_matrix* m, int64_t i);
const double* hu_dist_matrix_values(const hu_dist_matrix* m);     /* [n][n], row-major */

/* ---- hmmufotu-amd-permanova --design: covariates, several terms, strata (sequential sums of squares) ----
 * dist [n][n] as hu_permanova takes it, D2_ij = d_ij * d_ij (one rounded product).  An ordered list of T >= 1 terms, each a numeric
 * variable (one column), a categorical variable of L levels (L - 1 indicator columns, of the labels 1 .. L-1: the caller numbers the
 * levels in order of first appearance) or an interaction A:B of two variables (every product of a raw column of A with a raw column
 * of B, A's columns the outer loop).  An optional stratum label per sample.
 * hu_design_build (host): every raw column is centred, and one that holds a numeric variable is divided by its centred 2-norm.  The
 * columns are walked in term order: each is orthogonalised against all kept columns by modified Gram-Schmidt, applied twice, centred
 * again and normalised; a column whose norm after projection is below 1e-10 of its norm before is dropped.  Q [n][q] row-major: its
 * columns are orthonormal and orthogonal to the vector of ones.  df_t = the kept columns of term t, columns term_start[t] ..
 * term_start[t + 1] - 1; df_res = n - 1 - q.  Every inner product and every sum of the builder is compensated (two-product, two-sum), so
 * that max |Q'Q - I| <= q 2^-50 and max |1'Q| <= n 2^-52 hold (§33).  Q must have room for n * hu_design_raw_columns doubles; the first
 * n * q of them are the result.  HU_ERR_ARG by name (term_name [T], may be NULL: then by number) for a term with df_t = 0 ("adds nothing
 * to the terms before it"), for df_res < 1, for a value that is not finite, for labels that are negative or not dense.
 * Statistic, for a permutation pi of the sample indices (the design row of sample i is row pi(i) of Q), v_c[i] = Q[pi(i)][c]:
 *     s_c = v_c' D2 v_c,  SS_t = -1/2 sum_{c of term t, ascending} s_c,  SS_res = SS_T - (sum_t SS_t, t ascending),  SS_T = hu_permanova's,
 *     F_t = (SS_t / df_t) / (SS_res / df_res),  R2_t = SS_t(observed) / SS_T,
 *     p_t = (1 + #{pi : F_t(pi) >= F_t(obs) - 2^-26 |F_t(obs)|}) / (perms + 1).
 * The raw data are permuted (as vegan's adonis2(by = "terms")).  The observed statistic is the identity run through the same code.  The
 * tolerance 2^-26 is vegan's sqrt(eps) convention, not a measurement: a relabelling that keeps a categorical design's column space gives
 * the same F in exact arithmetic but other vectors and so other bits.  A permutation whose F_t is NaN does not count (count_nan).
 * Permutation p is a function of (seed, p, strata) alone: from the identity index array, for every stratum with members m_0 < ... <
 * m_{k-1}, for t = k-1 down to 1: x = Philox4x32-10 of the counter (m_t, p) under the key seed, packed as hu_permanova packs (i, p),
 * j = the high 64 bits of x (t + 1), swap idx[m_t] and idx[m_j].  Without strata these are hu_permanova's swaps: group[idx[i]] equals
 * hu_permanova_labels(n, group, seed, p)[i].
 * Order of sums: the bits of s_c are a function of (n, D2, v_c) alone.  On the device the rows go in blocks of 64 and the columns of D2
 * in the K slabs of hu_pcoa (a function of n); a cell of D2 v is accumulated by v_mfma_f64_16x16x4_f64 over its slab in ascending steps
 * of 4; over the block's 64 rows the cells times v_i are added in a fixed order: the 4 rows of a lane ascending by fma from +0, then by
 * plain adds the 4 lane groups ascending, the 4 waves ascending, the slabs ascending and the row blocks ascending.  Neither chunk, nor the column's place in a
 * launch, nor the grid enters.  The host path (opts->host, or device < 0: one thread, straight loops, no device needed) is held to the
 * same derived error bound as the device, |SS_t - exact| <= df_t n^3 2^-50 max D2, not to its bits: the matrix instruction's inner
 * order is not documented.
 * hu_permanova_design: Q, q, term_start as hu_design_build gives them (any orthonormal centred basis is taken); result [T];
 * ss_perm (may be NULL) [perms][T] receives SS_t of every permutation.  index32: 32-bit entries of the index array on the device where
 * 16-bit ones would do (n <= 65,536); the results are the same bits.
 * HU_ERR_ARG with the reason, before a device is asked for: the matrix refusals of hu_permanova, n < 3, q < 1, df_res < 1, a Q that is
 * not finite, term_start not ascending from 0 to q, a stratum label that is negative or not dense, every stratum a single sample,
 * perms < 1 or > 10^7, chunk < 0.  HU_ERR_NOMEM with the bytes needed and the bytes free when hu_permanova_design_need exceeds
 * mem_budget (checked before a device is asked for) or what the device reports free.
 * hu_permanova_design_need: with c = chunk rounded up to 64, e = 2 (n <= 65,536 and no index32) or 4, w = c q rounded up to 64,
 * b = ceil(n / 64) and s the K slabs of n: 8 n^2 for the matrix, e n c for the index array, 8 n q for Q, 8 b s w for the partial sums,
 * 8 w + 8 c T for the outputs, 4 (2 n + 1) for the strata and 1 MB of slack; -1 on a bad argument.  chunk 0 in the options: the largest
 * multiple of 64 that fits, 16,384 at the most.
 * hu_permanova_design_timing: of this thread's last device call, seconds [4] = copies up (with the squares), shuffles, quadratic-form
 * kernel, finish and copy back.
 * hu_permanova_perms: host only, out [count][n] the index arrays of permutations first .. first + count - 1. */
typedef struct {
	int32_t kind;         /* 0: numeric (value [n]); 1: categorical (label [n], dense in 0 .. L-1) */
	int32_t reserved;
	const double* value;
	const int32_t* label;
} hu_design_var;
typedef struct {
	int32_t a, b;         /* the variables of the term; b < 0: the variable a alone */
} hu_design_term;
typedef struct {
	int64_t perms;        /* 999 */
	uint64_t seed;        /* 1 */
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t index32;      /* 0; 1: 32-bit index entries on the device at any n */
	int64_t chunk;        /* 0: chosen from n, q and the memory */
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_permanova_design_opts;
typedef struct {
	int64_t df, df_res;
	double ss, ss_res, ss_total, R2, F;
	int64_t count_ge, count_nan;
	double p;
} hu_permanova_design_term;
int64_t hu_design_raw_columns(int64_t n, int64_t n_var, const hu_design_var* var, int64_t T, const hu_design_term* term);
int hu_design_build(int64_t n, int64_t n_var, const hu_design_var* var, int64_t T, const hu_design_term* term, const char* const* term_name,
		double* Q, int64_t* q, int64_t* term_start /* [T + 1] */, int64_t* df /* [T] */, int64_t* dropped /* [T] */);
void hu_permanova_design_default_opts(hu_permanova_design_opts* o);
int hu_permanova_perms(int64_t n, const int32_t* strata /* [n] or NULL */, uint64_t seed, int64_t first, int64_t count, int64_t* out /* [count][n] */);
int hu_permanova_design(int device, int64_t n, const double* dist, const double* Q, int64_t q, int64_t T, const int64_t* term_start,
		const int32_t* strata /* [n] or NULL */, const hu_permanova_design_opts* opts, hu_permanova_design_term* result /* [T] */,
		double* ss_perm /* [perms][T] or NULL */);
int64_t hu_permanova_design_need(int64_t n, int64_t q, int64_t T, int64_t chunk, int32_t index32);
int hu_permanova_design_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-tree: a neighbour-joining tree from the MSA ----
 * Plain neighbour joining (Saitou and Nei 1987, in the form of Studier and Keppler 1988) on the pairwise distances of the alignment's
 * rows: not a maximum-likelihood search.  rows [n][cs_len]: the pruned alignment in the codes of hu_msa_encode_table (0..3 = A C G T, a
 * negative code is no symbol; a code above 3 is refused).  A device below 0, or opts->host, runs the host path, which needs no device.
 *
 * hu_msa_pair_counts, for tests and small n: counts [n][n][4] = per pair N (the columns where both rows hold a symbol), P_R (A<->G
 * differences), P_Y (C<->T differences) and Q (transversions); the diagonal holds a row against itself.  Exact integers.
 *
 * hu_msa_distances: D [n][n], symmetric with a zero diagonal, from the closed forms of the reference's subDist (HU_DIST_JC69: src/JC69.h:103,
 * HU_DIST_K80: src/K80.h:120, HU_DIST_F81: src/F81.h:120, HU_DIST_HKY85: src/HKY85.h:155, HU_DIST_TN93: src/TN93.h:156) or the plain
 * p-distance; pi [4] is read by F81, HKY85 and TN93 only.  N == 0 gives 0, as the reference does.  A pair whose formula takes the
 * logarithm of a value <= 0 is saturated: it gets `sat` when sat > 0, and otherwise (sat == 0) twice the largest finite distance of the
 * matrix, set in a second pass; *n_saturated (may be NULL) counts such pairs (i < j).  Refused with HU_ERR_ARG: n < 2, cs_len outside
 * [1, 65535], a code above 3, an unknown type, a pi that is not four positive numbers where it is read, sat < 0 or not finite, and a
 * matrix without one finite off-diagonal distance when sat == 0.  The counts are integers, so D does not depend on the grid; the
 * device's log may differ from the host's in the last bits.
 *
 * hu_nj: D [n][n] (symmetric, zero diagonal, finite; anything else is refused) is not changed.  Leaves are nodes 0 .. n - 1; join t
 * (0 <= t < n - 3) makes node n + t from join[t][0] and join[t][1] with the branch lengths len[t][0] and len[t][1]; last3 [3] are the
 * nodes that hang on the top node, with last_len3 [3].  The order of every comparison and every sum is fixed, so the
 * host path and the device give the same bits, whatever the grid.  n >= 3; n above 262144 is refused.
 *
 * hu_msa_tree: both steps with the matrix kept on the device between them, as hmmufotu-amd-tree runs them; D_out (may be NULL) [n][n]
 * receives the distances.  Before anything is allocated the device's free memory (opts->mem_budget, when > 0 and smaller) is held
 * against the need, the n x n FP64 matrix, the bit-planes, the rows, the vectors and 1 MB of slack: HU_ERR_NOMEM names both numbers.
 * hu_nj and hu_msa_distances check the same way.
 * hu_nj_timing: of this thread's last device call, seconds [4] = copies up and encoding, distances, joins, copies back.
 *
 * hu_nj_newick: the tree as Newick text, unrooted with three children at the top node: leaves carry names[i], inner nodes no name,
 * lengths as %.17g.  A name that is no unquoted Newick label is written in single quotes; one that holds a quote or a byte that does
 * not print is refused.  Returns the length (without the terminator) and writes at most cap bytes, terminator included; HU_ERR_ARG
 * (negative) on a bad argument.  Host only. */
#define HU_DIST_PDIST 0
#define HU_DIST_JC69 1
#define HU_DIST_K80 2
#define HU_DIST_F81 3
#define HU_DIST_HKY85 4
#define HU_DIST_TN93 5
typedef struct {
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t reserved;
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_nj_opts;
void hu_nj_default_opts(hu_nj_opts* o);
int hu_msa_pair_counts(int device, int64_t n, int64_t cs_len, const int8_t* rows, int32_t* counts);
int hu_msa_distances(int device, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, double* D,
		int64_t* n_saturated);
int hu_nj(int device, int64_t n, const double* D, const hu_nj_opts* opts, int32_t* join, double* len, int32_t* last3, double* last_len3);
int hu_msa_tree(int device, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, const hu_nj_opts* opts,
		double* D_out, int64_t* n_saturated, int32_t* join, double* len, int32_t* last3, double* last_len3);
int hu_nj_timing(double* seconds /* [4] */);
int64_t hu_nj_newick(int64_t n, const char* const* names, const int32_t* join, const double* len, const int32_t* last3, const double* last_len3,
		char* buf, int64_t cap);

/* ---- hmmufotu-amd-tree --ml-lengths: maximum-likelihood branch lengths on a fixed topology ----
 * The tree is given as hu_tree_evaluate takes it: parent [n] (-1: the root), blen [n] (the root's is not read), seq [n][cs_len] with the
 * leaf rows in the codes of hu_msa_encode_table (inner rows are not read).  The model is the fixed-rate one: dg_k > 0 is refused with
 * HU_ERR_ARG, because the reference averages the rate categories at every inner node (src/PhyloTreeUnrooted.cpp:340-341), which leaves
 * no objective of one branch that does not depend on the root.
 *
 * The objective of the branch above a non-root node u, all other lengths fixed.  With up[u] the message of u's subtree at u and down[u]
 * that of everything else at u's parent (log space, neither carried over the branch: the convention of hu_tree_evaluate,
 * src/PhyloTreeUnrooted.cpp:315-374), x = exp(up[u][j] - max), y = exp(down[u][j] - max) and P(t) = U diag(exp(lam t)) U1
 * (hu_model_spectral; lam[0] = 0, U[.][0] = 1, U1[0][.] = pi):
 *   L_j(t) = sum_ab pi_a x_a P_ab(t) y_b = sum_k c_jk exp(lam_k t),   c_jk = (sum_a pi_a x_a U_ak) (sum_b U1_kb y_b),
 *   f_u(t) = sum_j log L_j(t) = sum_j [ log c_j0 + max up + max down + log(1 + sum_k>0 r_jk exp(lam_k t)) ],   r_jk = c_jk / c_j0,
 * c_j0 = (pi . x)(pi . y) > 0.  With N_j = sum_k r_jk lam_k e_k, M_j = sum_k r_jk lam_k^2 e_k, D_j = 1 + sum_k r_jk e_k:
 *   f_u'(t) = sum_j N_j / D_j,   f_u''(t) = sum_j [ M_j / D_j - (N_j / D_j)^2 ].
 * f_u(blen[u]) is the tree's log-likelihood for every u (the value of hu_tree_loglik; src/PhyloTreeUnrooted.cpp:707-712).
 *
 * hu_tree_branch_scores: f, d1, d2 [n] = f_u, f_u', f_u'' at t[u] (t == NULL: at blen[u]); the root's entries are 0.
 * hu_tree_branch_step: t_star [n] = the maximiser of f_u on [min_len, max_len] by safeguarded Newton on f_u': a bracket is kept, and the
 *   step is a bisection when f_u'' >= 0 or Newton's step leaves the bracket; f_u'(min_len) <= 0 gives min_len, f_u'(max_len) >= 0 gives
 *   max_len.  It stops at a step of at most HU_BLEN_TAU, after HU_BLEN_MAX_NEWTON steps at the latest; capped [n] (may be NULL) marks
 *   the branches that hit that cap and opts->n_capped counts them.  f, d1, d2 (may be NULL): the scores at blen[u].  The reference
 *   fits one branch at a time to BRANCH_EPS in the same way (optimizeBranchLength, src/PhyloTreeUnrooted.cpp:749-798).
 * hu_tree_optimize_lengths: rounds of simultaneous steps on blen [n], in place.  From ll = the log-likelihood at blen, a round sweeps
 *   up and down, takes t* of every branch and delta = max_u |t*_u - blen_u|; delta <= eps ends the run as converged.  Otherwise
 *   cand = blen + s (t* - blen) for s = 1, 1/2, ... (10 values at the most), each with an up sweep and the serial column sum of
 *   hu_tree_loglik; the first cand with a larger ll is taken, and if none is the run stops.  At most max_rounds rounds.  The report:
 *   ll_start, ll_final, n_rounds, stop, and per accepted round (rounds, when not NULL, holds rounds_cap entries) ll, s, delta and the
 *   branches that hit the Newton cap.  The two branches at a bifurcating root are one branch of the unrooted tree: each is fitted given
 *   the other, and only their sum is determined.
 * Memory: 64 n cs_len bytes of messages, n cs_len of rows, 24 n cs_len of ratios when cs_len is above HU_BLEN_LDS_COLS, 8 cs_len of column
 * values and 1 MB of slack (hu_blen_need).  It is held against mem_budget (when > 0) before anything is allocated, on the host path too,
 * and on the device against the free memory: HU_ERR_NOMEM names both numbers.  opts->host, or device < 0, runs the host path
 * (hu_blen_host.cpp), which needs no device.  hu_blen_timing: seconds [4] of this thread's last hu_tree_optimize_lengths = the full
 * sweeps, the steps, the trial sweeps with their log-likelihoods, the copies. */
#define HU_BLEN_TAU 1e-8           /* at most eps / 100 for every eps the entries take: eps below 1e-6 is refused */
#define HU_BLEN_MAX_NEWTON 100
#define HU_BLEN_MAX_HALVINGS 10
#define HU_BLEN_LDS_COLS 1450      /* the ratios of a branch stay in LDS up to this many columns: 24 cs_len + 6 KB of reduction scratch, four workgroups in a CU's 160 KB;
                                    * with fewer workgroups per CU the global scratch, which the L2 holds, was measured faster */
enum { HU_BLEN_CONVERGED = 0, HU_BLEN_NO_STEP = 1, HU_BLEN_MAX_ROUNDS = 2 };
typedef struct { double ll, s, delta; int64_t n_capped; } hu_blen_round;
typedef struct {
	double eps;           /* 1e-5, the reference's BRANCH_EPS (src/PhyloTreeUnrooted.cpp:71) */
	double min_len;       /* 0 */
	double max_len;       /* 10 */
	int32_t max_rounds;   /* 50 */
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t device;       /* 0 */
	int32_t rounds_cap;   /* entries of rounds */
	int64_t mem_budget;   /* 0: what the device reports free */
	hu_blen_round* rounds;
	/* the report */
	int32_t n_rounds, stop;
	double ll_start, ll_final;
	int64_t n_capped;     /* hu_tree_branch_step: branches at the Newton cap; hu_tree_optimize_lengths: of all rounds */
} hu_blen_opts;
void hu_blen_default_opts(hu_blen_opts* o);
int64_t hu_blen_need(int32_t n_nodes, int32_t cs_len);
int hu_tree_branch_scores(const hu_blen_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, const double* t, double* f, double* d1, double* d2);
int hu_tree_branch_step(hu_blen_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* t_star, double* f, double* d1, double* d2, uint8_t* capped);
int hu_tree_optimize_lengths(hu_blen_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, double* blen, const int8_t* seq,
		const hu_model_desc* model);
int hu_blen_timing(double* seconds /* [4] */);
/* the tree of hu_newick_parse written back with other branch lengths (blen [n], the root's is not written) at 17 significant digits:
 * the same topology, names and order of children; a name that is no unquoted label is written in single quotes.  Returns the length
 * (without the terminator) and writes at most cap bytes, terminator included; HU_ERR_ARG (negative) on a bad argument.  Host only. */
int64_t hu_newick_write(const hu_newick* t, const double* blen, char* buf, int64_t cap);

/* ---- hmmufotu-amd-tree --ml-lengths --gamma K: branch lengths and the shape under the discrete Gamma of rates ----
 * The textbook model (Yang 1994): every column has one of K equally probable rates, and its likelihood is the mean over the K
 * fixed-rate likelihoods with all lengths multiplied by the rate.  It is NOT the reference's DiscreteGammaModel (hu_dg_model), which
 * averages the categories at every inner node and whose rates sum to 1: here the rates sum to K, the mean rate is 1, and a length stays
 * substitutions per site in the unit of the model file.  `model` is the fixed-rate model: dg_k != 0 is refused as in §22.
 *
 * hu_gamma_rates: rates [K], ascending: rate_i = K [P(alpha + 1, q_{i+1}) - P(alpha + 1, q_i)] with q_i the i/K quantile of
 *   Gamma(shape alpha, scale 1), q_K = inf and P the regularised incomplete gamma function: the mean of Gamma(shape alpha, rate alpha)
 *   over its i-th K-quantile.  K is 1 to 16 (HU_MAX_DGK), alpha in [HU_GAMMA_ALPHA_MIN, HU_GAMMA_ALPHA_MAX].  Host only.
 *
 * The objective of the branch above u.  Category c has the messages up_c, down_c of the sweeps at the lengths rate_c blen, and a column
 * of it has the ratios r_jcm and the constant K_jc of §22.  With K_j = max_c K_jc, w_jc = exp(K_jc - K_j), e_cm = exp(lam_m rate_c t):
 *   S_j = sum_c w_jc (1 + sum_m r_jcm e_cm),  N_j = sum_c w_jc rate_c sum_m r_jcm lam_m e_cm,  M_j = sum_c w_jc rate_c^2 sum_m r_jcm lam_m^2 e_cm,
 *   f_u(t) = sum_j [K_j - log K + log S_j],   f_u' = sum_j N_j / S_j,   f_u'' = sum_j [M_j / S_j - (N_j / S_j)^2].
 * f_u(blen[u]) is the tree's log-likelihood under the model for every u.  A branch keeps w_jc and w_jc r_jcm of every column, 4 K
 * doubles, and an evaluation costs 3 K exp per branch and none per column.  With K = 1 every entry computes what its fixed-rate
 * counterpart computes.
 *
 * hu_tree_gamma_loglik: the log-likelihood at blen.  Per category the column values of hu_tree_loglik at the root message (per_cat
 *   [K][cs_len], may be NULL), per column log of the mean of their exp, taken above their maximum (per_col [cs_len], may be NULL),
 *   *ll their sum in serial column order on the host.
 * hu_tree_gamma_branch_scores, hu_tree_gamma_branch_step: hu_tree_branch_scores and hu_tree_branch_step for the objective above; the
 *   same rule of a step (hu_blen_solve), opts->n_capped counts the branches at the Newton cap.
 * These three read opts->k and opts->alpha (0: alpha = 1).
 * hu_tree_gamma_fit: blen [n] in place.  With opts->alpha > 0 it is one fit of the lengths (the rounds of hu_tree_optimize_lengths
 *   over the objective above) at that alpha.  With alpha 0 it starts at alpha = 1, and a pass (a) searches log alpha on
 *   [log HU_GAMMA_ALPHA_MIN, log HU_GAMMA_ALPHA_MAX] with the lengths held, by golden section with HU_GAMMA_SHAPE_EVALS evaluations, each
 *   the up sweeps and the log-likelihood, and takes the best point evaluated if it beats the alpha it has, then (b) fits the lengths with
 *   alpha held.  It stops when a pass gains less than eps_ll, or after max_outer passes.  The log-likelihood never falls.  The report:
 *   alpha_fit, rates, ll_start (at the given lengths and the first alpha), ll_final, n_outer, stop, and per pass (passes, when not NULL,
 *   holds passes_cap entries) alpha, ll and the rounds of its fit.
 * Memory (hu_gamma_need): 64 K n cs_len bytes of messages, n cs_len of rows, 8 (K + 1) cs_len of column values, the scratch of the
 *   step and 1 MB of slack.  The 4 K values of a branch's columns stay in LDS while 32 K cs_len + 72 K + 6 KB fit HU_GAMMA_LDS_BYTES
 *   (four workgroups in a CU's 160 KB: 1085, 541, 269 and 65 columns at K = 1, 2, 4 and 16); beyond that the step runs over slabs of
 *   max(HU_GAMMA_SLAB_MIN, n / 32) branches per launch (n at the most) with 32 K cs_len bytes of scratch per branch of a slab: 1/64 of
 *   the messages on a large tree.  The need is held against blen.mem_budget (when > 0) before anything is allocated, on the host path
 *   too, and on the device against the free memory: HU_ERR_NOMEM names both numbers.  Column windows are not offered: a tree of
 *   gg_97's size needs 391 GB at K = 4 and is refused on one device.
 * hu_gamma_timing: seconds [5] of this thread's last hu_tree_gamma_fit = the shape searches, the full sweeps, the steps, the trial
 *   sweeps with their log-likelihoods, the rest. */
#define HU_GAMMA_ALPHA_MIN 0.05    /* a choice, not a measurement: below it the lowest category's rate underflows any use */
#define HU_GAMMA_ALPHA_MAX 100.0   /* likewise: above it the rates are within a few percent of 1 */
#define HU_GAMMA_SHAPE_EVALS 24    /* of a golden-section search: the bracket of log alpha shrinks from 7.6 to 1.2e-4 */
#define HU_GAMMA_LDS_BYTES 40960   /* of a workgroup of k_gamma_step<true>: a quarter of a CU's 160 KB */
#define HU_GAMMA_SLAB_MIN 1024     /* branches of a launch of k_gamma_step<false> at the least: four workgroups for each of 256 CUs */
enum { HU_GAMMA_CONVERGED = 0, HU_GAMMA_MAX_OUTER = 1, HU_GAMMA_FIXED_ALPHA = 2 };
typedef struct { double alpha, ll; int32_t n_rounds, reserved; } hu_gamma_pass;
typedef struct {
	hu_blen_opts blen;    /* of every fit of the lengths: eps, min_len, max_len, max_rounds, host, device, mem_budget; its rounds are not recorded */
	int32_t k;            /* 4: the categories, 1 to 16 */
	int32_t max_outer;    /* 10: passes at the most */
	double alpha;         /* 0: estimated; above 0: kept at this value */
	double eps_ll;        /* 0.01: a pass that gains less ends the run */
	int32_t sweep_reruns; /* 0; 1: a sweep is K runs of the fixed-rate level kernels in place of the launches over all categories: the same
	                       * bits, for the comparison of profiles/gamma_rate.py */
	int32_t passes_cap;   /* entries of passes */
	hu_gamma_pass* passes;
	/* the report */
	int32_t n_outer, stop;
	double alpha_fit;
	double rates[16];     /* HU_MAX_DGK */
	double ll_start, ll_final;
	int64_t n_capped;     /* hu_tree_gamma_branch_step: branches at the Newton cap; hu_tree_gamma_fit: of all rounds */
} hu_gamma_opts;
int hu_gamma_rates(int32_t K, double alpha, double* rates);
int64_t hu_gamma_need(int32_t n_nodes, int32_t cs_len, int32_t K);
void hu_gamma_default_opts(hu_gamma_opts* o);
int hu_tree_gamma_loglik(const hu_gamma_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* per_col, double* per_cat, double* ll);
int hu_tree_gamma_branch_scores(const hu_gamma_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, const double* t, double* f, double* d1, double* d2);
int hu_tree_gamma_branch_step(hu_gamma_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, double* t_star, double* f, double* d1, double* d2, uint8_t* capped);
int hu_tree_gamma_fit(hu_gamma_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, double* blen, const int8_t* seq,
		const hu_model_desc* model);
int hu_gamma_timing(double* seconds /* [5] */);
/* the phases of a round on the device, one by one and reps times each (profiles/gamma_rate.py): seconds [reps][3] = a full sweep, a step,
 * a trial sweep with its log-likelihood, under opts->k, opts->alpha and opts->sweep_reruns; the first repetition also sends the rows */
int hu_gamma_profile(const hu_gamma_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t reps, double* seconds);

/* ---- hmmufotu-amd-tree --ml-lengths --nni: a hill climb over nearest-neighbour interchanges ----
 * The tree, the model and the limits are those of the branch-length fit above: parent [n], blen [n], seq [n][cs_len], the fixed-rate
 * model only, one device, no column windows.
 *
 * An eligible edge is an edge of the unrooted tree whose two ends have degree three; it is named by its lower end u.  With A < B the
 * children of u (node-id order) there are three rooted cases: parent[u] = p is not the root and has the children {u, C} (the fourth
 * subtree is everything above p, carried over blen[p]); p is the root with the children {u, C, D}, C < D; p is a bifurcating root
 * {u, s} and s has the two children C < D: blen[u] + blen[s] is the one edge, scored from the smaller of u and s.  Leaf edges are not
 * eligible; an edge between two inner nodes one of which has another degree is not either, and is counted (skipped).
 * With a, b, c, d the four subtrees' partial likelihoods carried to the ends of the edge, arrangement 0 is (a.b | c.d), the tree as it
 * stands, 1 is (a.c | b.d), B and C exchanged, and 2 is (b.c | a.d), A and C exchanged.  Each is an objective of the central length t
 * of the form of the branch-length fit, f^q(t) = sum_j [K^q_j + log(1 + sum_k r^q_jk exp(lam_k t))], and is maximised the same way.
 *
 * hu_tree_nni_scores: for the E eligible edges in ascending u, edge_node [E] = u, t_star [E][3] the maximiser of f^q on
 *   [min_len, max_len], f [E][3] = f^q(t_star), f0_at_blen [E] = f^0 at the current central length: the tree's log-likelihood.
 *   edge_cap: the entries the outputs hold (at most the number of inner nodes are needed); *n_edges = E, *skipped the edges at
 *   polytomies.  E = 0 is a success.
 * hu_tree_nni_apply: arrangement q (1 or 2) of the edge of u on the arrays, the central edge set to t (a root-spanning edge splits
 *   t in the old proportion, in halves when the old sum is 0): the exchanged subtrees keep their lengths and take each other's place
 *   in child_off / child_idx (the order of hu_newick_get; child_idx may be NULL).  The root, the node ids and the names stay.  Host.
 * hu_tree_nni_search: parent, blen (and child_idx) in place.  A round fits the lengths (hu_tree_optimize_lengths with opts->blen),
 *   scores all eligible edges and takes as candidates those with gain = max(f^1, f^2) - f^0 > min_gain, each at its own t_star.
 *   No candidate ends the run (local optimum).  The candidates go by gain descending, ties by the smaller u; every one that shares
 *   no end node with one taken before is taken; the taken swaps are applied at once and the tree's log-likelihood is taken from an
 *   up sweep.  If it is not above the fit's, the better half (rounded up) of the set is tried, down to one swap; if that fails too
 *   the run ends (no improving swap).  At most nni_rounds rounds; a last fit follows the last accepted round.  The report: n_rounds,
 *   stop, n_swaps, skipped, ll_start (after the first fit), ll_final, per accepted round (rounds, rounds_cap entries) the trial's ll,
 *   the edges scored, the candidates, the swaps taken at first and those applied, and per applied swap (swaps, swaps_cap triples)
 *   round, u, q.
 * Memory (hu_nni_need): hu_blen_need plus 160 bytes of edge record and outputs per inner node and, when cs_len is above
 *   HU_NNI_LDS_COLS, 72 cs_len bytes of ratios per inner node; held against opts->blen.mem_budget and the free memory as above.
 * hu_nni_timing: seconds [4] of this thread's last hu_tree_nni_search = the fits, the scoring, the trials, the rest.
 * hu_newick_from_arrays: Newick text from parent, the order of children, names (NULL or "" for none) and blen, with the quoting rule
 *   and the 17 significant digits of hu_newick_write; the top node is the root of parent.  Returns as hu_newick_write does.  Host. */
#define HU_NNI_LDS_COLS 483        /* the nine ratios of an edge stay in LDS up to this many columns: 72 cs_len + 6 KB of reduction scratch, four workgroups in a CU's 160 KB */
enum { HU_NNI_LOCAL_OPTIMUM = 0, HU_NNI_NO_SWAP = 1, HU_NNI_MAX_ROUNDS = 2 };
typedef struct { double ll; int32_t scored, candidates, taken, applied; } hu_nni_round;
typedef struct {
	hu_blen_opts blen;    /* of every fit: eps, min_len, max_len, max_rounds, host, device, mem_budget; its rounds are not recorded */
	double min_gain;      /* 1e-3, in units of log-likelihood */
	int32_t nni_rounds;   /* 20 */
	int32_t rounds_cap;   /* entries of rounds */
	hu_nni_round* rounds;
	int32_t* swaps;       /* [swaps_cap][3]: round (from 1), u, q */
	int64_t swaps_cap;
	/* the report */
	int32_t n_rounds, stop;
	int64_t n_swaps, skipped;
	double ll_start, ll_final;
} hu_nni_opts;
void hu_nni_default_opts(hu_nni_opts* o);
int64_t hu_nni_need(int32_t n_nodes, int32_t cs_len);
int hu_tree_nni_scores(const hu_nni_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f, double* f0_at_blen);
int hu_tree_nni_apply(int32_t n_nodes, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t u, int32_t q, double t);
int hu_tree_nni_search(hu_nni_opts* opts, int32_t n_nodes, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const hu_model_desc* model);
int hu_nni_timing(double* seconds /* [4] */);
int64_t hu_newick_from_arrays(int32_t n_nodes, const int32_t* parent, const int32_t* child_off, const int32_t* child_idx, const char* const* names,
		const double* blen, char* buf, int64_t cap);

/* ---- hmmufotu-amd-tree --support: local branch supports of the eligible edges ----
 * The tree, the model, the limits and the eligible edges are those of the NNI search above.  For every eligible edge e, with its three
 * arrangements q each at its own optimum t*_q on [min_len, max_len]:
 *   l^q_j = K^q_j + log D^q_j(t*_q), the log-likelihood of column j, whose sum over j is f^q(t*_q);
 *   alrt_e = 2 (f^0 - max(f^1, f^2)), left to the caller: f is returned;
 *   d^q_j = max(l^q_j - l^0_j, -DBL_MAX) for q = 1, 2.  A column with l^0_j not finite refuses the call: the tree has likelihood 0.
 * Replicate b draws cs_len columns with replacement; w_bj counts the draws of column j.  Draw i is word i % 4 of
 * Philox4x32-10(counter (i / 4, b, 0, 0x53555050), key (seed low word, seed high word)), col = (uint64(word) * cs_len) >> 32: the same
 * for every edge, and the first B' replicates of a run with B are those of a run with B'.  S^q_b = sum_j w_bj d^q_j, serially in
 * ascending j, a multiply and then an add.  Replicate b supports the edge when S^1_b < -eta and S^2_b < -eta, eta = HU_SUPPORT_TIE
 * |f^0(t*_0)|: on a collapsed edge, whose three arrangements are one star, d is rounding noise and the count is 0.  count [E] is the
 * number of supporting replicates, support = count / replicates.
 *
 * hu_support_weights: w [replicates][cs_len], host only.  hu_support_weights_device: the same table from the device's kernel.
 * hu_tree_nni_support: edge_node [E], t_star [E][3], f [E][3] as hu_tree_nni_scores gives them, count [E], and sums [E][B][2] =
 *   (S^1_b, S^2_b) when not NULL: for tests and small inputs.  E = 0 is a success.
 * Memory (hu_support_need): hu_nni_need, the table of weights (2 bytes per column and replicate, the replicates padded to a multiple
 *   of 4), 32 bytes of outputs per inner node and the sums of one launch's edges (at most 16 MB); d lies in LDS up to
 *   HU_SUPPORT_LDS_COLS columns and in the ratio scratch of the scoring beyond.  Held against opts->blen.mem_budget and the free memory.
 * hu_support_timing: seconds [4] of this thread's last hu_tree_nni_support = the sweep, the scoring, the weights, the support kernel. */
#define HU_SUPPORT_TIE 0x1p-40     /* 16 times the measured bar of f, 2^-44 */
#define HU_SUPPORT_LDS_COLS 4736   /* d of an edge stays in LDS up to this many columns: 16 cs_len + 6 KB of reduction scratch, two workgroups in a CU's 160 KB; with one
                                    * workgroup per CU the global scratch was measured faster */
#define HU_SUPPORT_MAX_REPLICATES 100000
typedef struct {
	hu_blen_opts blen;    /* min_len, max_len, device, host, mem_budget are read */
	int32_t replicates;   /* 1,000; 1 .. HU_SUPPORT_MAX_REPLICATES */
	int32_t reserved;
	uint64_t seed;        /* 1 */
} hu_support_opts;
void hu_support_default_opts(hu_support_opts* o);
int hu_support_weights(int32_t cs_len, int32_t replicates, uint64_t seed, uint16_t* w /* [replicates][cs_len] */);
int hu_support_weights_device(int32_t device, int32_t cs_len, int32_t replicates, uint64_t seed, uint16_t* w /* [replicates][cs_len] */);
int64_t hu_support_need(int32_t n_nodes, int32_t cs_len, int32_t replicates);
int hu_tree_nni_support(const hu_support_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t edge_cap, int32_t* n_edges, int64_t* skipped, int32_t* edge_node, double* t_star, double* f,
		int32_t* count, double* sums);
int hu_support_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-tree --ml-lengths --spr: subtree pruning and regrafting ----
 * The tree, the model and the limits are those of the branch-length fit above: parent [n], blen [n], seq [n][cs_len], the fixed-rate
 * model only, one device, no column windows.  All definitions are on the rooted arrays as they stand.
 *
 * A node v is prunable when it is not the root and p = parent[v] is not the root and has exactly the two children {v, s}; g = parent[p].
 * Every other non-root v is not pruned and is counted (skipped): p the root, p a polytomy.  In the pruned tree T' the subtree of v and
 * the node p are lifted out and s hangs on g with the length blen[s] + blen[p].  An edge of T' is named by its lower end w.
 * The targets of v are the edges w of T' whose distance from the edge of s is 1 .. radius; the distance is the number of nodes on the
 * path that joins the two edges, so edges that share a node are at distance 1, and a bifurcating root is a node like any other: its
 * two branches are two targets.  A binary neighbourhood has 2^(d+1) targets at distance d.  The edge of s is distance 0, the position
 * as it stands: the baseline, no move.  The targets come in the order of a depth-first walk from the edge of s: first into the subtree
 * of s, then from g; at a node its children in node-id order, then the edge above it; behind every target what lies beyond it.
 * Regraft at w: p goes into the edge of w, parent[p] = parent'(w), parent[w] = p, the children of p become {w, v}, parent[s] = g.  The
 * edge's length L_w in T' is split in halves between blen[w] and blen[p], blen[s] takes blen[s] + blen[p] and the pendant blen[v]
 * takes t.  Node ids, names and the root stay; in child_idx p takes w's place below parent'(w), s takes p's place below g and w takes
 * s's place below p.  The baseline keeps the real split (blen[s], blen[p]).
 * With x_j the product at the junction of the two sides of the target edge, each carried over its half, and y_j = up[v],
 *   f_w(t) = sum_j log sum_ab pi_a x_a P_ab(t) y_b
 * is an objective of the pendant length of the form of the branch-length fit (three ratios and a K_j per column, the same clamps and
 * -inf rules) and is maximised the same way from blen[v] on [min_len, max_len].  gain_w = f_w(t*_w) - f_s(t*_s): the pendant is at its
 * optimum on both sides.  f_s(blen[v]) is the tree's log-likelihood.  Of the two sides of a target the one away from s is a message of
 * the level sweeps (up[w] where w is no ancestor of p, down[w] where it is; down[p] over the merged length above s); the other one is
 * recomputed without v, one message per step of the walk, as the product of the carried messages of the node's other neighbours.  A
 * node of any degree is walked through.
 *
 * hu_tree_spr_scores: for the P prunable nodes in ascending v: prune_node [P] = v, v_off [P + 1] the CSR offsets of its targets,
 *   base_t [P] = t*_s, base_f [P] = f_s(t*_s), f_at_blen [P] = f_s(blen[v]); per target target_node = w, dist, t_star = t*_w,
 *   f = f_w(t*_w).  node_cap and target_cap: the entries the outputs hold; *n_pruned = P and *n_targets are set before they are held
 *   against the caps, and a call with both caps 0 only counts.  *skipped as above.  P = 0 is a success.
 * hu_tree_spr_apply: the regraft of v at w with the pendant t on the arrays (child_idx may be NULL).  Host.  Refused: a v that is not
 *   prunable, and a w that is no target position: the root, v, p, s (where v hangs) or a node inside v's subtree.  No radius is held.
 * hu_tree_spr_search: parent, blen (and child_idx) in place.  A round fits the lengths (hu_tree_optimize_lengths with opts->blen),
 *   scores every prunable v and takes as candidate the best target of every v (the largest f, ties by the smaller w) when its gain is
 *   above min_gain.  No candidate ends the run (local optimum).  The candidates go by gain descending, ties by the smaller v, then the
 *   smaller w; one is taken when none of {v, p, s, g, w, parent'(w)} and none of the nodes on the path from p to w is marked by one
 *   taken before.  The taken moves are applied at once and the tree's log-likelihood is taken from an up sweep.  If it is not above
 *   the fit's, the better half (rounded up) of the set is tried, down to one move; if that fails too the run ends (no improving
 *   move).  At most spr_rounds rounds; a last fit follows the last accepted round; ll never decreases.  The report: n_rounds, stop,
 *   n_moves, skipped (of the last scoring), ll_start (after the first fit), ll_final, per accepted round (rounds, rounds_cap entries)
 *   the trial's ll, the nodes pruned, the targets scored, the candidates, the moves taken at first and those applied, and per applied
 *   move (moves, moves_cap entries of five) round, v, w_from = s, w_to, dist.
 * Memory (hu_spr_need): hu_blen_need, plus 32 bytes per node, plus 96 bytes of record and outputs per target, at most
 *   min(2^(radius+2) - 3, n) targets per node and HU_SPR_REC_BYTES per launch, plus the scratch of a launch's workgroups: radius
 *   messages of 32 cs_len bytes each and, above HU_BLEN_LDS_COLS columns, 24 cs_len bytes of ratios, HU_SPR_SLAB_BYTES at the most and
 *   one workgroup's at the least.  Launches are cut into slabs of prune nodes that keep within these bounds (opts->slab > 0: at most so
 *   many nodes); the result does not depend on the slab.  Held against opts->blen.mem_budget and the free memory as above.
 * hu_spr_timing: seconds [4] of this thread's last hu_tree_spr_search = the fits, the scoring, the trials, the rest. */
#define HU_SPR_MAX_RADIUS 32
#define HU_SPR_SLAB_BYTES ((int64_t) 1 << 30)
#define HU_SPR_REC_BYTES ((int64_t) 1 << 26)
enum { HU_SPR_LOCAL_OPTIMUM = 0, HU_SPR_NO_MOVE = 1, HU_SPR_MAX_ROUNDS = 2 };
typedef struct { double ll; int64_t targets; int32_t pruned, candidates, taken, applied; } hu_spr_round;
typedef struct {
	hu_blen_opts blen;    /* of every fit: eps, min_len, max_len, max_rounds, host, device, mem_budget; its rounds are not recorded */
	double min_gain;      /* 1e-3, in units of log-likelihood */
	int32_t radius;       /* 5; 1 .. HU_SPR_MAX_RADIUS */
	int32_t spr_rounds;   /* 10 */
	int32_t rounds_cap;   /* entries of rounds */
	int32_t slab;         /* 0: what the bounds allow; > 0: at most this many prune nodes per launch */
	hu_spr_round* rounds;
	int32_t* moves;       /* [moves_cap][5]: round (from 1), v, w_from, w_to, dist */
	int64_t moves_cap;
	/* the report */
	int32_t n_rounds, stop;
	int64_t n_moves, skipped;
	double ll_start, ll_final;
} hu_spr_opts;
void hu_spr_default_opts(hu_spr_opts* o);
int64_t hu_spr_need(int32_t n_nodes, int32_t cs_len, int32_t radius);
int hu_tree_spr_scores(const hu_spr_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t node_cap, int64_t target_cap, int32_t* n_pruned, int64_t* n_targets, int64_t* skipped,
		int32_t* prune_node, int64_t* v_off, double* base_t, double* base_f, double* f_at_blen,
		int32_t* target_node, int32_t* dist, double* t_star, double* f);
int hu_tree_spr_apply(int32_t n_nodes, int32_t* parent, double* blen, const int32_t* child_off, int32_t* child_idx, int32_t v, int32_t w, double t);
int hu_tree_spr_search(hu_spr_opts* opts, int32_t n_nodes, int32_t cs_len, int32_t* parent, double* blen, const int8_t* seq,
		const int32_t* child_off, int32_t* child_idx, const hu_model_desc* model);
int hu_spr_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-tree --ml-lengths --start-tree T --add: new sequences inserted into a start tree ----
 * The tree, the model and the limits are those of the branch-length fit above: parent [n], blen [n], seq [n][cs_len], the fixed-rate
 * model only, one device, no column windows.  All definitions are on the rooted arrays as they stand.
 *
 * A query is a row of the alignment that is no leaf of the tree: qseq [n_query][cs_len] in the codes of seq, numbered in the order
 * given (the program gives them in ascending row of the MSA).  An edge is named by its lower end w, any non-root node.
 * Insert query r at w with the pendant t: two nodes are appended, p = n (inner, unnamed) and v = n + 1 (a leaf with r's row);
 * parent[p] = parent[w], parent[w] = p, parent[v] = p; blen[w] and blen[p] each take half of the old blen[w], blen[v] = t.  In the
 * child lists p takes w's place below parent(w), and the children of p are w, then v.  Existing ids, names and the top node stay.
 * With x_j the product at the junction of up[w] and down[w], each carried over half of blen[w], and y_j the leaf message of r's
 * column (one-hot where the row has a symbol, log pi where it has none),
 *   f_{w,r}(t) = sum_j log sum_ab pi_a x_a P_ab(t) y_b
 * is the log-likelihood of the tree with r inserted at w.  It has the form of the branch-length fit (three ratios and a K_j per
 * column, the same D_j >= DBL_MIN clamp and -inf rules: never a NaN) and is maximised the same way on [min_len, max_len], from the
 * mean length of the tree's non-root branches clipped to the interval.  The score of (w, r) is f_{w,r}(t*).  The junction does not
 * depend on the query and the query's side is a look-up: c_jk = A_jk T[k][s_rj], A_jk = sum_a pi_a x_a U_ak, T[k][s] = sum_b U1_kb
 * y^(s)_b over the five symbols, so an edge's ratios A_jk / A_j0 are computed once for a tile of queries.
 *
 * hu_tree_add_scores: t_star, f [n_query][n_nodes] (may both be NULL) = t* and f(t*) of every (query, edge), the root's entries 0 and
 *   -inf; best_w, best_t, best_f [n_query]: the best edge of every query, the largest f and the smaller w among equals.
 * hu_tree_add_apply: the insertion at w with the pendant t on arrays with room for two more nodes: parent, blen [n + 2], child_off
 *   [n + 3], child_idx [n + 1], the child lists rebuilt by the rule above (both may be NULL).  Host.  Refused: w the root or out of
 *   range, t outside [min_len, max_len].
 * hu_tree_add_search: arrays with room for n + 2 n_query nodes (seq [n + 2 n_query][cs_len], child_off [n + 2 n_query + 1],
 *   child_idx [n + 2 n_query - 1]), updated in place.  The lengths of the start tree are fitted on its own leaves
 *   (hu_tree_optimize_lengths with opts->blen).  Then rounds until no query is left: sweep up and down, score every remaining query
 *   against every edge, per edge take the one query with the largest f among those whose best edge it is (ties: the smaller query),
 *   insert the taken ones in ascending query, which fixes the new ids, and fit the lengths again.  The others wait for the next
 *   round, where they are scored against the grown tree.  Every round inserts at least one query.  query_node [n_query]: the leaf v
 *   of every query.  The report: n_rounds, n_inserted, ll_start (after the first fit), ll_final, per round (rounds, rounds_cap
 *   entries) ll after its fit, the queries scored and inserted, and per insertion (inserts, inserts_cap entries) round, query, v, w,
 *   t*, f.  n_query = 0 is the fit alone.
 * Memory (hu_add_need): hu_blen_need of the final tree plus a launch: per tile of HU_ADD_TILE queries 16 bytes of outputs per node
 *   and query, the queries' rows and records and, above HU_BLEN_LDS_COLS columns, 24 cs_len bytes of ratios per node;
 *   HU_ADD_SLAB_BYTES at the most and one tile at the least.  Launches are cut into slabs of queries that keep within these bounds
 *   (opts->slab > 0: at most so many queries; opts->tile > 0: so many queries per workgroup); the result does not depend on either,
 *   to the bit.  Held against opts->blen.mem_budget and the free memory as above.
 * hu_add_timing: seconds [4] of this thread's last hu_tree_add_search = the sweeps, the scoring, the fits, the rest. */
#define HU_ADD_TILE 16             /* queries of a workgroup of k_add_score */
#define HU_ADD_SLAB_BYTES ((int64_t) 1 << 32)
typedef struct { double ll; int32_t scored, inserted; } hu_add_round;
typedef struct { int32_t round, query, v, w; double t, f; } hu_add_insert;
typedef struct {
	hu_blen_opts blen;    /* of every fit: eps, min_len, max_len, max_rounds, host, device, mem_budget; its rounds are not recorded */
	int32_t slab;         /* 0: what the bounds allow; > 0: at most this many queries per launch */
	int32_t tile;         /* 0: HU_ADD_TILE; > 0: this many queries per workgroup */
	int32_t rounds_cap;   /* entries of rounds */
	int32_t reserved;
	hu_add_round* rounds;
	hu_add_insert* inserts;
	int64_t inserts_cap;
	/* the report */
	int32_t n_rounds, n_inserted;
	double ll_start, ll_final;
} hu_add_opts;
void hu_add_default_opts(hu_add_opts* o);
int64_t hu_add_need(int32_t final_nodes, int32_t cs_len, int32_t n_query);
int hu_tree_add_scores(const hu_add_opts* opts, int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const int8_t* seq,
		const hu_model_desc* model, int32_t n_query, const int8_t* qseq, double* t_star, double* f, int32_t* best_w, double* best_t, double* best_f);
int hu_tree_add_apply(int32_t n_nodes, int32_t* parent, double* blen, int32_t* child_off, int32_t* child_idx, int32_t w, double t, double min_len, double max_len);
int hu_tree_add_search(hu_add_opts* opts, int32_t n_nodes, int32_t cs_len, int32_t n_query, int32_t* parent, double* blen, int8_t* seq,
		int32_t* child_off, int32_t* child_idx, const int8_t* qseq, int32_t* query_node, const hu_model_desc* model);
int hu_add_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-pcoa: the principal coordinates of a distance matrix (PCoA, classical scaling, Gower 1966) ----
 * dist [n][n] row-major with the properties hu_permanova requires (symmetric, finite, non-negative, zero on the diagonal, not all zero;
 * the same code checks them).  With D2_ij = d_ij * d_ij (one rounded product) and J = I - 11'/n:
 *     B      = -1/2 J D2 J                  (Gower's centred matrix; never stored)
 *     B u_a  = lambda_a u_a,  |u_a| = 1,  lambda_1 >= lambda_2 >= ...  (algebraic order)
 *     x_ia   = u_ia * sqrt(lambda_a)        the coordinates, for the k largest lambda_a, all of which must be > 0
 *     prop_a = lambda_a / trace(B),  trace(B) = (1/n) sum_{i<j} D2_ij = SS_T of hu_permanova, by the same code and so the same bits.
 * UniFrac and Bray-Curtis matrices are not Euclidean: B then has negative eigenvalues, the positive ones add up to more than the trace,
 * and prop_a is a share of the trace, not of that sum (which nobody knows without all n eigenvalues).
 * Sign: u_a is flipped so that its entry of largest magnitude (the lowest index on a tie) is positive.
 * resid [k]: res_a = | B u_a - lambda_a u_a |_2, from one more product with the final vectors after the last iteration; by Weyl's theorem
 * an eigenvalue of B lies within res_a of lambda_a, so a result certifies itself.
 * The method is a block subspace iteration with Rayleigh-Ritz on m = min(k + oversample, n - 1) columns (64 at the most), started from
 * Philox4x32-10 (hu_sim_philox): entry (row, col) of the start block is hu_sim_u01(w[1], w[0]) - 1/2 of the counter (row & 0xffffffff,
 * row >> 32, col & 0xffffffff, col >> 32) under the key (seed & 0xffffffff, seed >> 32).  A result is a function of (dist, k, oversample,
 * seed, tol, max_it) and of the path (device or host) alone; the two paths agree within their residuals, not in their bits.  It stops when
 * res_a <= tol * lambda_1 for the k axes kept.  A block with fewer than k positive Ritz values after 3 iterations doubles oversample
 * (0 becomes 8) and starts again; the iterations count on.
 * coords [n][k], eigval [k], resid [k].  opts->host, or device < 0: the host path, one thread, no device needed.
 * HU_ERR_ARG with the reason, before a device is asked for: the matrix refusals of hu_permanova, n < 3, k < 1 or k > n - 1,
 * oversample < 0, min(k + oversample, n - 1) > 64, tol outside (0, 1e-3], max_it < 1.  HU_ERR_NOMEM with the bytes needed and the bytes
 * free when hu_pcoa_need exceeds mem_budget (checked before a device is asked for) or what the device reports free.  HU_ERR_NUMERIC: no
 * convergence within max_it iterations (the worst axis and its residual are named), or fewer than k positive axes ("only P positive
 * axes; k asked": exact, at m = n - 1; or at the block's ceiling of 64 columns, once its Ritz values have settled, "P positive axes found
 * in a settled block of 64 columns, the widest; k asked").
 * hu_pcoa_need: the bytes on the device, with m = min(k + oversample, n - 1), mp = m rounded up to 16, S = hu_pcoa_slabs(n) and
 * c = ceil(n / 256): 8 n^2 for the squares, 8 (S + 4) n mp for the partial products and four blocks, 8 (c + 3) mp^2 + 8 c mp for the
 * partial Gram matrices, the small matrices and the column sums, and 1 MB of slack; -1 on a bad argument.
 * hu_pcoa_slabs: the K slabs of the product kernel, min(8, ceil(n / 128)): a function of n alone; -1 for n < 1.
 * hu_pcoa_timing: of this thread's last call, seconds [6] = copies up, the squares, the product kernel, the small kernels, the host's
 * m x m work, the copy back. */
typedef struct {
	int64_t k;            /* 3: the axes wanted */
	int64_t oversample;   /* 8: columns of the block beyond k */
	double tol;           /* 1e-10 */
	int64_t max_it;       /* 1000 */
	uint64_t seed;        /* 1 */
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t reserved;
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_pcoa_opts;
typedef struct {
	int64_t n, k, m_final, iterations;
	double trace;
	int64_t positive_in_block;
} hu_pcoa_result;
void hu_pcoa_default_opts(hu_pcoa_opts* o);
int hu_pcoa(int device, int64_t n, const double* dist, const hu_pcoa_opts* opts, hu_pcoa_result* out, double* coords /* [n][k] */,
		double* eigval /* [k] */, double* resid /* [k] */);
int64_t hu_pcoa_need(int64_t n, int64_t k, int64_t oversample);
int64_t hu_pcoa_slabs(int64_t n);
int hu_pcoa_timing(double* seconds /* [6] */);

/* ---- hmmufotu-amd-alpha: alpha diversity of the samples of an OTU table, and rarefaction curves ----
 * Column j of counts [n_otu][n_sample] is a sample; its cells n_i are non-negative integers, N = sum n_i, 0 < N < 2^32 (the checks of
 * hu_otu_subset; a sample without reads is refused as hu_unifrac refuses it).
 * Integer statistics, exact, the same on host and device:
 *     S = #{n_i > 0},  F1 = #{n_i = 1},  F2 = #{n_i = 2},  Q = sum n_i^2  (Q <= N^2 < 2^64)
 * Float statistics:
 *     A  = sum over n_i >= 2 of n_i ln n_i
 *     PD = sum of b_k over the kept branches k below which the sample has a read.  The tree, the convention for reads on inner nodes and
 *          for an OTU that is the root, and the branch numbering are hu_unifrac's.  Without a tree (tree == NULL) PD is NaN.
 * Metrics, by hu_alpha_metrics on both paths:
 *     observed = S, singles = F1, doubles = F2
 *     chao1 = S + (double) F1 * (double) (F1 - 1) / (2.0 * (double) (F2 + 1))        (bias-corrected, always defined)
 *     shannon = max(0, ln N - A / N) in nats, exactly 0 when S <= 1
 *     simpson = 1 - (double) Q / ((double) N * (double) N)
 *     goods_coverage = 1 - (double) F1 / (double) N
 *     faith_pd = PD
 * Rarefied draws: the draw (j, m, r), 1 <= m <= N_j, r = 0 .. reps - 1, is column j of hu_otu_subset(counts, m, HU_OTU_UNIFORM,
 * seed + r) (the sum wraps at 2^64), and its metrics are that column's: a definition by names.  m = N_j is the whole sample; for
 * m > N_j the draw does not exist: reads = 0, the integers 0 and every double NaN.  For a fixed (j, r) the kept sets are nested in m
 * (the m smallest (key, t) of one key sequence); the tie rule and key_bits are hu_otu_subset's.
 * hu_alpha: whole_out [n_sample], draws_out [n_sample][n_depth][reps] (may be NULL when n_depth * reps == 0).  depths [n_depth] strictly
 * ascending, each >= 1.  opts->host, or device < 0: the host path, no device needed.  The device path uploads every sample's nonzero cells
 * once and keeps them resident: their prefixes in table order, which numbers the reads as hu_otu_subset does, and for each cell its
 * place in the depth-first row order of hu_unifrac's embedding, in which a draw's cells are kept; draws are processed
 * draw_chunk at a time (0: as many as the memory holds): the cut key of every draw by the radix select of hu_otu_subset, the keys of a
 * (sample, repeat) computed once per pass for up to 8 depths, the kept reads counted into the draw's copy of the sample's nonzero cells
 * (never [n_otu][draws]), one kernel for S, F1, F2, Q, A and one for PD (a presence prefix over the draw's cells and the sample's branch
 * intervals); 40 bytes per draw come back.  S, F1, F2, Q: integer sums.  A: thread x of 256 adds the draw's cells x, x + 256, ... of that order;
 * PD: thread x adds the sample's branch entries x, x + 256, ... (ascending branch number; an absent branch adds +0); the 256 partial sums
 * are then added as a tree: within each 64 v[l] += v[l + d] for d = 32, 16, .. 1, then (w0 + w1) + (w2 + w3).  The host path adds PD in
 * that order (the same bits) and A in ascending cell order (libm's log: the same value within DESIGN §30's bound, not the same bits).
 * No result depends on chunk, draw_chunk, the grid or the device.
 * HU_ERR_ARG with the reason, before a device is asked for: the cell and total checks of hu_otu_subset, the tree checks of hu_unifrac,
 * a sample without reads, a depth of 0, depths not strictly ascending, reps < 0, reps == 0 with depths given, n_depth * reps * n_sample
 * above 2^31, key_bits, chunk, draw_chunk or mem_budget out of range.  HU_ERR_NOMEM naming both numbers when hu_alpha_need for the
 * draw_chunk (for one draw when it is 0) exceeds mem_budget (checked before a device is asked for) or what the device reports free.
 * hu_alpha_need: the bytes on the device for n_draw resident draws of a table with n_sample samples, n_cell nonzero cells, n_entry
 * branch entries (pairs of a sample and a kept branch below which it has a nonzero cell), max_nnz the most nonzero cells of a sample
 * and max_chunk the largest ceil(N_j / chunk):
 *     32 n_sample + 4 (2 n_cell + n_sample) + 16 n_entry + n_draw (1136 + 4 max_nnz + 24 max_chunk) + 2^20
 * (the samples, their prefixes and places, the entries; per draw its record, selection state, histogram, result, group, cells, tie counts and
 * chunk list; 1 MB of slack); -1 on a negative argument.  The whole samples count as draws.
 * hu_alpha_sizes: out [6] = n_cell, n_entry, max_nnz, max_chunk, the draws of the call (n_sample whole ones included), the kept
 * branches B: what hu_alpha_need takes, for the same arguments and refusals as hu_alpha.  Host only.
 * hu_alpha_metrics: the metrics of a record from its reads, S, F1, F2, Q, A and PD.
 * hu_alpha_curve: x [n] -> *mean = (x_0 + x_1 + ...) / n added in ascending order, *sd = sqrt(sum (x - mean)^2 / (n - 1)) in the same
 * order, NaN for n == 1; HU_ERR_ARG for n < 1.
 * hu_alpha_timing: of this thread's last device call, seconds [6] = copies up, select, take, metrics, PD, copy back. */
typedef struct {
	int32_t host;         /* 0; 1: the host path, no device needed */
	int32_t chunk;        /* 16384: reads per workgroup */
	int32_t key_bits;     /* 64; below 64 keys tie: for the tie tests only */
	int32_t reserved;
	int64_t draw_chunk;   /* 0: as many draws resident as the memory holds */
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_alpha_opts;
typedef struct {
	uint64_t reads;       /* N of the column: N_j, or m for a draw; 0: the draw does not exist */
	uint64_t S, F1, F2, Q;
	double A, PD;
	double observed, singles, doubles, chao1, shannon, simpson, goods_coverage, faith_pd;
} hu_alpha_rec;
void hu_alpha_default_opts(hu_alpha_opts* o);
int hu_alpha(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, uint64_t seed, const hu_alpha_opts* opts, hu_alpha_rec* whole_out, hu_alpha_rec* draws_out);
int64_t hu_alpha_need(int64_t n_sample, int64_t n_cell, int64_t n_entry, int64_t max_nnz, int64_t max_chunk, int64_t n_draw);
int hu_alpha_sizes(const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		int64_t n_depth, const uint64_t* depths, int64_t reps, const hu_alpha_opts* opts, int64_t* out /* [6] */);
void hu_alpha_metrics(hu_alpha_rec* r);
int hu_alpha_curve(int64_t n, const double* x, double* mean, double* sd);
int hu_alpha_timing(double* seconds /* [6] */);

/* ---- hmmufotu-amd-diffabund: which OTUs differ between the sample groups? (Kruskal-Wallis by permutation) ----
 * counts [n_otu][n_sample] row-major, finite and non-negative.  group [n_sample]: a label g_j in 0 .. a-1 per sample, n_g the group
 * sizes, N = n_sample.  Per OTU o:
 *   values      rank_by 0 (fraction): x_j = counts[o][j] / total_j, one rounded division, total_j the column sum added in ascending OTU
 *               order; rank_by 1 (count): x_j = counts[o][j].
 *   ranks       doubled mid-ranks, integers: r2_j = 2 #{k : x_k < x_j} + #{k : x_k == x_j} + 1; centred e_j = r2_j - (N + 1), so
 *               sum_j e_j = 0, and every zero cell has the same e_z.
 *   group sums  C_g = sum_{j in g} e_j = n_g e_z + D_g, D_g = the sum of e_j - e_z over the cells of g above 0: only those are visited.
 *   T           the integer sum_g C_g^2 (L / n_g), L = lcm(n_0 .. n_{a-1}), in unsigned 128-bit arithmetic on both paths.  A permutation
 *               moves labels and keeps sizes, so L and the tie correction are constant per OTU and Kruskal-Wallis' H is monotone in T:
 *               no floating-point operation decides a tie.
 *   p           (1 + #{pi : T(pi) >= T(observed)}) / (perms + 1); count_ge is the count.
 *   H           plain IEEE operations in this order, no fma: x = (double) T_hi * 2^64 + (double) T_lo,
 *               tc = 1 - (double) sum_ties (t^3 - t) / (double) (N^3 - N), H = ((x / (double) L) * (3.0 / ((double) N * (double) (N + 1)))) / tc:
 *               Kruskal-Wallis with the tie correction, for a == 2 the two-sided Wilcoxon rank-sum test; non-decreasing in T.
 *   p_maxT      single-step maxT (Westfall-Young): M(pi) = the maximum over the tested OTUs of H_o(T_o(pi)),
 *               p_maxT_o = (1 + #{pi : M(pi) >= H_o(observed)}) / (perms + 1).
 *   q           Benjamini-Hochberg on the p of the m tested OTUs: sorted ascending, stable by OTU order, q = (p * (double) m) / (double) j
 *               for the j-th (1-based), then the running minimum from the end, capped at 1.
 *   best        the group with the largest C_g / n_g, compared by integer cross-multiplication; the first group wins a tie.
 *   not tested  an OTU whose cells all tie (tc == 0: all zero, or all equal) or with fewer than min_prevalence nonzero cells: tested 0,
 *               best -1, NaN in H, p, p_maxT and q; it takes no part in M or in m.
 * Permutation p is the labelling hu_permanova_labels(n, group, seed, p) gives.  The host path (opts->host, or device < 0: one thread, no
 * device needed) gives the same bits in every field and in maxstat_perm_out [perms] (may be NULL), which receives M(pi).
 * HU_ERR_ARG with the reason, before a device is asked for: n_sample < 3 or > 16,384, a negative label, labels not dense in 0 .. a-1,
 * a < 2, a > 64, a > n-1, L >= 2^64 (with the group sizes), perms < 1 or > 10^7, chunk < 0, min_prevalence < 0, rank_by not 0 or 1, a
 * negative or non-finite cell, a sample without reads under rank_by 0, every OTU untested.  HU_ERR_NOMEM with the bytes needed and the
 * bytes free when hu_diffabund_need exceeds mem_budget (checked before a device is asked for) or what the device reports free.
 * chunk: permutations per launch; 0: the largest multiple of 256 that fits, 16,384 at the most and never more than perms.
 * hu_diffabund_ranks: host only, r2_out [n_otu][n_sample] the doubled mid-ranks.
 * hu_diffabund_need: the bytes on the device; n_otu and n_cell are the tested OTUs and their cells above 0 (the whole table's bound them).
 * With c = chunk rounded up to 256 and b = (n_otu + 63) / 64: 4 n_cell for the cells, n_sample c for the labels, 8 b c for the partial
 * maxima, 8 c for the maxima, n_sample + 16 a for the tables, 52 n_otu + 8 for the rows and 1 MB of slack; -1 on a bad argument.
 * hu_diffabund_timing: of this thread's last device call, seconds [4] = copies up, shuffles, sums, finish and copy back. */
typedef struct {
	int64_t perms;          /* 999 */
	uint64_t seed;          /* 1 */
	int32_t host;           /* 0; 1: the host path, no device needed */
	int32_t rank_by;        /* 0: fraction of the sample's reads; 1: count */
	int64_t min_prevalence; /* 1 */
	int64_t chunk;          /* 0: chosen from the sizes and the memory */
	int64_t mem_budget;     /* 0: what the device reports free */
} hu_diffabund_opts;
typedef struct {
	int32_t tested, best;
	int64_t prevalence;
	uint64_t T_hi, T_lo;
	int64_t count_ge;
	double H, p, p_maxT, q;
} hu_diffabund_rec;
void hu_diffabund_default_opts(hu_diffabund_opts* o);
int hu_diffabund(int device, int64_t n_otu, int64_t n_sample, const double* counts, const int32_t* group, const hu_diffabund_opts* opts,
		hu_diffabund_rec* rec_out /* [n_otu] */, double* maxstat_perm_out /* [perms] or NULL */);
int hu_diffabund_ranks(int64_t n_otu, int64_t n_sample, const double* counts, int32_t rank_by, int32_t* r2_out /* [n_otu][n_sample] */);
int64_t hu_diffabund_need(int64_t n_sample, int64_t a, int64_t n_otu, int64_t n_cell, int64_t chunk);
int hu_diffabund_timing(double* seconds /* [4] */);

/* ---- hmmufotu-amd-unifrac --rarefy: the distances averaged over rarefied draws ----
 * The inputs of hu_unifrac, a depth M >= 1, R >= 1 repeats and a 64-bit seed.
 * Kept samples: the columns with N_j >= M, in table order, S' of them; kept_out [n_sample] (may be NULL) is 1 for them and 0 for the
 *     dropped ones (N_j < M).  Fewer than 2 kept samples are refused.
 * Draw r (r = 0 .. R-1) is the table X_r: column j of X_r is column j of hu_otu_subset(counts, M, HU_OTU_UNIFORM, seed + r) of the
 *     original table (the Philox key takes the original column index, so a dropped column does not renumber the others; seed + r wraps
 *     at 2^64): hu_alpha's draw (j, M, r).  A sample with N_j == M is itself in every draw.  X_r keeps every row, empty ones too.
 * D_r is hu_unifrac of X_r restricted to the kept columns, with the same otu_node, tree, method and alpha, and the slab L = opts->slab
 *     or hu_unifrac_default_slab(S', B) when that is 0; B depends on the ids alone, so every draw has the same.  A branch below which
 *     neither sample has a read adds +0 to every sum: D_r has the bits hu_unifrac returns for that table and that L, device against
 *     device and host against host.
 * Result: mean_out [S'][S'] and sd_out [S'][S'] by Welford's recurrence in ascending r, every operation rounded on its own:
 *     mean = 0, M2 = 0; for r = 1 .. R with x = D_{r-1}[i][j]:  d = x - mean;  mean = mean + d / r;  M2 = M2 + d * (x - mean)
 *     sd = sqrt(M2 / (R - 1)), NaN for R == 1.  The diagonal is exactly 0 in both, [j][i] is the stored copy of [i][j].
 *     draws_out [R][S'][S'] (may be NULL) receives every D_r.
 * All six methods; HU_UF_BRAY_CURTIS and HU_UF_JACCARD on the identity tree (tree == NULL).  Uniform draws only.  No PD: hu_alpha has it.
 * opts->host, or device < 0: the host path (hu_otu_subset's host selection, hu_unifrac's host path per draw, the same recurrence): the
 * same bits as the device for every method but HU_UF_GENERALIZED with 0 < alpha < 1, where the two agree as hu_unifrac's paths do.
 * The device path uploads the table once, as hu_alpha does (every sample's nonzero cells), and no draw's table comes back: per chunk of
 * draw_chunk repeats the select / ties / take kernels of hu_alpha draw every kept sample, one kernel turns a (sample, repeat)'s counters
 * into its column of P_r [B][Sp] (an integer prefix over the counters, one rounded division per branch entry), hu_unifrac's pair kernel
 * runs over (tile, slab, draw) in one launch, and one kernel adds a draw's slabs in ascending order, divides and applies the recurrence,
 * the draws in ascending r.  No atomics in the floating-point path.  No result depends on draw_chunk, chunk, the grid or the device.
 * HU_ERR_ARG with the reason, before a device is asked for: whatever hu_unifrac and hu_alpha refuse of the table, the tree and the
 * options, M == 0, R < 1 or R > 100,000, fewer than 2 kept samples (the message gives the largest M that keeps 2), a NULL mean_out or
 * sd_out.  HU_ERR_NOMEM with both numbers when hu_unifrac_rarefied_need for draw_chunk (for 1 when it is 0) exceeds mem_budget (checked
 * before a device is asked for) or what the device reports free.
 * hu_unifrac_rarefied_need: the bytes on the device, with Sp = 64 ceil(n_kept / 64), tiles = hu_unifrac's and slabs = ceil(n_branch / slab):
 *     32 n_sample + 4 (2 n_cell + n_sample) + 20 n_entry + 8 n_branch                          the resident table, entries, lengths
 *   + draw_chunk (n_kept (1096 + 4 max_nnz + 24 max_chunk) + 8 n_branch Sp + 65536 slabs tiles)  select state, counters, P, partial sums
 *   + (want_draws ? draw_chunk : 0) 8 n_kept^2 + 16 n_kept^2 + 2^20                            the D_r of a chunk, mean and M2, slack
 * -1 on a negative argument or slab < 1.
 * hu_unifrac_rarefied_sizes: host only, for the arguments and refusals of hu_unifrac_rarefied: out [8] = n_kept, n_cell, n_entry, max_nnz,
 * max_chunk, n_branch, the slab L, the largest M that keeps 2 samples.
 * hu_unifrac_rarefied_timing: of this thread's last device call, seconds [6] = copies up, draws, embedding, pair kernels, accumulate,
 * copy back; resident_draws (may be NULL) receives the draws that were resident at once. */
typedef struct {
	int32_t method;       /* HU_UF_WEIGHTED */
	int32_t host;         /* 0; 1: the host path, no device needed */
	double alpha;         /* 0.5; read by HU_UF_GENERALIZED only */
	int64_t slab;         /* 0: hu_unifrac_default_slab(S', B) */
	int32_t chunk;        /* 16384: reads per workgroup of the draw kernels */
	int32_t key_bits;     /* 64; below 64 keys tie: for the tie tests only */
	int64_t draw_chunk;   /* 0: as many draws resident as the memory holds */
	int64_t mem_budget;   /* 0: what the device reports free */
} hu_unifrac_rarefied_opts;
#define HU_UFR_MAX_REPS 100000
void hu_unifrac_rarefied_default_opts(hu_unifrac_rarefied_opts* o);
int hu_unifrac_rarefied(int device, const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, uint64_t seed, const hu_unifrac_rarefied_opts* opts, uint8_t* kept_out /* [n_sample] or NULL */,
		double* mean_out /* [S'][S'] */, double* sd_out /* [S'][S'] */, double* draws_out /* [reps][S'][S'] or NULL */);
int hu_unifrac_rarefied_sizes(const hu_unifrac_tree* tree, int64_t n_otu, int64_t n_sample, const int32_t* otu_node, const double* counts,
		uint64_t depth, int64_t reps, const hu_unifrac_rarefied_opts* opts, int64_t* out /* [8] */);
int64_t hu_unifrac_rarefied_need(int64_t n_sample, int64_t n_kept, int64_t n_cell, int64_t n_entry, int64_t max_nnz, int64_t max_chunk,
		int64_t n_branch, int64_t slab, int64_t draw_chunk, int32_t want_draws);
int hu_unifrac_rarefied_timing(double* seconds /* [6] */, int64_t* resident_draws);

#ifdef __cplusplus
}
#endif
#endif /* HMMUFOTU_AMD_H_ */
