// hmmufotu-sim without its per-site loop, host only: the generator's known-answer entry, the rejection loop that
// chooses branch, branch point and columns of every read (src/hmmufotu-sim.cpp:351-380), and the description of a read's FASTA record
// (:413-416).  The sites themselves are drawn on the device (hu_sim_reads, hu_kern_sim.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "hu_common.h"
#include "hu_sim_rng.h"

extern "C" int hu_sim_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) try {
	if(!counter || !key || !out) { hu_set_error("hu_sim_philox: null argument"); return HU_ERR_ARG; }
	hu_philox4x32_10(counter, key, out);
	return HU_OK;
} catch(...) { return hu_catch_all("hu_sim_philox"); }

extern "C" void hu_sim_default_opts(hu_sim_opts* o) {
	if(!o) return;
	/* DEFAULT_MAX_DIST .. DEFAULT_MAX_SIZE, src/hmmufotu-sim.cpp:56-60 */
	o->max_dist = INFINITY; o->mean_size = 500; o->sd_size = 30; o->min_size = 0; o->max_size = 0;
	o->n_regions = 0; o->regions = nullptr;
}

extern "C" int hu_sim_region_ok(int32_t s, int32_t e, int32_t cs_len) { return 0 <= s && s < e && e < cs_len; }

/* the draws of attempt `a`: counter (block, a & 0xffffffff, a >> 32, 1) — word 3 sets them apart from the sites' draws, which have 0 there */
namespace {
struct Draws {
	uint32_t key[2]; uint64_t a;
	void block(uint32_t b, uint32_t w[4]) const { const uint32_t c[4] = {b, (uint32_t) a, (uint32_t)(a >> 32), 1u}; hu_philox4x32_10(c, key, w); }
};
inline int64_t pick(double u, int64_t count) { const int64_t i = (int64_t)(u * (double) count); return i < count ? i : count - 1; }
}

extern "C" int hu_sim_plan(int32_t n_nodes, int32_t cs_len, const int32_t* parent, const double* blen, const double* height, const hu_sim_opts* o,
		uint64_t seed, int64_t* attempt, int64_t n, int32_t* node, double* rc, int32_t* start, int32_t* end) try {
	const char* fn = "hu_sim_plan";
	if(n_nodes < 2 || cs_len < 1 || !parent || !blen || !height || !o || !attempt || *attempt < 0 || n < 0 || (n > 0 && (!node || !rc || !start || !end)) ||
			o->n_regions < 0 || (o->n_regions > 0 && !o->regions)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	/* the checks of src/hmmufotu-sim.cpp:208-223, for a caller that is not the program */
	if(!(o->mean_size > 0) || !(o->sd_size > 0) || !(o->min_size >= 0) || !(o->max_size >= 0 && o->max_size >= o->min_size)) { hu_set_error("%s: sizes: mean %g, sd %g, min %g, max %g", fn, o->mean_size, o->sd_size, o->min_size, o->max_size); return HU_ERR_ARG; }
	/* node_dist: weight 1, or 0 for a node higher than max_dist (:337-344); the root keeps its weight and is redrawn (:355-356) */
	std::vector<int32_t> allowed;
	bool anyBranch = false;
	for(int32_t i = 0; i < n_nodes; ++i) {
		if(parent[i] >= n_nodes) { hu_set_error("%s: parent of node %d out of range", fn, i); return HU_ERR_ARG; }
		if(!(height[i] > o->max_dist)) { allowed.push_back(i); anyBranch |= parent[i] >= 0; }
	}
	if(!anyBranch) { hu_set_error("%s: no node below the root is within %g of a leaf: the reference would draw for ever", fn, o->max_dist); return HU_ERR_ARG; }
	/* myLoci (:294-308): start + 1, end of every BED line inside the consensus; a line that ends AT cs_len is dropped too, the reference
	 * would read column cs_len of the messages for it */
	std::vector<int32_t> loci;
	for(int64_t i = 0; i < o->n_regions; ++i) if(hu_sim_region_ok(o->regions[2 * i], o->regions[2 * i + 1], cs_len)) { loci.push_back(o->regions[2 * i] + 1); loci.push_back(o->regions[2 * i + 1]); }
	const int64_t nLoci = (int64_t) loci.size() / 2;
	const double lenMax = 2147483647.0;
	const int minLen = (int) std::min(o->min_size, lenMax), maxLen = (int) std::min(o->max_size, lenMax);
	if(nLoci == 0 && minLen >= cs_len) { hu_set_error("%s: no read of %d + 1 columns fits a consensus of %d", fn, minLen, cs_len); return HU_ERR_ARG; }
	Draws dr; dr.key[0] = (uint32_t)(seed & 0xffffffffu); dr.key[1] = (uint32_t)(seed >> 32); dr.a = (uint64_t) *attempt;
	const int64_t maxTries = 10000000;     /* per read: a plan that cannot be drawn ends with a message, not with a loop */
	for(int64_t r = 0; r < n; ++r) {
		int64_t tries = 0;
		for(;; ++dr.a) {
			if(++tries > maxTries) { hu_set_error("%s: read %lld: no acceptable draw in %lld attempts (max_dist %g, sizes %g .. %g of %d columns)", fn, (long long) r, (long long) maxTries, o->max_dist, o->min_size, o->max_size, cs_len); *attempt = (int64_t) dr.a; return HU_ERR_ARG; }
			uint32_t w[4];
			dr.block(0, w);
			const int32_t c = allowed[(size_t) pick(hu_sim_u01(w[0], w[1]), (int64_t) allowed.size())];
			if(parent[c] < 0) continue;                                   /* no parent branch available */
			const double v = blen[c], x = hu_sim_u01(w[2], w[3]);
			if(height[c] + v * x > o->max_dist) continue;                 /* too far from any leaf */
			int64_t s, e;
			dr.block(1, w);
			if(nLoci == 0) {
				s = pick(hu_sim_u01(w[0], w[1]), cs_len);                   /* uniform_smallint(0, csLen - 1) */
				dr.block(2, w);
				/* normal_distribution(mean, sd) by Box and Muller; 1 - u lies in (0, 1] */
				const double z = std::sqrt(-2.0 * std::log(1.0 - hu_sim_u01(w[0], w[1]))) * std::cos(6.283185307179586476925 * hu_sim_u01(w[2], w[3]));
				int len = (int) std::max(-lenMax, std::min(lenMax, o->mean_size + o->sd_size * z));     /* int len = size_dist(rng) */
				if(len < o->min_size) len = minLen;
				if(o->max_size > 0 && len > o->max_size) len = maxLen;
				if(len < 0) continue;                                       /* the reference would write an empty record */
				e = s + len;                                                /* len + 1 columns: the reference's loop is inclusive */
				if(!(e < cs_len)) continue;                                 /* outside consensus range */
			}
			else { const int64_t i = pick(hu_sim_u01(w[0], w[1]), nLoci); s = loci[(size_t) 2 * i]; e = loci[(size_t) 2 * i + 1]; }
			node[r] = c; rc[r] = x; start[r] = (int32_t) s; end[r] = (int32_t) e;
			++dr.a;
			break;
		}
	}
	*attempt = (int64_t) dr.a;
	return HU_OK;
} catch(...) { return hu_catch_all("hu_sim_plan"); }

extern "C" int64_t hu_sim_description(int32_t c, int32_t p, const char* taxon_c, const char* taxon_p, double rc, int32_t start, int32_t end, int64_t seq_len,
		char* out, int64_t cap) try {
	if(!taxon_c || !taxon_p || (cap > 0 && !out)) { hu_set_error("hu_sim_description: null argument"); return HU_ERR_ARG; }
	char num[64];
	snprintf(num, sizeof num, "%.17g", rc);     /* boost::lexical_cast<string>(double): 17 significant digits, general format */
	const bool near = rc <= 0.5;
	const std::string d = "branchID=" + std::to_string(c) + "->" + std::to_string(p) + ";taxonID=" + std::to_string(near ? c : p) + ";taxonName=\"" + (near ? taxon_c : taxon_p)
		+ "\";branchPoint=" + num + ";csStart=" + std::to_string(start) + ";csEnd=" + std::to_string(end) + ";seqLen=" + std::to_string(seq_len) + ";";
	if(cap > 0) { const size_t k = std::min<size_t>(d.size(), (size_t) cap - 1); memcpy(out, d.data(), k); out[k] = 0; }
	return (int64_t) d.size();
} catch(...) { return hu_catch_all("hu_sim_description"); }
