// The host half of hmmufotu-amd-tree: the checks, the host path of the pair counts, the distances and neighbour
// joining, and the Newick writer.  Plain C++ with no HIP headers (tests/san/nj_driver.cpp builds it alone).  The host path of hu_nj
// restates the device's order, one step for one kernel of hu_kern_nj.h, with the rules of hu_tree_nj.h that both sides compile.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "hu_tree_nj.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

extern "C" void hu_nj_default_opts(hu_nj_opts* o) { if(o) { o->host = 0; o->reserved = 0; o->mem_budget = 0; } }

int hu_dist_check(const char* fn, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat) {
	if(n < 2 || n > HU_NJ_MAX_N) { hu_set_error("%s: %lld rows: between 2 and %d are taken", fn, (long long) n, HU_NJ_MAX_N); return HU_ERR_ARG; }
	if(cs_len < 1 || cs_len > 65535) { hu_set_error("%s: %lld columns: between 1 and 65535 are taken", fn, (long long) cs_len); return HU_ERR_ARG; }
	if(!rows) { hu_set_error("%s: null rows", fn); return HU_ERR_ARG; }
	if(dist_type < HU_DIST_PDIST || dist_type > HU_DIST_TN93) { hu_set_error("%s: unknown distance type %d", fn, dist_type); return HU_ERR_ARG; }
	if(dist_type >= HU_DIST_F81) {
		if(!pi) { hu_set_error("%s: the distance type needs the base frequencies", fn); return HU_ERR_ARG; }
		for(int b = 0; b < 4; ++b) if(!(pi[b] > 0) || !std::isfinite(pi[b])) { hu_set_error("%s: base frequency %d is %g", fn, b, pi[b]); return HU_ERR_ARG; }
	}
	if(!(sat >= 0) || !std::isfinite(sat)) { hu_set_error("%s: the distance of a saturated pair must be positive, or 0 for twice the largest", fn); return HU_ERR_ARG; }
	const size_t tot = (size_t) n * (size_t) cs_len;
	for(size_t e = 0; e < tot; ++e) if(rows[e] > 3) {
		hu_set_error("%s: row %zu, column %zu holds the code %d: 0 to 3, or a negative one for no symbol", fn, e / (size_t) cs_len, e % (size_t) cs_len, (int) rows[e]); return HU_ERR_ARG; }
	return HU_OK;
}

static inline void pair_counts(const int8_t* a, const int8_t* b, int64_t L, int32_t* c) {
	int32_t N = 0, PR = 0, PY = 0, Q = 0;
	for(int64_t k = 0; k < L; ++k) {
		const int x = a[k], y = b[k];
		if(x < 0 || y < 0) continue;
		++N;
		if(x == y) continue;
		if(((x ^ y) & 1) != 0) ++Q;                /* bit 0 separates A, G from C, T */
		else if((x & 1) == 0) ++PR; else ++PY;
	}
	c[0] = N; c[1] = PR; c[2] = PY; c[3] = Q;
}

void hu_dist_host_counts(int64_t n, int64_t cs_len, const int8_t* rows, int32_t* counts) {
	for(int64_t i = 0; i < n; ++i) for(int64_t j = i; j < n; ++j) {
		int32_t c[4];
		pair_counts(rows + i * cs_len, rows + j * cs_len, cs_len, c);
		memcpy(counts + (i * n + j) * 4, c, sizeof(c)); memcpy(counts + (j * n + i) * 4, c, sizeof(c));
	}
}

int hu_dist_host(const char* fn, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, double* D, int64_t* n_sat) {
	int64_t nSat = 0; double mx = -1.0;
	for(int64_t i = 0; i < n; ++i) {
		D[i * n + i] = 0.0;
		for(int64_t j = i + 1; j < n; ++j) {
			int32_t c[4]; int s = 0;
			pair_counts(rows + i * cs_len, rows + j * cs_len, cs_len, c);
			double d = hu_sub_dist(dist_type, pi, c[0], c[1], c[2], c[3], &s);
			if(s) { ++nSat; d = sat > 0 ? sat : INFINITY; }
			else if(d > mx) mx = d;
			D[i * n + j] = d; D[j * n + i] = d;
		}
	}
	if(n_sat) *n_sat = nSat;
	if(nSat > 0 && !(sat > 0)) {
		if(mx < 0) { hu_set_error("%s: every pair of rows is saturated: no finite distance to scale from, give one", fn); return HU_ERR_ARG; }
		const double fill = 2 * mx;
		for(int64_t e = 0; e < n * n; ++e) if(std::isinf(D[e])) D[e] = fill;
	}
	return HU_OK;
}

int hu_nj_check(const char* fn, int64_t n, const double* D) {
	if(n < 3 || n > HU_NJ_MAX_N) { hu_set_error("%s: %lld nodes: between 3 and %d are taken", fn, (long long) n, HU_NJ_MAX_N); return HU_ERR_ARG; }
	if(!D) { hu_set_error("%s: null matrix", fn); return HU_ERR_ARG; }
	for(int64_t i = 0; i < n; ++i) {
		if(D[i * n + i] != 0.0) { hu_set_error("%s: the diagonal holds %g at %lld", fn, D[i * n + i], (long long) i); return HU_ERR_ARG; }
		for(int64_t j = i + 1; j < n; ++j) {
			const double a = D[i * n + j], b = D[j * n + i];
			if(!std::isfinite(a)) { hu_set_error("%s: the distance of %lld and %lld is not finite", fn, (long long) i, (long long) j); return HU_ERR_ARG; }
			if(a != b) { hu_set_error("%s: the matrix is not symmetric at %lld and %lld", fn, (long long) i, (long long) j); return HU_ERR_ARG; }
		}
	}
	return HU_OK;
}

/* the sum of row `row` over the slots [0, r): blocks of HU_NJ_SUM_BLOCK in ascending order, then the block sums in ascending order (k_nj_rowsum) */
static double row_sum(const double* D, int64_t n, int64_t row, int64_t r) {
	double tot = 0.0;
	for(int64_t b0 = 0; b0 < r; b0 += HU_NJ_SUM_BLOCK) {
		const int64_t b1 = b0 + HU_NJ_SUM_BLOCK < r ? b0 + HU_NJ_SUM_BLOCK : r;
		double s = 0.0;
		for(int64_t k = b0; k < b1; ++k) s += D[row * n + k];
		tot += s;
	}
	return tot;
}

void hu_nj_host_run(int64_t n, double* D, int32_t* join, double* len, int32_t* last3, double* last_len3) {
	std::vector<double> R((size_t) n);
	std::vector<int32_t> id((size_t) n);
	for(int64_t i = 0; i < n; ++i) { R[(size_t) i] = row_sum(D, n, i, n); id[(size_t) i] = (int32_t) i; }
	int64_t r = n;
	for(int64_t t = 0; t < n - 3; ++t, --r) {
		/* pick (k_nj_pick, k_nj_winner) */
		double bq = INFINITY; int32_t bi = INT32_MAX, bj = INT32_MAX;
		for(int64_t i = 0; i < r; ++i) {
			const double Ri = R[(size_t) i];
			const double* row = D + i * n;
			for(int64_t j = i + 1; j < r; ++j) {
				const double q = hu_nj_q(r, row[j], Ri, R[(size_t) j]);
				if(hu_nj_less(q, (int32_t) i, (int32_t) j, bq, bi, bj)) { bq = q; bi = (int32_t) i; bj = (int32_t) j; }
			}
		}
		if(bi == INT32_MAX) { bi = 0; bj = 1; }                           /* every Q is not a number (sums beyond the doubles): still a tree */
		const int64_t i = bi, j = bj, last = r - 1;
		const double dij = D[i * n + j];
		hu_nj_lengths(r, dij, R[(size_t) i], R[(size_t) j], &len[2 * t], &len[2 * t + 1]);
		join[2 * t] = id[(size_t) i]; join[2 * t + 1] = id[(size_t) j];
		id[(size_t) i] = (int32_t)(n + t);
		/* the new node in slot i (k_nj_update) */
		for(int64_t k = 0; k < r; ++k) {
			if(k == i || k == j) continue;
			const double dik = D[i * n + k], djk = D[j * n + k];
			const double duk = hu_nj_duk(dik, djk, dij);
			R[(size_t) k] = hu_nj_rk(R[(size_t) k], dik, djk, duk);
			D[i * n + k] = duk; D[k * n + i] = duk;
		}
		/* the last slot into slot j (k_nj_move) */
		if(j != last) {
			for(int64_t k = 0; k < last; ++k) {
				if(k == j) { D[j * n + j] = 0.0; continue; }
				const double v = D[last * n + k];
				D[j * n + k] = v; D[k * n + j] = v;
			}
			R[(size_t) j] = R[(size_t) last]; id[(size_t) j] = id[(size_t) last];
		}
		/* R of the new node (k_nj_rowsum) */
		R[(size_t) i] = row_sum(D, n, i, r - 1);
	}
	/* the end (k_nj_end): r == 3 */
	for(int s = 0; s < 3; ++s) last3[s] = id[(size_t) s];
	hu_nj_last3(D[1], D[2], D[n + 2], last_len3);
}

extern "C" int64_t hu_nj_newick(int64_t n, const char* const* names, const int32_t* join, const double* len, const int32_t* last3, const double* last_len3,
		char* buf, int64_t cap) try {
	const char* fn = "hu_nj_newick";
	if(n < 3 || n > 0x3fffffff || !names || (n > 3 && (!join || !len)) || !last3 || !last_len3 || (cap > 0 && !buf)) { hu_set_error("%s: bad argument", fn); return HU_ERR_ARG; }
	const int64_t tot = 2 * n - 3;                                     /* nodes below the top node */
	std::vector<std::string> label((size_t) n);
	for(int64_t i = 0; i < n; ++i) {
		const char* s = names[i];
		if(!s || !*s) { hu_set_error("%s: leaf %lld has no name", fn, (long long) i); return HU_ERR_ARG; }
		bool plain = true;
		for(const char* p = s; *p; ++p) {
			const unsigned char c = (unsigned char) *p;
			if(c == '\'' || c < 0x20 || c == 0x7f) { hu_set_error("%s: the name of leaf %lld holds a quote or a byte that does not print", fn, (long long) i); return HU_ERR_ARG; }
			if(c == ' ' || strchr("()[]:;,", c)) plain = false;
		}
		label[(size_t) i] = plain ? std::string(s) : "'" + std::string(s) + "'";
	}
	std::vector<int8_t> seen((size_t) tot, 0);
	auto use = [&](int32_t v, int64_t below) { if(v < 0 || v >= below || seen[(size_t) v]) return false; seen[(size_t) v] = 1; return true; };
	for(int64_t t = 0; t < n - 3; ++t) if(!use(join[2 * t], n + t) || !use(join[2 * t + 1], n + t)) { hu_set_error("%s: join %lld names a node twice or one not yet made", fn, (long long) t); return HU_ERR_ARG; }
	for(int s = 0; s < 3; ++s) if(!use(last3[s], tot)) { hu_set_error("%s: the top node names a node twice or one that does not exist", fn); return HU_ERR_ARG; }
	std::string out;
	char num[64];
	/* depth first without recursion: a frame is (node, next child) */
	struct Frame { int32_t node; int32_t next; double blen; };
	std::vector<Frame> st;
	out += '(';
	for(int s = 0; s < 3; ++s) {
		if(s) out += ',';
		st.push_back({last3[s], 0, last_len3[s]});
		while(!st.empty()) {
			Frame& f = st.back();
			if(f.node < n) out += label[(size_t) f.node];
			else if(f.next < 2) {
				const int64_t t = f.node - n;
				out += f.next == 0 ? '(' : ',';
				const int32_t c = join[2 * t + f.next]; const double l = len[2 * t + f.next];
				++f.next;
				st.push_back({c, 0, l});
				continue;
			}
			else out += ')';
			snprintf(num, sizeof(num), ":%.17g", f.blen);
			out += num;
			st.pop_back();
		}
	}
	out += ");\n";
	const int64_t L = (int64_t) out.size();
	if(cap > 0) { const int64_t k = L < cap - 1 ? L : cap - 1; memcpy(buf, out.data(), (size_t) k); buf[k] = '\0'; }
	return L;
} catch(...) { return hu_catch_all("hu_nj_newick"); }
