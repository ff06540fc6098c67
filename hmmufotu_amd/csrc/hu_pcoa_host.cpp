// hu_pcoa without a device: the checks, the plan of a call, the block iteration (written once, against HuPcOps), the
// m x m work of both paths (Cholesky, the inverse of a triangle, cyclic Jacobi) and the host's operations in plain loops on one thread.
// No HIP headers: a plain C++ compiler builds this file (tests/san/pcoa_driver.cpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
#include "hu_pcoa.h"
#include "hu_permanova.h"

void hu_set_error(const char* fmt, ...);
int hu_catch_all(const char* fn) noexcept;

static thread_local double g_pcTiming[6] = {0, 0, 0, 0, 0, 0};
double* hu_pc_timing_slots() { return g_pcTiming; }

extern "C" int hu_pcoa_timing(double* seconds) {
	if(!seconds) return HU_ERR_ARG;
	memcpy(seconds, g_pcTiming, sizeof(g_pcTiming));
	return HU_OK;
}

extern "C" void hu_pcoa_default_opts(hu_pcoa_opts* o) {
	if(!o) return;
	o->k = 3; o->oversample = 8; o->tol = 1e-10; o->max_it = 1000; o->seed = 1; o->host = 0; o->reserved = 0; o->mem_budget = 0;
}

extern "C" int64_t hu_pcoa_slabs(int64_t n) { return n < 1 ? -1 : hu_pc_slabs(n); }

extern "C" int64_t hu_pcoa_need(int64_t n, int64_t k, int64_t oversample) {
	if(n < 3 || n > 0x7fffffffll || k < 1 || k > n - 1 || oversample < 0 || oversample > 0x7fffffffll) return -1;
	const int64_t m = std::min(k + oversample, n - 1);
	if(m > HU_PCOA_MAX_MP) return -1;
	return hu_pc_need_m(n, m);
}

int hu_pc_plan(const char* fn, int64_t n, const double* dist, const hu_pcoa_opts* opts, HuPcPlan& pl) {
	hu_pcoa_opts o;
	if(opts) o = *opts; else hu_pcoa_default_opts(&o);
	if(!dist) { hu_set_error("%s: null argument", fn); return HU_ERR_ARG; }
	if(n < 3) { hu_set_error("%s: %lld samples: principal coordinates need 3 at the least", fn, (long long) n); return HU_ERR_ARG; }
	if(n > 0x7fffffffll) { hu_set_error("%s: %lld samples: more than a grid holds", fn, (long long) n); return HU_ERR_ARG; }
	if(o.k < 1 || o.k > n - 1) { hu_set_error("%s: %lld axes of %lld samples: between 1 and %lld", fn, (long long) o.k, (long long) n, (long long)(n - 1)); return HU_ERR_ARG; }
	if(o.oversample < 0) { hu_set_error("%s: oversample %lld below 0", fn, (long long) o.oversample); return HU_ERR_ARG; }
	if(o.oversample > 0x7fffffffll) { hu_set_error("%s: oversample %lld above %lld", fn, (long long) o.oversample, 0x7fffffffll); return HU_ERR_ARG; }
	if(std::min(o.k + o.oversample, n - 1) > HU_PCOA_MAX_MP) {
		hu_set_error("%s: a block of %lld columns (%lld axes and %lld beyond them): %d at the most", fn, (long long) std::min(o.k + o.oversample, n - 1), (long long) o.k,
			(long long) o.oversample, HU_PCOA_MAX_MP); return HU_ERR_ARG; }
	if(!(o.tol > 0 && o.tol <= 1e-3)) { hu_set_error("%s: tol %g: above 0 and 1e-3 at the most", fn, o.tol); return HU_ERR_ARG; }
	if(o.max_it < 1) { hu_set_error("%s: max_it %lld below 1", fn, (long long) o.max_it); return HU_ERR_ARG; }
	const int rc = hu_pm_check_matrix(fn, n, dist);
	if(rc != HU_OK) return rc;
	pl.n = n; pl.k = o.k; pl.oversample = o.oversample; pl.tol = o.tol; pl.max_it = o.max_it; pl.seed = o.seed; pl.host = o.host != 0;
	pl.budget = o.mem_budget > 0 ? o.mem_budget : 0;
	return HU_OK;
}

/* ---- the m x m work ---- */

bool hu_pc_cholesky(int64_t m, int64_t ld, double* G, int64_t* fail) {
	for(int64_t j = 0; j < m; ++j) {
		double d = G[j * ld + j];
		for(int64_t p = 0; p < j; ++p) d = std::fma(-G[j * ld + p], G[j * ld + p], d);
		if(!(d > 0x1p-40)) { *fail = j; return false; }                    /* of a Gram matrix scaled to a unit diagonal */
		const double l = std::sqrt(d);
		G[j * ld + j] = l;
		for(int64_t i = j + 1; i < m; ++i) {
			double s = G[i * ld + j];
			for(int64_t p = 0; p < j; ++p) s = std::fma(-G[i * ld + p], G[j * ld + p], s);
			G[i * ld + j] = s / l;
		}
		for(int64_t i = 0; i < j; ++i) G[i * ld + j] = 0.0;
	}
	return true;
}

void hu_pc_jacobi(int64_t m, int64_t ld, double* H, double* theta, double* Q) {
	for(int64_t i = 0; i < m; ++i) for(int64_t j = 0; j < m; ++j) Q[i * ld + j] = i == j ? 1.0 : 0.0;
	for(int sweep = 0; sweep < 60; ++sweep) {
		double off = 0.0, diag = 0.0;
		for(int64_t i = 0; i < m; ++i) { diag += H[i * ld + i] * H[i * ld + i]; for(int64_t j = i + 1; j < m; ++j) off += H[i * ld + j] * H[i * ld + j]; }
		if(off == 0.0 || off <= 0x1p-106 * diag) break;
		for(int64_t p = 0; p < m; ++p) for(int64_t q = p + 1; q < m; ++q) {
			const double apq = H[p * ld + q];
			if(apq == 0.0) continue;
			const double tau = (H[q * ld + q] - H[p * ld + p]) / (2.0 * apq);
			const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau)), c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
			for(int64_t r = 0; r < m; ++r) {                                   /* H <- H R */
				const double x = H[r * ld + p], y = H[r * ld + q];
				H[r * ld + p] = c * x - s * y; H[r * ld + q] = s * x + c * y;
			}
			for(int64_t r = 0; r < m; ++r) {                                   /* H <- R' H */
				const double x = H[p * ld + r], y = H[q * ld + r];
				H[p * ld + r] = c * x - s * y; H[q * ld + r] = s * x + c * y;
			}
			H[p * ld + q] = H[q * ld + p] = 0.0;
			for(int64_t r = 0; r < m; ++r) {
				const double x = Q[r * ld + p], y = Q[r * ld + q];
				Q[r * ld + p] = c * x - s * y; Q[r * ld + q] = s * x + c * y;
			}
		}
	}
	for(int64_t i = 0; i < m; ++i) theta[i] = H[i * ld + i];
}

/* ---- the iteration ---- */

namespace {
struct Clock {
	std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	~Clock() { g_pcTiming[4] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

struct Run {
	const char* fn; HuPcOps& ops; const HuPcPlan& pl;
	int64_t m = 0, mp = 0;
	std::vector<double> G, M1, M2, Q, theta;

	void size(int64_t m_) { m = m_; mp = hu_pc_pad(m); G.assign((size_t)(mp * mp), 0.0); M1 = G; M2 = G; Q = G; theta.assign((size_t) mp, 0.0); }

	/* M1 = S L^-T of the Gram matrix in G, S its diagonal scaling: block * M1 has orthonormal columns.  false: column *fail depends on those before it */
	bool inverse_factor(int64_t* fail) {
		Clock c;
		std::vector<double> s((size_t) m);
		for(int64_t j = 0; j < m; ++j) { const double d = G[j * mp + j]; if(!(d > 0) || !std::isfinite(d)) { *fail = j; return false; } s[(size_t) j] = 1.0 / std::sqrt(d); }
		for(int64_t i = 0; i < m; ++i) {
			G[i * mp + i] = 1.0;
			for(int64_t j = i + 1; j < m; ++j) G[i * mp + j] = G[j * mp + i] = 0.5 * (G[i * mp + j] + G[j * mp + i]) * s[(size_t) i] * s[(size_t) j];
		}
		if(!hu_pc_cholesky(m, mp, G.data(), fail)) return false;
		/* X = L^-1 by forward substitution, column by column; M1 = S X' */
		std::fill(M1.begin(), M1.end(), 0.0);
		std::vector<double> x((size_t) m);
		for(int64_t col = 0; col < m; ++col) {
			for(int64_t i = 0; i < m; ++i) {
				double v = i == col ? 1.0 : 0.0;
				for(int64_t p = col; p < i; ++p) v = std::fma(-G[i * mp + p], x[(size_t) p], v);
				x[(size_t) i] = i < col ? 0.0 : v / G[i * mp + i];
			}
			for(int64_t i = 0; i < m; ++i) M1[col * mp + i] = s[(size_t) col] * x[(size_t) i];      /* (S L^-T)[col][i] = s_col (L^-1)[i][col] */
		}
		return true;
	}

	/* block `dst` = block `src` with orthonormal columns (CholQR2), `tmp` is lost; HU_OK, an error, or 1 with *fail */
	int orth(int src, int tmp, int dst, int64_t* fail) {
		int rc;
		if((rc = ops.gram(src, src, G.data())) != HU_OK) return rc;
		if(!inverse_factor(fail)) return 1;
		if((rc = ops.apply(src, M1.data(), -1, nullptr, tmp)) != HU_OK) return rc;
		if((rc = ops.gram(tmp, tmp, G.data())) != HU_OK) return rc;
		if(!inverse_factor(fail)) return 1;
		return ops.apply(tmp, M1.data(), -1, nullptr, dst);
	}

	/* res [m] = the column norms of block x, by its Gram matrix's diagonal */
	int norms(int x, double* res) {
		const int rc = ops.gram(x, x, G.data());
		if(rc != HU_OK) return rc;
		for(int64_t a = 0; a < m; ++a) res[a] = std::sqrt(std::max(0.0, G[a * mp + a]));
		return HU_OK;
	}
};
}

int hu_pc_run(const char* fn, HuPcOps& ops, const HuPcPlan& pl, double trace, hu_pcoa_result* out, double* coords, double* eigval, double* resid) {
	const int64_t n = pl.n, k = pl.k, top = std::min<int64_t>(n - 1, HU_PCOA_MAX_MP);
	Run r{fn, ops, pl};
	int64_t over = pl.oversample, iterations = 0;
	int rc;
	for(;;) {	/* one block width */
		r.size(std::min(k + over, top));
		const int64_t m = r.m, mp = r.mp;
		{
			std::vector<double> start((size_t)(n * mp), 0.0);
			for(int64_t i = 0; i < n; ++i) for(int64_t c = 0; c < m; ++c) start[(size_t)(i * mp + c)] = hu_pc_start(pl.seed, (uint64_t) i, (uint64_t) c);
			if((rc = ops.setup(m, start.data(), 1)) != HU_OK) return rc;
		}
		int64_t fail = 0;
		if((rc = ops.centre(1, 2)) != HU_OK) return rc;
		rc = r.orth(2, 3, 0, &fail);
		if(rc == 1) { hu_set_error("%s: column %lld of the start block of seed %llu depends on those before it: try another seed", fn, (long long) fail, (unsigned long long) pl.seed); return HU_ERR_NUMERIC; }
		if(rc != HU_OK) return rc;
		int V = 0, W = 1, T = 2, T2 = 3;                                     /* the four blocks by role */
		std::vector<int64_t> pos; std::vector<double> res((size_t) mp, 0.0);
		std::vector<char> keep((size_t) m);
		std::vector<double> prev;                                            /* the sorted Ritz values of the iteration before, at the widest block */
		bool widen = false;
		for(int64_t since = 1; !widen; ++since) {
			if(iterations >= pl.max_it) {
				int64_t worst = -1; double wr = -1;
				for(int64_t a = 0; a < (int64_t) pos.size() && a < k; ++a) if(res[(size_t) pos[(size_t) a]] > wr) { wr = res[(size_t) pos[(size_t) a]]; worst = a; }
				if(worst < 0 || (int64_t) pos.size() < k) hu_set_error("%s: no convergence in %lld iterations: the block of %lld columns holds %zu positive axes of the %lld asked", fn, (long long) pl.max_it, (long long) m, pos.size(), (long long) k);
				else hu_set_error("%s: no convergence in %lld iterations: axis %lld has the residual %.3g, above tol * lambda_1 = %.3g", fn, (long long) pl.max_it,
					(long long)(worst + 1), wr, pl.tol * r.theta[(size_t) pos[0]]);
				return HU_ERR_NUMERIC;
			}
			++iterations;
			if((rc = ops.bv(V, W)) != HU_OK) return rc;
			if((rc = ops.gram(V, W, r.G.data())) != HU_OK) return rc;
			double tmax = 0;
			{	/* Rayleigh-Ritz: H = V'BV = Q Theta Q' */
				Clock c;
				for(int64_t i = 0; i < m; ++i) for(int64_t j = i; j < m; ++j) r.G[i * mp + j] = r.G[j * mp + i] = 0.5 * (r.G[i * mp + j] + r.G[j * mp + i]);
				hu_pc_jacobi(m, mp, r.G.data(), r.theta.data(), r.Q.data());
				pos.clear();
				for(int64_t a = 0; a < m; ++a) tmax = std::max(tmax, std::fabs(r.theta[(size_t) a]));
			/* positive: above the rounding of B's own entries, n 2^-52 of the largest magnitude; below it a value is not told from 0 */
			for(int64_t a = 0; a < m; ++a) if(r.theta[(size_t) a] > (double) n * 0x1p-52 * tmax) pos.push_back(a);
				std::stable_sort(pos.begin(), pos.end(), [&](int64_t a, int64_t b) { return r.theta[(size_t) a] > r.theta[(size_t) b]; });
			}
			const int64_t P = (int64_t) pos.size();
			out->positive_in_block = P; out->m_final = m; out->iterations = iterations;
			if(P < k) {
				if(m == n - 1) { hu_set_error("%s: only %lld positive axes; %lld asked", fn, (long long) P, (long long) k); return HU_ERR_NUMERIC; }      /* exact */
				if(m < top) {
					if(since >= HU_PCOA_GROW_AFTER) { over = over ? 2 * over : 8; widen = true; continue; }
				} else {
					/* the widest block: not a count of B's positive axes, so it is refused only once its Ritz values have settled, none of them
					 * moving by more than tol * max |theta| in an iteration; until then the power step goes on, to max_it at the latest */
					std::vector<double> now(r.theta.begin(), r.theta.begin() + m);
					std::sort(now.begin(), now.end());
					double moved = INFINITY;
					if(prev.size() == now.size()) { moved = 0; for(int64_t a = 0; a < m; ++a) moved = std::max(moved, std::fabs(now[(size_t) a] - prev[(size_t) a])); }
					prev.swap(now);
					if(since >= HU_PCOA_GROW_AFTER && moved <= pl.tol * tmax) {
						hu_set_error("%s: %lld positive axes found in a settled block of %lld columns, the widest; %lld asked", fn, (long long) P, (long long) m, (long long) k);
						return HU_ERR_NUMERIC;
					}
				}
			} else {
				/* the residuals of the Ritz pairs: R = W Q - V Q Theta */
				{
					Clock c;
					std::fill(r.M2.begin(), r.M2.end(), 0.0);
					for(int64_t i = 0; i < m; ++i) for(int64_t a = 0; a < m; ++a) r.M2[i * mp + a] = -r.Q[i * mp + a] * r.theta[(size_t) a];
				}
				if((rc = ops.apply(W, r.Q.data(), V, r.M2.data(), T)) != HU_OK) return rc;
				if((rc = r.norms(T, res.data())) != HU_OK) return rc;
				const double bar = pl.tol * r.theta[(size_t) pos[0]];
				bool done = true;
				for(int64_t a = 0; a < k; ++a) done = done && res[(size_t) pos[(size_t) a]] <= bar;
				if(done) {
					/* the certificate: one more product with the final vectors U = V Q */
					if((rc = ops.apply(V, r.Q.data(), -1, nullptr, T)) != HU_OK) return rc;
					if((rc = ops.bv(T, T2)) != HU_OK) return rc;
					if((rc = ops.gram(T, T2, r.G.data())) != HU_OK) return rc;
					std::vector<double> lam((size_t) m);
					{
						Clock c;
						std::fill(r.M1.begin(), r.M1.end(), 0.0); std::fill(r.M2.begin(), r.M2.end(), 0.0);
						for(int64_t a = 0; a < m; ++a) { lam[(size_t) a] = r.G[a * mp + a]; r.M1[a * mp + a] = 1.0; r.M2[a * mp + a] = -lam[(size_t) a]; }
					}
					if((rc = ops.apply(T2, r.M1.data(), T, r.M2.data(), W)) != HU_OK) return rc;
					if((rc = r.norms(W, res.data())) != HU_OK) return rc;
					std::vector<int64_t> fin(pos.begin(), pos.begin() + k);
					std::stable_sort(fin.begin(), fin.end(), [&](int64_t a, int64_t b) { return lam[(size_t) a] > lam[(size_t) b]; });
					const double bar2 = pl.tol * lam[(size_t) fin[0]];
					bool ok = true;
					for(int64_t a = 0; a < k; ++a) ok = ok && lam[(size_t) fin[(size_t) a]] > 0 && res[(size_t) fin[(size_t) a]] <= bar2;
					if(ok) {
						std::vector<double> U((size_t)(n * mp));
						if((rc = ops.fetch(T, U.data())) != HU_OK) return rc;
						Clock c;
						for(int64_t a = 0; a < k; ++a) {
							const int64_t col = fin[(size_t) a];
							double big = 0; int64_t at = 0;
							for(int64_t i = 0; i < n; ++i) if(std::fabs(U[(size_t)(i * mp + col)]) > big) { big = std::fabs(U[(size_t)(i * mp + col)]); at = i; }
							const double sc = (U[(size_t)(at * mp + col)] < 0 ? -1.0 : 1.0) * std::sqrt(lam[(size_t) col]);
							for(int64_t i = 0; i < n; ++i) coords[i * k + a] = U[(size_t)(i * mp + col)] * sc;
							eigval[a] = lam[(size_t) col]; resid[a] = res[(size_t) col];
						}
						out->n = n; out->k = k; out->trace = trace;
						return HU_OK;
					}
					std::swap(V, T);                                                  /* rounding alone can bring this about: go on from U */
					continue;
				}
			}
			/* the power step: column a of Z is B u_a = (W Q)_a, or u_a itself where theta_a is too small to carry a direction */
			for(int64_t a = 0; a < m; ++a) keep[(size_t) a] = !(std::fabs(r.theta[(size_t) a]) > HU_PCOA_KEEP * tmax);
			for(;;) {
				{
					Clock c;
					std::fill(r.M1.begin(), r.M1.end(), 0.0); std::fill(r.M2.begin(), r.M2.end(), 0.0);
					for(int64_t i = 0; i < m; ++i) for(int64_t a = 0; a < m; ++a) (keep[(size_t) a] ? r.M2 : r.M1)[i * mp + a] = r.Q[i * mp + a];
				}
				if((rc = ops.apply(W, r.M1.data(), V, r.M2.data(), T)) != HU_OK) return rc;
				rc = r.orth(T, T2, W, &fail);
				if(rc == HU_OK) break;
				if(rc != 1) return rc;
				if(keep[(size_t) fail]) { hu_set_error("%s: the block lost its rank at column %lld", fn, (long long) fail); return HU_ERR_NUMERIC; }
				keep[(size_t) fail] = 1;                                              /* Z'Z >= the kept columns' identity: ends with all kept at the latest */
			}
			std::swap(V, W);
		}
	}
}

/* ---- the host's operations ---- */

namespace {
struct HostOps : HuPcOps {
	int64_t n, m = 0, mp = 0;
	std::vector<double> D2, blk[4], tmp;
	HostOps(int64_t n_, const double* dist) : n(n_), D2((size_t)(n_ * n_)) { for(size_t i = 0; i < D2.size(); ++i) D2[i] = dist[i] * dist[i]; }
	int setup(int64_t m_, const double* start, int dst) override {
		m = m_; mp = hu_pc_pad(m);
		for(auto& b : blk) b.assign((size_t)(n * mp), 0.0);
		tmp.assign((size_t)(n * mp), 0.0);
		std::copy(start, start + n * mp, blk[dst].begin());
		return HU_OK;
	}
	/* dst = scale * (src - the column means of src) */
	void centred(const std::vector<double>& src, double scale, std::vector<double>& dst) {
		for(int64_t c = 0; c < m; ++c) {
			double s = 0.0;
			for(int64_t i = 0; i < n; ++i) s += src[(size_t)(i * mp + c)];
			const double mean = s / (double) n;
			for(int64_t i = 0; i < n; ++i) dst[(size_t)(i * mp + c)] = scale * (src[(size_t)(i * mp + c)] - mean);
		}
	}
	int bv(int src, int dst) override {
		const double* V = blk[src].data();
		std::fill(tmp.begin(), tmp.end(), 0.0);
		for(int64_t i = 0; i < n; ++i) {
			double* w = tmp.data() + i * mp;
			const double* row = D2.data() + i * n;
			for(int64_t j = 0; j < n; ++j) { const double d = row[j]; const double* v = V + j * mp; for(int64_t c = 0; c < m; ++c) w[c] = std::fma(d, v[c], w[c]); }
		}
		centred(tmp, -0.5, blk[dst]);
		return HU_OK;
	}
	int centre(int src, int dst) override { centred(blk[src], 1.0, blk[dst]); return HU_OK; }
	int gram(int x, int y, double* G) override {
		std::fill(G, G + mp * mp, 0.0);
		for(int64_t i = 0; i < n; ++i) {
			const double *a = blk[x].data() + i * mp, *b = blk[y].data() + i * mp;
			for(int64_t p = 0; p < m; ++p) for(int64_t q = 0; q < m; ++q) G[p * mp + q] = std::fma(a[p], b[q], G[p * mp + q]);
		}
		return HU_OK;
	}
	int apply(int x, const double* M1, int y, const double* M2, int dst) override {
		for(int64_t i = 0; i < n; ++i) for(int64_t c = 0; c < m; ++c) {
			double s = 0.0;
			for(int64_t a = 0; a < m; ++a) s = std::fma(blk[x][(size_t)(i * mp + a)], M1[a * mp + c], s);
			if(y >= 0) for(int64_t a = 0; a < m; ++a) s = std::fma(blk[y][(size_t)(i * mp + a)], M2[a * mp + c], s);
			blk[dst][(size_t)(i * mp + c)] = s;
		}
		return HU_OK;
	}
	int fetch(int src, double* out) override { std::copy(blk[src].begin(), blk[src].end(), out); return HU_OK; }
};
}

HuPcOps* hu_pc_host_ops(int64_t n, const double* dist) { return new HostOps(n, dist); }
