// What the host half (hu_nj_host.cpp, a plain C++ compiler) and the device half (hu_tree.cpp, hu_kern_dist.h, hu_kern_nj.h) of
// hmmufotu-amd-tree share: the distance formulas, the rules of one join and the constants that fix the summation order.
// Every function here is compiled for both sides from this one text, and both translation units are built with -ffp-contract=off, so
// that no multiply and add is fused on one side only; the one fused operation, in hu_nj_q, is written as fma.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/hmmufotu_amd.h"

#if defined(__HIPCC__)
#define HU_NJ_HD __host__ __device__ inline
#else
#define HU_NJ_HD inline
#endif

#define HU_DIST_TILE 64          /* rows per side of a tile of the pair matrix */
#define HU_DIST_CHUNK 8          /* 64-bit plane words staged at a time; the words of a row are padded to a multiple of it */
#define HU_NJ_SUM_BLOCK 256      /* R: serial sums of blocks of this many slots, then the block sums in ascending order */
#define HU_NJ_MAX_N 262144       /* 1024 blocks of HU_NJ_SUM_BLOCK: what the row sum's LDS holds */
#define HU_NJ_PICK_WG 1024       /* workgroups of the argmin's first stage, at the most */

/* The closed-form distances of the reference's DNASubModel::subDist(D, N), from the four integers every one of them needs: N compared
 * columns, P_R A<->G and P_Y C<->T differences, Q transversions.
 *   HU_DIST_PDIST  (P_R + P_Y + Q) / N
 *   HU_DIST_JC69   src/JC69.h:103-108     HU_DIST_K80   src/K80.h:120-126     HU_DIST_F81  src/F81.h:120-126
 *   HU_DIST_HKY85  src/HKY85.h:155-168    HU_DIST_TN93  src/TN93.h:156-172
 * Each expression is the reference's, term for term.  Two remarks: TN93's second coefficient is 2 g c / y there where
 * Tamura and Nei have 2 t c / y, and it is kept as the reference has it; in HKY85 the reference's locals A and C hide the base
 * enumerators of the same names in the two lines that count, and the counts meant by their comments (transitions, transversions) are
 * used here.  N == 0 gives 0.  *sat is set when a logarithm's argument is <= 0 (or not a number); the value is then not used. */
HU_NJ_HD double hu_sub_dist(int type, const double* pi, int32_t N, int32_t PR, int32_t PY, int32_t Q, int* sat) {
	*sat = 0;
	if(N == 0) return 0.0;
	const double n = (double) N;
	double d = 0.0;
	if(type == HU_DIST_PDIST) d = (double)(PR + PY + Q) / n;
	else if(type == HU_DIST_JC69) {
		const double p = (double)(PR + PY + Q) / n;
		const double x = 1.0 - 4.0 / 3.0 * p;
		if(!(x > 0)) { *sat = 1; return 0.0; }
		d = - 3.0 / 4.0 * log(x);
	}
	else if(type == HU_DIST_K80) {
		const double p = (double)(PR + PY) / n, q = (double) Q / n;
		const double x = 1 - 2 * p - q, y = 1 - 2 * q;
		if(!(x > 0) || !(y > 0)) { *sat = 1; return 0.0; }
		d = - 1.0 / 2 * log(x) - 1.0 / 4 * log(y);
	}
	else if(type == HU_DIST_F81) {
		const double p = (double)(PR + PY + Q) / n;
		const double E = 1 - (pi[0] * pi[0] + pi[1] * pi[1] + pi[2] * pi[2] + pi[3] * pi[3]);
		const double x = 1 - p / E;
		if(!(x > 0)) { *sat = 1; return 0.0; }
		d = - E * log(x);
	}
	else if(type == HU_DIST_HKY85) {
		const double a = pi[0], c = pi[1], g = pi[2], t = pi[3];
		const double A = a * g / (a + g) + c * t / (c + t);
		const double B = a * g + c * t;
		const double C = (a + g) * (c + t);
		const double p = (double)(PR + PY) / n, q = (double) Q / n;
		const double x = 1 - p / (2 * A) - (A - B) * q / (2 * A * C);
		if(!(x > 0)) { *sat = 1; return 0.0; }
		d = - 2 * A * log(x);
	}
	else {
		const double a = pi[0], c = pi[1], g = pi[2], t = pi[3];
		const double r = a + g, y = c + t;
		const double pr = (double) PR / n, py = (double) PY / n, q = (double) Q / n;
		const double x1 = 1 - r / (2 * a * g) * pr - 1 / (2 * r) * q;
		const double x2 = 1 - y / (2 * t * c) * py - 1 / (2 * y) * q;
		const double x3 = 1 - 1 / (2 * r * y) * q;
		if(!(x1 > 0) || !(x2 > 0) || !(x3 > 0)) { *sat = 1; return 0.0; }
		d = - 2 * a * g / r * log(x1)
			- 2 * g * c / y * log(x2)
			- 2 * (r * y - a * g * y / r - t * c * r / y) * log(x3);
	}
	if(!(d == d) || d - d != 0.0) { *sat = 1; return 0.0; }     /* a pi with a zero: no distance */
	return d + 0.0;                                              /* -0 of log(1) becomes +0 */
}

/* ---- one join of neighbour joining, the rules of DESIGN.md §21 ---- */
HU_NJ_HD double hu_nj_q(int64_t r, double dij, double Ri, double Rj) { return fma((double)(r - 2), dij, -(Ri + Rj)); }
/* (Q, i, j) in lexicographic order: the smaller Q, then the smaller i, then the smaller j */
HU_NJ_HD bool hu_nj_less(double Qa, int32_t ia, int32_t ja, double Qb, int32_t ib, int32_t jb) {
	if(Qa < Qb) return true;
	if(Qb < Qa) return false;
	if(ia != ib) return ia < ib;
	return ja < jb;
}
HU_NJ_HD void hu_nj_lengths(int64_t r, double dij, double Ri, double Rj, double* li, double* lj) {
	double a = dij / 2 + (Ri - Rj) / (2.0 * (double)(r - 2));
	double b = dij - a;
	if(a < 0) { a = 0.0; b = dij; }
	else if(b < 0) { b = 0.0; a = dij; }
	*li = a; *lj = b;
}
HU_NJ_HD double hu_nj_duk(double dik, double djk, double dij) { return (dik + djk - dij) / 2; }
HU_NJ_HD double hu_nj_rk(double Rk, double dik, double djk, double duk) { return (Rk - dik - djk) + duk; }
HU_NJ_HD void hu_nj_last3(double dab, double dac, double dbc, double* l) {
	l[0] = (dab + dac - dbc) / 2; l[1] = (dab + dbc - dac) / 2; l[2] = (dac + dbc - dab) / 2;
}

/* the host half, hu_nj_host.cpp */
/* the arguments of a distance call, checked: HU_OK or HU_ERR_ARG with the message set */
int hu_dist_check(const char* fn, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat);
void hu_dist_host_counts(int64_t n, int64_t cs_len, const int8_t* rows, int32_t* counts /* [n][n][4] */);
/* D [n][n]; sat <= 0: twice the largest finite distance.  HU_ERR_ARG when no off-diagonal distance is finite */
int hu_dist_host(const char* fn, int64_t n, int64_t cs_len, const int8_t* rows, int dist_type, const double* pi, double sat, double* D, int64_t* n_sat);
int hu_nj_check(const char* fn, int64_t n, const double* D);
/* D [n][n] is used up */
void hu_nj_host_run(int64_t n, double* D, int32_t* join, double* len, int32_t* last3, double* last_len3);
