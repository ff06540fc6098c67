"""hmmufotu-amd-permanova --design: sequential PERMANOVA of covariates, factors and interactions, with strata;
hu_design_build, hu_permanova_perms and hu_permanova_design on the host and on the device, and the program.

The yardstick shares no code with the library.  Philox4x32-10 and the stratified shuffle are restated in plain Python integers.  The
raw design (an intercept, the values of a covariate, the indicators of levels 2 .. L in order of first appearance, the products of an
interaction) is built from the variables themselves; the projectors H_1, H_{1..2}, ... come from the normal equations; B = -1/2 J D2 J
comes from the exact squares of the doubles; SS_t = tr((H_{1..t} - H_{1..t-1}) B) for the observed order and for every permutation.
All of it is integer arithmetic on fixed-point numbers: 200 binary places hold every double of the fixtures exactly, X'X and the traces
are exact, and only the inverse of X'X is rounded, by Gauss-Jordan elimination with 600 binary places (180 digits, where 50 would do: this
suite keeps mpmath to the generator of its golden files, so the yardstick brings its own arithmetic).

The bar (derived there): |SS_t - yardstick| <= df_t n^3 2^-50 max D2.  Of the basis: max |Q'Q - I| <= q 2^-50 and
max |1'Q| <= n 2^-52, both evaluated exactly.

The condition on every fixture, asserted from the yardstick alone before p is compared: the F_t of a permutation lies within 2^-40
relatively of the observed one (a tie, which must count) or further than 2^-20 from it.  Under it count_ge and p are compared exactly."""
import functools
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
M32 = 0xffffffff
FP = 200                                                                    # binary places of the fixed-point integers
WP = 600                                                                    # binary places of the inverse of X'X


def _bin(name="hmmufotu-amd-permanova"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ---- the restatement ----

def philox(counter, key):
    c0, c1, c2, c3 = counter; k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0; p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32; k1 = (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def perm_index(n, strata, seed, p):
    """the index array of permutation p: within every stratum, members ascending, step t moves sample m_t"""
    idx = list(range(n))
    blocks = {}
    for i in range(n):
        blocks.setdefault(0 if strata is None else strata[i], []).append(i)
    for key in sorted(blocks):
        m = blocks[key]
        for t in range(len(m) - 1, 0, -1):
            w = philox((m[t] & M32, m[t] >> 32, p & M32, p >> 32), (seed & M32, (seed >> 32) & M32))
            j = (((w[1] << 32) | w[0]) * (t + 1)) >> 64
            idx[m[t]], idx[m[j]] = idx[m[j]], idx[m[t]]
    return idx


def fixed(x):
    """the double x as an integer of FP binary places, exactly"""
    f = Fraction(float(x)) * (1 << FP)
    assert f.denominator == 1, "a double of the fixture has more than %d binary places" % FP
    return int(f)


def inverse_fixed(A, places):
    """the inverse of the symmetric positive definite A (integers of `places` binary places) as integers of WP places: Gauss-Jordan with
    partial pivoting on [A | I], every quotient and product rounded down at WP places"""
    k = len(A)
    M = [[int(A[r][c]) << (WP - places) if WP >= places else int(A[r][c]) >> (places - WP) for c in range(k)] + [(1 << WP) if c == r else 0 for c in range(k)] for r in range(k)]
    for col in range(k):
        piv = max(range(col, k), key=lambda r: abs(M[r][col]))
        assert M[piv][col] != 0, "the normal equations are singular"
        M[col], M[piv] = M[piv], M[col]
        top = M[col]
        for r in range(k):
            if r != col and M[r][col]:
                f = (M[r][col] << WP) // top[col]
                M[r] = [x - ((f * y) >> WP) for x, y in zip(M[r], top)]
    return [[(M[r][k + c] << WP) // M[r][r] for c in range(k)] for r in range(k)]


def first_levels(values):
    first = {}
    return [first.setdefault(v, len(first)) for v in values]


def raw_columns(variables, factors, name):
    """the raw columns of a variable: its values, or the indicators of its levels 2 .. L in order of first appearance"""
    vals = variables[name]
    if name in factors:
        lab = first_levels(vals)
        return [[1.0 if l == k else 0.0 for l in lab] for k in range(1, max(lab) + 1)]
    return [[float(v) for v in vals]]


class Yard:
    """the exact sums of a matrix and a design: G [T] the differences of successive projectors, Bn = -2 n^2 B, all fixed-point integers"""

    def __init__(self, dist, variables, factors, terms):
        d = np.asarray(dist, np.float64)
        self.n = n = d.shape[0]
        D2 = np.array([[fixed(x) ** 2 for x in row] for row in d], dtype=object)          # 2 FP places
        r = D2.sum(axis=1); tot = int(r.sum())
        self.Bn = n * n * D2 - n * r[:, None] - n * r[None, :] + tot                          # (nI - 11') D2 (nI - 11') = -2 n^2 B
        self.max_d2 = float(np.max(d * d))
        self.ss_total = Fraction(int(sum(D2[i, j] for i in range(n) for j in range(i + 1, n))), n << (2 * FP))
        cols = [[1.0] * n]
        self.df = []
        H = [np.array([[(1 << FP) // n] * n] * n, dtype=object)]                              # the projector on the intercept
        self.G = []
        for term in terms:
            parts = term.split(":")
            new = raw_columns(variables, factors, parts[0])
            if len(parts) == 2:
                new = [[a * b for a, b in zip(ca, cb)] for ca in new for cb in raw_columns(variables, factors, parts[1])]
            cols += new
            self.df.append(len(new))
            X = np.array([[fixed(c[i]) for c in cols] for i in range(n)], dtype=object)        # [n][k], FP places
            A = X.T.dot(X)                                                                     # exact, 2 FP places
            Af = np.array(inverse_fixed(A.tolist(), 2 * FP), dtype=object)                      # the normal equations, WP places
            Ht = X.dot(Af).dot(X.T)                                                            # 2 FP + WP places
            Ht = np.array([[int(v) >> (FP + WP) for v in row] for row in Ht], dtype=object)
            self.G.append(Ht - H[-1])
            H.append(Ht)
        # a projector's trace is its rank: the check that the normal equations were solved
        for t, g in enumerate(self.G):
            assert abs(Fraction(int(np.trace(g)), 1 << FP) - self.df[t]) < Fraction(1, 10 ** 30), "term %d: the projector's trace is not its rank" % t

    def ss(self, idx):
        """[T] SS_t with the design row of sample i row idx[i]"""
        ix = np.ix_(idx, idx)
        scale = -2 * self.n * self.n << (3 * FP)
        return [Fraction(int((g[ix] * self.Bn).sum()), scale) for g in self.G]


class Case:
    def __init__(self, dist, variables, factors, terms, perms, seed, strata=None):
        self.dist = np.ascontiguousarray(dist, np.float64); self.variables = variables; self.factors = tuple(factors); self.terms = list(terms)
        self.perms = perms; self.seed = seed; self.strata = None if strata is None else first_levels(strata)
        self.n = n = self.dist.shape[0]
        self.yard = y = Yard(self.dist, variables, self.factors, self.terms)
        self.df = y.df; self.q = sum(y.df); self.df_res = n - 1 - self.q
        self.bar = [df * n ** 3 * 2.0 ** -50 * y.max_d2 for df in y.df]
        self.index = [perm_index(n, self.strata, seed, p) for p in range(perms)]
        self.obs = y.ss(list(range(n)))
        memo = {}
        self.ss = []
        for idx in self.index:
            key = tuple(idx)
            if key not in memo:
                memo[key] = y.ss(idx)
            self.ss.append(memo[key])
        self.F_obs = self.F(self.obs)
        self.count_ge = [0] * len(terms)
        for p, row in enumerate(self.ss):
            for t, f in enumerate(self.F(row)):
                gap = abs(f - self.F_obs[t])
                tie = gap <= Fraction(1, 2 ** 40) * abs(self.F_obs[t])
                # the condition on the fixture
                assert tie or gap > Fraction(1, 2 ** 20) * abs(self.F_obs[t]), "permutation %d, term %d: F lies between a tie and 2^-20 of the observed one" % (p, t)
                self.count_ge[t] += 1 if tie or f > self.F_obs[t] else 0

    def F(self, row):
        res = self.yard.ss_total - sum(row)
        return [(row[t] / self.df[t]) / (res / self.df_res) for t in range(len(row))]

    def build(self):
        return E.design_build(self.variables, self.terms, factors=self.factors)

    def check(self, out, D, scale=1.0):
        """a result of the library against the yardstick: every SS_t(p) within the bar, the observed ones, the counts and p"""
        assert list(D["df"]) == self.df
        for t, term in enumerate(out["terms"]):
            assert abs(Fraction(term["ss"]) - self.obs[t]) <= scale * Fraction(self.bar[t]), (t, term["ss"], float(self.obs[t]))
            assert term["df"] == self.df[t] and term["df_res"] == self.df_res and term["count_nan"] == 0
        err = max(float(abs(Fraction(float(out["ss_perm"][p][t])) - self.ss[p][t])) / self.bar[t] for p in range(self.perms) for t in range(len(self.terms)))
        assert err <= scale, "SS_t(p) is %g bars from the yardstick" % err
        assert abs(Fraction(out["ss_total"]) - self.yard.ss_total) <= self.n ** 2 * Fraction(1, 2 ** 52) * self.yard.ss_total
        for t, term in enumerate(out["terms"]):
            assert term["count_ge"] == self.count_ge[t], (t, term["count_ge"], self.count_ge[t])
            assert term["p"] == (1 + self.count_ge[t]) / (self.perms + 1)
        return err


def points(n, seed, dims=3, shift=None):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dims))
    if shift is not None:
        x[:, 0] += np.asarray(shift, float)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = float(np.sqrt(((x[i] - x[j]) ** 2).sum()))
    return d


def factor(n, levels, seed):
    """labels with every level used, twice where n allows (an interaction with a covariate needs that), as strings"""
    rng = np.random.default_rng(seed + 500)
    g = (list(range(levels)) * 2)[:min(n, 2 * levels)]
    g += rng.integers(0, levels, n - len(g)).tolist()
    return ["L%d" % int(x) for x in rng.permutation(g)]


def covariate(n, seed):
    return [float(x) for x in np.random.default_rng(seed + 900).normal(size=n)]


DESIGNS = {
    "factor": (("g",), ("g",)),
    "covariate": (("c",), ()),
    "factor+covariate": (("g", "c"), ("g",)),
    "factor*covariate": (("g", "c", "g:c"), ("g",)),
}


@functools.lru_cache(maxsize=None)
def cpu_case(n, design, perms=40, seed=11):
    terms, factors = DESIGNS[design]
    return Case(points(n, 100 + n), dict(g=factor(n, 2 if n < 7 else 3, n), c=covariate(n, n)), factors, terms, perms, seed)


def run_case(case, **kw):
    D = case.build()
    out = E.permanova_design(case.dist, D["Q"], D["term_start"], strata=case.strata, perms=case.perms, seed=case.seed, **kw)
    return D, out


# ---- CPU: the library's host path ----

def test_philox_and_perms_match_the_restatement():
    for n, strata in ((7, None), (9, [0, 1, 0, 2, 1, 0, 2, 2, 0]), (65, [i % 5 for i in range(65)])):
        got = E.permanova_perms(n, strata=strata, seed=77, first=0, count=6)
        for p in range(6):
            assert got[p].tolist() == perm_index(n, strata, 77, p)


def test_six_samples_by_hand():
    """points (x, y) with x = -5 .. 5 in steps of 2 and y = (1, -1, 0, 0, -1, 1): x and y are centred and orthogonal, so with the covariate x
    SS_x = x'x = 70, SS_res = y'y = 4, SS_T = 74, F = 70 / (4 / 4), R2 = 70 / 74"""
    x = np.array([-5.0, -3, -1, 1, 3, 5]); y = np.array([1.0, -1, 0, 0, -1, 1])
    d = np.sqrt((x[:, None] - x[None]) ** 2 + (y[:, None] - y[None]) ** 2)
    D = E.design_build(dict(x=x.tolist()), ["x"])
    assert D["q"] == 1 and list(D["df"]) == [1] and list(D["term_start"]) == [0, 1]
    assert np.allclose(D["Q"][:, 0], x / np.sqrt(70.0), rtol=0, atol=1e-15)
    out = E.permanova_design(d, D["Q"], D["term_start"], perms=99, seed=1, host=True)
    bar = 6 ** 3 * 2.0 ** -50 * 104
    t = out["terms"][0]
    assert abs(t["ss"] - 70) <= bar and abs(t["ss_res"] - 4) <= 2 * bar and abs(t["ss_total"] - 74) <= bar
    assert abs(t["F"] - 70) <= 1e-9 and abs(t["R2"] - 70 / 74) <= 1e-12 and t["df"] == 1 and t["df_res"] == 4


@pytest.mark.parametrize("design", sorted(DESIGNS))
@pytest.mark.parametrize("n", [4, 7, 65])
def test_host_against_the_yardstick(n, design):
    if n == 4 and design == "factor*covariate":
        with pytest.raises(E.EngineError, match="residual degrees of freedom"):
            terms, factors = DESIGNS[design]
            E.design_build(dict(g=factor(4, 2, 4), c=covariate(4, 4)), terms, factors=factors)
        return
    case = cpu_case(n, design)
    D, out = run_case(case, host=True)
    case.check(out, D)


@pytest.mark.parametrize("n", [4, 7, 65])
def test_basis_is_orthonormal_and_centred(n):
    for design in sorted(DESIGNS):
        if n == 4 and design == "factor*covariate":
            continue
        terms, factors = DESIGNS[design]
        D = E.design_build(dict(g=factor(n, 2 if n < 7 else 3, n), c=covariate(n, n)), terms, factors=factors)
        Q = [[Fraction(float(v)) for v in row] for row in D["Q"]]
        q = D["q"]
        for a in range(q):
            assert abs(sum(Q[i][a] for i in range(n))) <= Fraction(n, 2 ** 52)
            for b in range(a + 1):
                dot = sum(Q[i][a] * Q[i][b] for i in range(n))
                assert abs(dot - (1 if a == b else 0)) <= Fraction(q, 2 ** 50), (a, b, float(dot))


@pytest.mark.parametrize("n", [4, 7, 65])
def test_collinear_and_duplicated_terms_are_refused_by_name(n):
    g = factor(n, 2 if n < 7 else 3, n)
    twin = ["x" + v for v in g]                                                  # the same partition under other names
    with pytest.raises(E.EngineError, match="term 'h' adds nothing to the terms before it"):
        E.design_build(dict(g=g, h=twin), ["g", "h"], factors=("g", "h"))
    c = covariate(n, n)
    with pytest.raises(E.EngineError, match="term 'c2' adds nothing to the terms before it"):
        E.design_build(dict(c=c, c2=[2 * v + 1 for v in c]), ["c", "c2"])


def test_one_factor_against_permanova():
    n, perms, seed = 65, 60, 9
    d = points(n, 31, shift=[3.0 * (i % 3) for i in range(n)])
    g = first_levels(factor(n, 3, 2))
    D = E.design_build(dict(g=g), ["g"], factors=("g",))
    out = E.permanova_design(d, D["Q"], D["term_start"], perms=perms, seed=seed, host=True)
    ref = E.permanova(d, g, perms=perms, seed=seed, host=True)
    idx = E.permanova_perms(n, seed=seed, count=perms)
    assert (np.asarray(g)[idx] == E.permanova_labels(g, seed=seed, count=perms)).all()
    bar = 2 * n ** 3 * 2.0 ** -50 * float(np.max(d * d))
    ss_res = out["ss_total"] - out["ss_perm"][:, 0]
    assert np.max(np.abs(ss_res - ref["ssw_perm"])) <= bar
    assert out["ss_total"].hex() == ref["ss_total"].hex()
    assert out["terms"][0]["p"] == ref["p"]


def test_strata():
    n = 12
    d = points(n, 5)
    strata = [i // 3 for i in range(n)]
    idx = E.permanova_perms(n, strata=strata, seed=4, count=50)
    for row in idx:
        assert sorted(row.tolist()) == list(range(n)) and all(strata[row[i]] == strata[i] for i in range(n))
    assert (E.permanova_perms(n, strata=[0] * n, seed=4, count=50) == E.permanova_perms(n, seed=4, count=50)).all()
    two = E.permanova_perms(5, strata=[0, 1, 2, 1, 3], seed=4, count=64)
    assert {tuple(r) for r in two.tolist()} == {(0, 1, 2, 3, 4), (0, 3, 2, 1, 4)}
    # a design that is constant within the strata: every permutation is the observed design
    D = E.design_build(dict(g=strata), ["g"], factors=("g",))
    out = E.permanova_design(d, D["Q"], D["term_start"], strata=strata, perms=99, seed=4, host=True)
    assert out["terms"][0]["count_ge"] == 99 and out["terms"][0]["p"] == 1.0
    with pytest.raises(E.EngineError, match="every stratum is a single sample"):
        E.permanova_design(d, D["Q"], D["term_start"], strata=list(range(n)), perms=9, host=True)
    with pytest.raises(E.EngineError, match="not dense"):
        E.permanova_design(d, D["Q"], D["term_start"], strata=[0, 2] * 6, perms=9, host=True)
    with pytest.raises(E.EngineError, match="negative"):
        E.permanova_design(d, D["Q"], D["term_start"], strata=[0, -1] * 6, perms=9, host=True)


def test_ties_decide_p_at_four_samples():
    case = Case(points(4, 8), dict(g=["a", "b", "a", "b"]), ("g",), ["g"], 99, 3)
    assert 30 < case.count_ge[0] < 99                                               # three partitions: the observed one comes back often
    D, out = run_case(case, host=True)
    case.check(out, D)


def test_prefixes_and_chunks():
    whole = E.permanova_perms(9, strata=[0, 1, 0, 1, 0, 1, 0, 1, 0], seed=5, first=0, count=20)
    assert (E.permanova_perms(9, strata=[0, 1, 0, 1, 0, 1, 0, 1, 0], seed=5, first=13, count=7) == whole[13:]).all()
    case = cpu_case(7, "factor+covariate")
    outs = [run_case(case, host=True, chunk=c)[1] for c in (1, 7, 0)]
    assert all(o["ss_perm"].tobytes() == outs[0]["ss_perm"].tobytes() and o["terms"] == outs[0]["terms"] for o in outs)


def test_separated_clusters_against_random_labels():
    n = 24
    lab = [i % 2 for i in range(n)]
    d = points(n, 12, shift=[50.0 * l for l in lab])
    D = E.design_build(dict(g=lab), ["g"], factors=("g",))
    out = E.permanova_design(d, D["Q"], D["term_start"], perms=199, seed=2, host=True)
    assert out["terms"][0]["p"] == 1 / 200 and out["terms"][0]["R2"] > 0.99
    rnd = [int(v) for v in np.random.default_rng(3).permutation(lab)]
    D = E.design_build(dict(g=rnd), ["g"], factors=("g",))
    assert E.permanova_design(d, D["Q"], D["term_start"], perms=199, seed=2, host=True)["terms"][0]["p"] > 0.05


def test_first_principal_coordinate_as_covariate():
    n = 30
    rng = np.random.default_rng(21)
    x = rng.normal(size=(n, 4)) * np.array([5.0, 2.0, 1.0, 0.5])
    d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    pc = E.pcoa(d, k=1, host=True)
    D = E.design_build(dict(pc1=pc["coords"][:, 0].tolist()), ["pc1"])
    out = E.permanova_design(d, D["Q"], D["term_start"], perms=9, host=True)
    bar = n ** 3 * 2.0 ** -50 * float(np.max(d * d))
    assert abs(out["terms"][0]["R2"] - pc["prop"][0]) <= (bar + pc["resid"][0]) / out["ss_total"] + 2.0 ** -40


def test_refusals_of_the_call():
    d = points(6, 1)
    D = E.design_build(dict(c=covariate(6, 1)), ["c"])
    Q, ts = D["Q"], D["term_start"]
    for kw, why in ((dict(perms=0), "permutations"), (dict(perms=10 ** 7 + 1), "permutations"), (dict(chunk=-1), "chunk")):
        with pytest.raises(E.EngineError, match=why):
            E.permanova_design(d, Q, ts, **kw)
    bad = Q.copy(); bad[2, 0] = np.nan
    with pytest.raises(E.EngineError, match="not finite"):
        E.permanova_design(d, bad, ts)
    with pytest.raises(E.EngineError, match="term_start"):
        E.permanova_design(d, Q, [0, 2])
    with pytest.raises(E.EngineError, match="3 at the least"):
        E.permanova_design(d[:2, :2], Q[:2], ts)
    with pytest.raises(E.EngineError, match="residual degrees of freedom"):
        E.permanova_design(d[:3, :3], np.hstack([Q[:3], Q[:3]]), [0, 2])
    asym = d.copy(); asym[0, 1] += 1
    with pytest.raises(E.EngineError, match="not symmetric"):
        E.permanova_design(asym, Q, ts)
    need = E.permanova_design_need(6, 1, 1, 1)
    assert need == 8 * 36 + 2 * 6 * 64 + 8 * 6 + 8 * 64 + 8 * 64 + 8 * 64 + 4 * 13 + (1 << 20) and E.permanova_design_need(0, 1, 1, 1) == -1
    with pytest.raises(E.EngineError, match=r"need %d bytes.* 1000 bytes are free" % need) as e:
        E.permanova_design(d, Q, ts, chunk=1, mem_budget=1000)
    assert "device visible" not in str(e.value)


# ---- CPU: the program ----

def write_matrix(path, d, names):
    with open(path, "w") as f:
        f.write("".join("\t" + s for s in names) + "\n")
        for s, row in zip(names, d):
            f.write(s + "".join("\t%r" % float(v) for v in row) + "\n")


def write_meta(path, names, columns, header="sample", extra=""):
    with open(path, "w") as f:
        f.write(header + "".join("\t" + c for c in columns) + "\n\n# a comment\n" + extra)
        for i, s in enumerate(names):
            f.write(s + "".join("\t%s" % (repr(v[i]) if isinstance(v[i], float) else v[i]) for v in columns.values()) + "\n")


def parse_table(text):
    lines = text.strip().split("\n")
    assert lines[0] == "term\tdf\tSS\tR2\tF\tp"
    rows = {}
    for l in lines[1:]:
        if not l.startswith("#"):
            f = l.split("\t")
            assert len(f) == 6
            rows[f[0]] = f[1:]
    return rows, [l for l in lines if l.startswith("#")]


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pmd")
    case = cpu_case(7, "factor*covariate")
    names = ["s%d" % i for i in range(7)]
    write_matrix(tmp / "d.tsv", case.dist, names)
    cols = dict(g=case.variables["g"], c=case.variables["c"], code=[1, 2, 3, 1, 2, 3, 1], subj=["u", "u", "u", "v", "v", "v", "v"])
    write_meta(tmp / "meta.tsv", names, cols, header="#SampleID", extra="other\tL0\t0.5\t1\tu\n")
    return tmp, case, names, cols


def test_program_format_and_perm_out(study):
    tmp, case, names, cols = study
    r = _run([_bin(), tmp / "d.tsv", "--design", tmp / "meta.tsv", "--terms", "g,c,g:c", "--host", "-n", case.perms, "-S", case.seed, "--perm-out", tmp / "po.tsv", "-v"])
    assert r.returncode == 0, r.stderr
    rows, notes = parse_table(r.stdout)
    assert list(rows) == ["g", "c", "g:c", "Residual", "Total"] and notes == ["# perms: %d" % case.perms, "# seed: %d" % case.seed]
    D, out = run_case(case, host=True)
    for t, term in enumerate(case.terms):
        o = out["terms"][t]
        assert rows[term] == [str(o["df"]), "%.17g" % o["ss"], "%.17g" % o["R2"], "%.17g" % o["F"], "%.17g" % o["p"]]
    assert rows["Residual"] == [str(case.df_res), "%.17g" % out["ss_res"], "%.17g" % (out["ss_res"] / out["ss_total"]), "NA", "NA"]
    assert rows["Total"] == ["6", "%.17g" % out["ss_total"], "1", "NA", "NA"]
    assert "1 line(s)" in r.stderr and "term 'g:c': 2 column(s) kept, 0 dropped" in r.stderr and "F = NaN" in r.stderr
    po = open(tmp / "po.tsv").read().strip().split("\n")
    assert po[0] == "perm\tSS_g\tF_g\tSS_c\tF_c\tSS_g:c\tF_g:c" and len(po) == 1 + case.perms
    f = po[4].split("\t")
    assert f[0] == "3" and [f[1], f[3], f[5]] == ["%.17g" % v for v in out["ss_perm"][3]]
    res = out["ss_total"] - sum(out["ss_perm"][3])
    assert float(f[2]) == (out["ss_perm"][3][0] / case.df[0]) / (res / case.df_res)


def test_program_factor_strata_and_output_file(study):
    tmp, case, names, cols = study
    r = _run([_bin(), tmp / "d.tsv", "--design", tmp / "meta.tsv", "--terms", "code", "--host", "-n", 19])
    assert r.returncode == 0 and parse_table(r.stdout)[0]["code"][0] == "1"
    r = _run([_bin(), tmp / "d.tsv", "--design", tmp / "meta.tsv", "--terms", "code", "--factor", "code", "--strata", "subj", "--host", "-n", 19, "-o", tmp / "out.tsv"])
    assert r.returncode == 0 and r.stdout == ""
    rows, notes = parse_table(open(tmp / "out.tsv").read())
    assert rows["code"][0] == "2" and notes[-1] == "# strata: subj (2 blocks)"
    D = E.design_build(dict(code=cols["code"]), ["code"], factors=("code",))
    out = E.permanova_design(case.dist, D["Q"], D["term_start"], strata=first_levels(cols["subj"]), perms=19, host=True)
    assert rows["code"][1:] == ["%.17g" % out["terms"][0][k] for k in ("ss", "R2", "F", "p")]


def test_program_on_a_unifrac_matrix(tmp_path):
    """a matrix written by hmmufotu-amd-unifrac --host goes straight into the test"""
    rng = np.random.default_rng(4)
    counts = rng.integers(0, 40, (9, 6)); counts[0] += 1
    names = ["site %d" % j for j in range(6)]
    with open(tmp_path / "t.txt", "w") as f:
        f.write("# HmmUFOtu v1.5.1 OTU table generated by test\notuID\t" + "\t".join(names) + "\ttaxonomy\n")
        for i, row in enumerate(counts):
            f.write("%d\t%s\t\n" % (i, "\t".join(str(v) for v in row)))
    r = _run([_bin("hmmufotu-amd-unifrac"), tmp_path / "t.txt", "--method", "bray-curtis", "--host", "-o", tmp_path / "d.tsv"])
    assert r.returncode == 0, r.stderr
    write_meta(tmp_path / "m.tsv", names, dict(ph=[0.5, 1.5, 1.0, 3.0, 2.5, 4.0]))
    r = _run([_bin(), tmp_path / "d.tsv", "--design", tmp_path / "m.tsv", "--terms", "ph", "--host", "-n", 49])
    assert r.returncode == 0, r.stderr
    m = E.dist_matrix_read(tmp_path / "d.tsv")
    D = E.design_build(dict(ph=[0.5, 1.5, 1.0, 3.0, 2.5, 4.0]), ["ph"])
    out = E.permanova_design(m["dist"], D["Q"], D["term_start"], perms=49, host=True)
    assert parse_table(r.stdout)[0]["ph"][1] == "%.17g" % out["terms"][0]["ss"]


def test_program_refusals(study):
    tmp, case, names, cols = study
    d, meta = tmp / "d.tsv", tmp / "meta.tsv"
    with open(tmp / "groups.tsv", "w") as f:
        f.write("".join("%s\t%s\n" % (s, g) for s, g in zip(names, cols["g"])))

    def variant(name, edit):
        lines = open(meta).read().split("\n")
        open(tmp / name, "w").write("\n".join(edit(lines)))
        return tmp / name
    cases = [
        ([d, tmp / "groups.tsv", "--design", meta, "--terms", "g"], "GROUPS"),
        ([d, "--design", meta, "--terms", "g", "--pairwise"], "--pairwise"),
        ([d, tmp / "groups.tsv", "--terms", "g"], "need --design"),
        ([d, tmp / "groups.tsv", "--factor", "g"], "need --design"),
        ([d, tmp / "groups.tsv", "--strata", "g"], "need --design"),
        ([d, "--design", meta], "needs --terms"),
        ([d, "--design", meta, "--terms", "g,nope"], "'nope' is no column"),
        ([d, "--design", meta, "--terms", "g", "--factor", "nope"], "'nope' is no column"),
        ([d, "--design", meta, "--terms", "g", "--strata", "nope"], "'nope' is no column"),
        ([d, "--design", meta, "--terms", "g:c:code"], "more than two variables"),
        ([d, "--design", variant("m1.tsv", lambda l: [x for x in l if not x.startswith("s3\t")]), "--terms", "g"], "Sample 's3' of the matrix has no line"),
        ([d, "--design", variant("m2.tsv", lambda l: l + [[x for x in l if x.startswith("s3\t")][0], ""]), "--terms", "g"], "Sample 's3' is named twice"),
        ([d, "--design", variant("m3.tsv", lambda l: [x.replace("s2\t" + cols["g"][2], "s2\tNA") for x in l]), "--terms", "g"], "Sample 's2' has the NA value in column 'g'"),
        ([d, "--design", variant("m4.tsv", lambda l: [x.replace("s2\t" + cols["g"][2], "s2\t") for x in l]), "--terms", "c,g"], "Sample 's2' has an empty value in column 'g'"),
        ([d, "--design", variant("m5.tsv", lambda l: [x + "\tmore" if x.startswith("s4\t") else x for x in l]), "--terms", "g"], "line 9: 6 fields"),
        ([d, "--design", meta, "--terms", "g,c,g"], "term 'g' adds nothing"),
        ([d, "--design", meta, "--terms", "g,c,code,code:c", "--factor", "code"], "residual degrees of freedom"),
        ([d, "--design", meta, "--terms", "g", "--chunk", 1, "--mem", 1e-6], "bytes are free"),
    ]
    for k, (args, why) in enumerate(cases):
        out = tmp / ("refused%d.tsv" % k)
        r = _run([_bin()] + args + ["-o", out, "--perm-out", str(out) + ".perm"] + ([] if "--mem" in args else ["--host"]))
        assert r.returncode != 0 and why in r.stderr, (args, r.stderr)
        assert "device" not in r.stderr.replace("device memory", ""), r.stderr
        assert len(r.stderr.strip().split("\n")) == 1, r.stderr
        assert not os.path.exists(out) and not os.path.exists(str(out) + ".perm")
    r = _run([_bin(), d, "--design", meta, "--terms", "g", "--chunk", 1, "--mem", 1e-6])
    need = E.permanova_design_need(7, 2, 1, 1)
    assert "need %d bytes" % need in r.stderr and "%d bytes are free" % int(1e-6 * 2 ** 30) in r.stderr


def test_program_without_design_is_hu_permanova(study):
    tmp, case, names, cols = study
    with open(tmp / "groups2.tsv", "w") as f:
        f.write("".join("%s\t%s\n" % (s, g) for s, g in zip(names, cols["g"])))
    r = _run([_bin(), tmp / "d.tsv", tmp / "groups2.tsv", "--host", "-n", 29, "-S", 4])
    assert r.returncode == 0, r.stderr
    o = E.permanova(case.dist, first_levels(cols["g"]), perms=29, seed=4, host=True)
    want = "test\tn\tgroups\tperms\tSS_total\tSS_within\tSS_among\tF\tR2\tp\n" + "\t".join(
        ["all", str(o["n"]), str(o["a"]), "29"] + ["%.17g" % o[k] for k in ("ss_total", "ss_within", "ss_among", "F", "R2", "p")]) + "\n"
    assert r.stdout == want


def test_host_half_under_the_sanitizers(tmp_path):
    """the builder, the checks, the host path and the META reader as a stand-alone program under AddressSanitizer + UBSan"""
    exe = tmp_path / "permanova_design_driver"
    src = [os.path.join(ROOT, "tests", "san", "permanova_design_driver.cpp"), os.path.join(CSRC, "hu_permanova_design_host.cpp"), os.path.join(CSRC, "hu_permanova_host.cpp")]
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + src)
    assert r.returncode == 0, r.stderr
    r = _run([exe, tmp_path / "scratch.tsv"])
    assert r.returncode == 0 and "cases" in r.stdout, r.stdout + r.stderr


# ---- GPU ----

@functools.lru_cache(maxsize=None)
def gpu_case(name):
    if name == "n3":
        return Case(points(3, 41), dict(c=covariate(3, 1)), (), ["c"], 255, 2)                                         # q 1
    if name == "n4":
        return Case(points(4, 42), dict(g=["a", "b", "c", "a"]), ("g",), ["g"], 999, 3)                                # q 2, df_res 1
    if name == "n7":
        return Case(points(7, 43), dict(g=factor(7, 2, 7), c=covariate(7, 7)), ("g",), ["c", "g"], 256, 4)             # q 2, P 256
    if name == "n63":
        return Case(points(63, 44), dict(g=factor(63, 16, 1)), ("g",), ["g"], 17, 5)                              # q 15
    if name == "n64":
        return Case(points(64, 45), dict(g=factor(64, 17, 2)), ("g",), ["g"], 1, 6)                               # q 16, P 1
    if name == "n65":                                                                                                  # q 17 in four terms, P 257
        return Case(points(65, 46), dict(g=factor(65, 4, 3), c=covariate(65, 3), h=factor(65, 11, 4)), ("g", "h"), ["g", "c", "g:c", "h"], 257, 7)
    if name == "n129q33":
        return Case(points(129, 47), dict(g=factor(129, 34, 5)), ("g",), ["g"], 9, 8)
    if name == "n129q65":
        return Case(points(129, 48), dict(g=factor(129, 66, 6)), ("g",), ["g"], 5, 9)
    if name == "n280q65":
        return Case(points(280, 49), dict(g=factor(280, 66, 7)), ("g",), ["g"], 5, 10)
    if name == "n280strata":                                                                                           # q 2, strata of 7 blocks
        return Case(points(280, 50), dict(g=factor(280, 2, 8), c=covariate(280, 8)), ("g",), ["c", "g"], 40, 11, strata=[i % 7 for i in range(280)])
    raise KeyError(name)


GPU_CHUNKS = {"n3": (1, 256, 300, 0), "n4": (256, 300, 0), "n7": (1, 256, 0), "n63": (0,), "n64": (0,), "n65": (256, 300, 0), "n129q33": (0, 1), "n129q65": (0, 2),
              "n280q65": (0, 3), "n280strata": (0, 7)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GPU_CHUNKS))
def test_device_against_the_yardstick(name):
    _need_gpu()
    case = gpu_case(name)
    assert case.q == {"n3": 1, "n4": 2, "n7": 2, "n63": 15, "n64": 16, "n65": 17, "n129q33": 33, "n129q65": 65, "n280q65": 65, "n280strata": 2}[name]
    if case.n == 280:
        assert E.pcoa_slabs(280) == 3                                              # more than one K slab
    first = None
    for chunk in GPU_CHUNKS[name]:
        D, out = run_case(case, chunk=chunk)
        err = case.check(out, D)
        print("%s chunk %d: %.3g bars from the yardstick" % (name, chunk, err))
        if first is None:
            first = out
            host = run_case(case, host=True)[1]
            gap = max(abs(out["ss_perm"][p][t] - host["ss_perm"][p][t]) / case.bar[t] for p in range(case.perms) for t in range(len(case.terms)))
            assert gap <= 2, "the device is %g bars from the host path" % gap
            again = run_case(case, chunk=chunk)[1]
            assert again["ss_perm"].tobytes() == out["ss_perm"].tobytes() and again["terms"] == out["terms"]
        assert out["ss_perm"].tobytes() == first["ss_perm"].tobytes() and out["terms"] == first["terms"], "chunk %d gives other bytes" % chunk


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n65", "n280strata"])
def test_device_index_entries_of_32_bits(name):
    _need_gpu()
    case = gpu_case(name)
    a = run_case(case)[1]; b = run_case(case, index32=True)[1]
    assert a["ss_perm"].tobytes() == b["ss_perm"].tobytes() and a["terms"] == b["terms"]
    assert E.permanova_design_need(case.n, case.q, len(case.terms), 64, True) - E.permanova_design_need(case.n, case.q, len(case.terms), 64) == 2 * case.n * 64


@pytest.mark.gpu
def test_device_strata_are_those_of_permanova_perms():
    """a design whose only term is the covariate i reveals the index array: SS(p) follows from permanova_perms"""
    _need_gpu()
    n, perms = 129, 70
    d = points(n, 61)
    strata = [i % 5 for i in range(n)]
    D = E.design_build(dict(i=[float(i) for i in range(n)]), ["i"])
    out = E.permanova_design(d, D["Q"], D["term_start"], strata=strata, perms=perms, seed=13)
    idx = E.permanova_perms(n, strata=strata, seed=13, count=perms)
    bar = n ** 3 * 2.0 ** -50 * float(np.max(d * d))
    D2 = (d * d).astype(np.longdouble)
    for p in range(perms):
        v = D["Q"][idx[p], 0].astype(np.longdouble)
        assert abs(float(-0.5 * (v @ D2 @ v)) - out["ss_perm"][p, 0]) <= bar
    free = E.permanova_design(d, D["Q"], D["term_start"], perms=perms, seed=13)
    assert np.min(np.abs(free["ss_perm"] - out["ss_perm"])) > 100 * bar                # another index array is far away


@pytest.mark.gpu
def test_device_memory_refusal_and_budget():
    _need_gpu()
    case = gpu_case("n65")
    D = case.build()
    T = len(case.terms)
    need1 = E.permanova_design_need(case.n, case.q, T, 1)
    with pytest.raises(E.EngineError, match=r"need %d bytes.* %d bytes are free" % (need1, need1 - 1)):
        E.permanova_design(case.dist, D["Q"], D["term_start"], perms=case.perms, seed=case.seed, mem_budget=need1 - 1)
    # the default chunk of 257 permutations is 320 slots; a budget that holds 64 but not 128 shrinks it, and the bytes stay
    assert E.permanova_design_need(case.n, case.q, T, 128) > E.permanova_design_need(case.n, case.q, T, 64) + 1000
    small = E.permanova_design(case.dist, D["Q"], D["term_start"], perms=case.perms, seed=case.seed, mem_budget=E.permanova_design_need(case.n, case.q, T, 64) + 1000)
    assert small["ss_perm"].tobytes() == run_case(case)[1]["ss_perm"].tobytes()


@pytest.mark.gpu
def test_program_on_the_device_against_host(study):
    _need_gpu()
    tmp, case, names, cols = study
    args = [_bin(), tmp / "d.tsv", "--design", tmp / "meta.tsv", "--terms", "g,c,g:c", "-n", case.perms, "-S", case.seed]
    dev = _run(args + ["-v"]); host = _run(args + ["--host"])
    assert dev.returncode == 0 and host.returncode == 0, dev.stderr + host.stderr
    assert "quadratic forms" in dev.stderr
    a, b = parse_table(dev.stdout)[0], parse_table(host.stdout)[0]
    for t, term in enumerate(case.terms):
        assert a[term][0] == b[term][0] and a[term][4] == b[term][4]
        assert abs(float(a[term][1]) - float(b[term][1])) <= 2 * case.bar[t]
        assert abs(Fraction(float(a[term][1])) - case.obs[t]) <= case.bar[t]
