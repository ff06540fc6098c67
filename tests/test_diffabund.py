"""hmmufotu-amd-diffabund: Kruskal-Wallis per OTU between the sample groups by permutation, hu_diffabund on the host and
on the device, and the program.

The yardstick is a restatement that shares no code with the library: Philox4x32-10 and the Fisher-Yates shuffle in plain Python
integers (checked against hu_sim_philox on a few counters), the doubled mid-ranks from their definition (counting the cells below and
equal; the fractions are the rounded quotients the definition names, and doubles compare as the rationals they are), the group sums
and T of the observed labelling and of every permutation as exact Python integers.  So count_ge and p are compared exactly, with no
tolerance and no condition on the fixtures.  H, M(pi), p_maxT and q are restated with the same plain float operations and compared bit
for bit.

scipy, where it imports (CPU tests only; DESIGN.md §31 derives the bound).  With u = 2^-53: H takes one conversion of T, two
divisions and a product (4 roundings), tc a division and a subtraction, which the division by tc carries over at most doubled where
tc >= 1/2, as in the fixtures held to scipy: |H - exact| <= 8 u H.  scipy.stats.kruskal computes A - 3 (N + 1) with
A = 12 / (N (N + 1)) sum R_g^2 / n_g, near 3 (N + 1) + H tc, from a + 4 rounded operations (a quotients, a - 1 adds, the factor's product
and quotient, the product with it), subtracts, and divides by its tc (2 more): |scipy - exact| <= (a + 6) u (H tc + 3 (N + 1)) / tc.
The test holds |H - scipy| to the sum of the two.  The largest difference seen is 0.20 of that bound (printed by the test); no margin is
taken over a measurement.  For a == 2 the same H against mannwhitneyu's U, which is exact, through
H = (U - n0 n1 / 2)^2 / (n0 n1 (N + 1) tc / 12): six rounded operations on the test's side and the 8 u above, held to 16 u H."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
HEADER = "otu\tprevalence\tH\tp\tp_maxT\tq\tbest\ttaxonomy"
M32 = 0xffffffff
M64 = (1 << 64) - 1
BLOCK = 64          # tested OTUs per workgroup of k_da_sums
STAGE = 1024        # cells of a row staged in LDS at a time


def _bin(name="hmmufotu-amd-diffabund"):
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


def shuffled(labels, seed, p):
    g = list(labels)
    for i in range(len(g) - 1, 0, -1):
        w = philox((i & M32, i >> 32, p & M32, p >> 32), (seed & M32, (seed >> 32) & M32))
        j = ((((w[1] << 32) | w[0]) * (i + 1)) >> 64)
        g[i], g[j] = g[j], g[i]
    return g


def lcm(xs):
    import math
    L = 1
    for x in xs:
        L = L // math.gcd(L, x) * x
    return L


def values(counts, rank_by):
    """x [n_otu][n_sample]: the counts, or their rounded quotients by the column sums added in ascending OTU order"""
    c = np.asarray(counts, np.float64)
    if rank_by == "count":
        return c
    tot = np.zeros(c.shape[1])
    for row in c:
        tot = tot + row
    return c / tot


def ranks2(x):
    """the doubled mid-ranks of one row, from the definition"""
    x = np.asarray(x)
    return (2 * (x[None, :] < x[:, None]).sum(1) + (x[None, :] == x[:, None]).sum(1) + 1).astype(np.int64)


def H_of(T, L, N, tc):
    x = float(T >> 64) * 18446744073709551616.0 + float(T & M64)
    return ((x / float(L)) * (3.0 / (float(N) * float(N + 1)))) / tc


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


class Yard:
    """everything hu_diffabund reports for (counts, group, perms, seed), restated"""

    def __init__(self, counts, group, perms, seed, rank_by="fraction", min_prevalence=1):
        c = np.asarray(counts, np.float64)
        self.counts = c; self.group = [int(v) for v in group]; self.perms = perms; self.seed = seed; self.rank_by = rank_by; self.min_prevalence = min_prevalence
        M, N = c.shape
        self.N = N; self.a = a = max(self.group) + 1
        self.sizes = sizes = [self.group.count(k) for k in range(a)]
        self.L = L = lcm(sizes)
        x = values(c, rank_by)
        self.r2 = np.array([ranks2(row) for row in x])
        e = self.r2 - (N + 1)
        assert (e.sum(1) == 0).all()
        self.prevalence = (c != 0).sum(1)
        self.tc = []
        for row in x:
            _, t = np.unique(row, return_counts=True)
            self.tc.append(1.0 - float(int((t.astype(object) ** 3 - t).sum())) / float(N ** 3 - N))
        self.tested = [self.tc[i] != 0 and self.prevalence[i] >= min_prevalence for i in range(M)]
        self.labels = [self.group] + [shuffled(self.group, seed, p) for p in range(perms)]
        onehot = (np.asarray(self.labels)[:, :, None] == np.arange(a)[None, None, :]).astype(np.int64)     # [1 + P][N][a]
        rows = [i for i in range(M) if self.tested[i]]
        C = np.einsum("mn,pna->mpa", e[rows], onehot)                                                      # exact: |C| <= N^2
        w = np.array([L // s for s in sizes], dtype=object)
        T = ((C.astype(object) ** 2) * w[None, None, :]).sum(2)                                            # [m][1 + P] Python integers
        self.T = {i: int(T[k, 0]) for k, i in enumerate(rows)}
        self.Tperm = {i: [int(v) for v in T[k, 1:]] for k, i in enumerate(rows)}
        self.count_ge = {i: sum(1 for v in self.Tperm[i] if v >= self.T[i]) for i in rows}
        self.H = {i: H_of(self.T[i], L, N, self.tc[i]) for i in rows}
        self.max_H = [max(H_of(self.Tperm[i][p], L, N, self.tc[i]) for i in rows) for p in range(perms)] if rows else []
        self.p = {i: float(1 + self.count_ge[i]) / float(perms + 1) for i in rows}
        self.p_maxT = {i: float(1 + sum(1 for v in self.max_H if v >= self.H[i])) / float(perms + 1) for i in rows}
        order = sorted(rows, key=lambda i: self.p[i])                                                      # stable: by OTU order among equals
        m = len(rows); run = 1.0; self.q = {}
        for j in range(m, 0, -1):
            i = order[j - 1]
            run = min(run, (self.p[i] * float(m)) / float(j))
            self.q[i] = run
        self.best = {}
        for k, i in enumerate(rows):
            b = 0
            for g in range(1, a):
                if int(C[k, 0, g]) * sizes[b] > int(C[k, 0, b]) * sizes[g]:
                    b = g
            self.best[i] = b
        self.rows = rows


def call(y, **kw):
    kw.setdefault("host", True)
    return E.diffabund(y.counts, y.group, perms=y.perms, seed=y.seed, rank_by=y.rank_by, min_prevalence=y.min_prevalence, **kw)


def hold(r, y, what=""):
    """every field of every record and every M(pi) against the restatement: integers exactly, doubles bit for bit"""
    rec = r["rec"]
    assert rec["prevalence"].tolist() == y.prevalence.tolist(), what
    assert rec["tested"].tolist() == [1 if t else 0 for t in y.tested], what
    for i in range(len(rec)):
        x = rec[i]
        if not y.tested[i]:
            assert x["best"] == -1 and x["count_ge"] == 0 and all(np.isnan(x[k]) for k in ("H", "p", "p_maxT", "q")), "%s OTU %d" % (what, i)
            continue
        assert (int(x["T_hi"]) << 64) | int(x["T_lo"]) == y.T[i], "%s OTU %d: T" % (what, i)
        assert int(x["count_ge"]) == y.count_ge[i], "%s OTU %d: count_ge %d, restated %d" % (what, i, x["count_ge"], y.count_ge[i])
        for k, want in (("p", y.p[i]), ("H", y.H[i]), ("p_maxT", y.p_maxT[i]), ("q", y.q[i])):
            assert bits(x[k]) == bits(want), "%s OTU %d: %s %r, restated %r" % (what, i, k, x[k], want)
        assert int(x["best"]) == y.best[i], "%s OTU %d: best" % (what, i)
    assert np.array_equal(bits(r["max_H"]), bits(y.max_H)), what


def same_bytes(x, y):
    return x["rec"].tobytes() == y["rec"].tobytes() and x["max_H"].tobytes() == y["max_H"].tobytes()


def groups(n, a, seed):
    """labels 0 .. a-1, dense, every group used, unbalanced: a label is drawn in proportion to its number plus one"""
    rng = np.random.default_rng(seed + 1000)
    g = list(range(a)) + rng.choice(a, n - a, p=np.arange(1, a + 1) / (a * (a + 1) / 2)).tolist()
    return [int(v) for v in rng.permutation(g)]


def table(n_otu, n, seed, density=0.3, special=True):
    """sparse counts with ties, samples of unequal depth; with `special` the first rows are: all zero, a single nonzero cell, every cell
    nonzero and distinct, every cell equal, and heavy ties (two values)"""
    rng = np.random.default_rng(seed)
    depth = rng.integers(1, 6, n)
    c = (rng.random((n_otu, n)) < density) * rng.integers(1, 5, (n_otu, n)) * depth[None, :]
    c = c.astype(np.float64)
    c[-1] += 1.0                                                                 # no sample without reads
    if special and n_otu >= 6:
        c[0] = 0; c[1] = 0; c[1, n // 2] = 3
        c[2] = (rng.permutation(n) + 1) * 1000.0
        c[3] = 7
        c[4] = np.where(rng.random(n) < 0.5, 2.0, 4.0) * depth
    return c


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(n_otu, n, a, perms, seed=5, density=0.3, **kw):
        key = (n_otu, n, a, perms, seed, density, tuple(sorted(kw.items())))
        if key not in memo:
            memo[key] = Yard(table(n_otu, n, seed + n, density), groups(n, a, seed), perms, seed, **kw)
        return memo[key]
    return get


# ---- the restatement against the library's pieces ----

def test_the_restated_philox_is_the_librarys():
    rng = np.random.default_rng(1)
    for _ in range(6):
        ctr = [int(v) for v in rng.integers(0, 2 ** 32, 4)]; key = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        assert E.sim_philox(ctr, key).tolist() == philox(ctr, key)


def test_labellings_are_those_of_permanova():
    for n, a, seed in ((3, 2, 1), (7, 3, 2), (65, 5, (1 << 63) + 12345)):
        g = groups(n, a, 3)
        got = E.permanova_labels(g, seed=seed, first=0, count=9)
        assert got.tolist() == [shuffled(g, seed, p) for p in range(9)]


def test_ranks_are_the_definition():
    c = table(12, 17, 3)
    for rank_by in ("fraction", "count"):
        got = E.diffabund_ranks(c, rank_by)
        assert got.dtype == np.int32 and got.tolist() == [ranks2(row).tolist() for row in values(c, rank_by)]
    assert E.diffabund_ranks([[0, 0, 5, 0, 5, 5], [3, 1, 2, 2, 0, 0]], "count").tolist() == [[4, 4, 10, 4, 10, 10], [12, 6, 9, 9, 3, 3]]


# ---- six samples and four OTUs by hand ----

def test_six_samples_by_hand():
    """groups {0, 1, 2} and {3, 4, 5}, ranked by count, L = 3.
    A = 1 2 3 4 5 6: r2 = 2 4 .. 12, e = -5 -3 -1 1 3 5, C = (-9, 9), T = 81 + 81 = 162, no ties, H = (162 / 3) (3 / 42) = 27 / 7.
    B = all zero: not tested.
    C = 0 0 5 0 5 5: the zeros r2 = 4, the fives r2 = 2 x 3 + 3 + 1 = 10, e = -3 -3 3 -3 3 3, C = (-3, 3), T = 18,
        ties 2 (27 - 3) = 48, tc = 1 - 48 / 210 = 27 / 35, H = (18 / 3) (3 / 42) / tc = 5 / 9.
    D = all 7: every cell ties, not tested, prevalence 6."""
    c = [[1, 2, 3, 4, 5, 6], [0] * 6, [0, 0, 5, 0, 5, 5], [7] * 6]
    g = [0, 0, 0, 1, 1, 1]
    r = E.diffabund(c, g, perms=99, seed=1, rank_by="count", host=True)
    rec = r["rec"]
    assert rec["tested"].tolist() == [1, 0, 1, 0] and rec["prevalence"].tolist() == [6, 0, 3, 6] and rec["best"].tolist() == [1, -1, 1, -1]
    assert rec["T_hi"].tolist() == [0, 0, 0, 0] and rec["T_lo"].tolist() == [162, 0, 18, 0]
    assert rec["H"][0] == ((162.0 / 3.0) * (3.0 / 42.0)) / 1.0 and abs(rec["H"][0] - 27 / 7) < 1e-15
    assert rec["H"][2] == ((18.0 / 3.0) * (3.0 / 42.0)) / (1.0 - 48.0 / 210.0) and abs(rec["H"][2] - 5 / 9) < 1e-15
    # A: T >= 162 only for the two labellings that split {1, 2, 3} from {4, 5, 6}
    lab = [shuffled(g, 1, p) for p in range(99)]
    extreme = sum(1 for l in lab if l in ([0, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 0]))
    assert rec["count_ge"][0] == extreme and rec["p"][0] == (1 + extreme) / 100
    hold(r, Yard(c, g, 99, 1, rank_by="count"), "by hand")


# ---- the host path against the restatement ----

SHAPES = [(3, 2), (4, 2), (4, 3), (7, 2), (7, 3), (7, 6), (65, 2), (65, 3), (65, 64)]


@pytest.mark.parametrize("n,a", SHAPES)
@pytest.mark.parametrize("perms", [1, 99])
def test_host_against_the_restatement(cases, n, a, perms):
    y = cases(9, n, a, perms)
    hold(call(y), y, "n %d a %d P %d" % (n, a, perms))


def test_host_999_permutations_and_the_chunk(cases):
    y = cases(9, 65, 3, 999)
    r = call(y)
    hold(r, y, "P 999")
    for chunk in (1, 7):
        assert same_bytes(call(y, chunk=chunk), r)


def test_ties_decide_p_at_three_and_four_samples(cases):
    """at n = 3 and 4 there are a handful of partitions, so most permutations give the observed T exactly"""
    for n, a in ((3, 2), (4, 2), (4, 3)):
        y = cases(9, n, a, 99)
        assert any(sum(1 for v in y.Tperm[i] if v == y.T[i]) > 10 for i in y.rows)
        hold(call(y), y, "ties n %d" % n)


def test_equal_groups_that_swap():
    """three groups of three, an OTU present in two samples: a relabelling that swaps groups gives the same T, which a floating-point
    sum of C_g^2 / n_g in another order need not"""
    g = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    c = np.zeros((3, 9)); c[0, 1] = 4; c[0, 5] = 9; c[1] = [3, 1, 4, 1, 5, 9, 2, 6, 5]; c[2] = 1
    y = Yard(c, g, 299, 4)
    assert sum(1 for v in y.Tperm[0] if v == y.T[0]) > 50 and 0 < y.count_ge[0] <= 299
    hold(call(y), y, "swaps")


def test_a_group_of_one_and_unbalanced_groups():
    c = table(8, 9, 11)
    for g in ([0, 1, 1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1, 2], [2, 0, 1, 0, 0, 0, 0, 0, 0]):
        y = Yard(c, g, 99, 2)
        hold(call(y), y, str(g))


def test_count_against_fraction_on_unequal_depths():
    c = np.array([[10.0, 1, 30, 2, 50, 3], [5, 5, 5, 5, 5, 5], [85, 4, 65, 3, 45, 2]])
    g = [0, 0, 0, 1, 1, 1]
    assert E.diffabund_ranks(c, "count")[1].tolist() == [7] * 6                   # equal counts tie, their fractions do not
    assert len(set(E.diffabund_ranks(c, "fraction")[1].tolist())) > 1
    yc, yf = Yard(c, g, 99, 1, rank_by="count"), Yard(c, g, 99, 1)
    assert yc.tested == [True, False, True] and yf.tested == [True, True, True]
    hold(call(yc), yc, "count"); hold(call(yf), yf, "fraction")


def test_min_prevalence(cases):
    c = table(12, 17, 8, density=0.2)
    g = groups(17, 3, 1)
    y1, y4 = Yard(c, g, 99, 1), Yard(c, g, 99, 1, min_prevalence=4)
    assert sum(y4.tested) < sum(y1.tested) and sum(y4.tested) > 0
    hold(call(y1), y1, "prevalence 1"); hold(call(y4), y4, "prevalence 4")
    y0 = Yard(c, g, 9, 1, min_prevalence=0)
    assert y0.tested == y1.tested                                                 # an OTU whose cells all tie stays untested
    hold(call(y0), y0, "prevalence 0")


def test_a_large_least_common_multiple():
    """groups of the first 15 primes: 328 samples, L = 614,889,782,588,491,410 < 2^64, T beyond 64 bits; the 16th prime is refused"""
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53]
    g = [k for k, s in enumerate(primes[:15]) for _ in range(s)]
    y = Yard(table(6, 328, 2, special=False), g, 9, 1)
    assert y.L == 614889782588491410 and max(y.T.values()) >> 64 > 0
    hold(call(y), y, "large L")
    g = [k for k, s in enumerate(primes) for _ in range(s)]
    with pytest.raises(E.EngineError, match=r"least common multiple of the group sizes \(2, 3, 5, .*, 53\) is 2\^64 or more") as ei:
        E.diffabund(table(3, 381, 2, special=False), g, perms=1, host=True)
    assert "error -1" in str(ei.value) and "device" not in str(ei.value)


def test_a_planted_otu_has_the_smallest_p_maxT():
    rng = np.random.default_rng(7)
    n = 24; g = [0] * 12 + [1] * 12
    c = rng.integers(0, 20, (40, n)).astype(np.float64)
    c[17, :12] = rng.integers(0, 5, 12); c[17, 12:] = rng.integers(500, 600, 12)
    # ranked by count: under fractions the planted reads would lower every other OTU's share in group 1, and those would differ too
    r = E.diffabund(c, g, perms=999, seed=3, rank_by="count", host=True)["rec"]
    assert r["p_maxT"].argmin() == 17 and r["p_maxT"][17] == 1 / 1000 and r["best"][17] == 1
    assert (np.delete(r["p_maxT"], 17) > 0.05).all() and r["q"][17] <= 0.05


def test_need_is_the_documented_formula():
    for n, a, m, cells, chunk in ((3, 2, 1, 2, 1), (65, 3, 64, 900, 256), (129, 64, 65, 5000, 257), (16384, 8, 100000, 5 * 10 ** 6, 9999)):
        c = -(-chunk // 256) * 256; b = -(-m // 64)
        assert E.diffabund_need(n, a, m, cells, chunk) == 4 * cells + n * c + 8 * b * c + 8 * c + n + 16 * a + 52 * m + 8 + (1 << 20)
    assert E.diffabund_need(0, 2, 1, 1, 1) == -1 and E.diffabund_need(16385, 2, 1, 1, 1) == -1 and E.diffabund_need(9, 65, 1, 1, 1) == -1


def test_what_the_library_refuses():
    c = table(6, 5, 1); g = [0, 1, 0, 1, 1]

    def bad(why, counts=c, group=g, **kw):
        kw.setdefault("host", True)
        with pytest.raises(E.EngineError, match=why) as ei:
            E.diffabund(counts, group, **kw)
        assert "error -1" in str(ei.value) and "device" not in str(ei.value)
    bad("3 at the least", counts=c[:, :2], group=[0, 1])
    bad("16385 samples: 16384 at the most", counts=np.ones((1, 16385)), group=[0, 1] * 8192 + [0], perms=1)
    bad("negative label", group=[0, -1, 0, 1, 1])
    bad("not dense", group=[0, 2, 0, 2, 2])
    bad("not dense", group=[0, 7, 0, 1, 1])
    bad("one group", group=[0] * 5)
    bad("every group is a single sample", group=[0, 1, 2, 3, 4])
    bad("65 groups: 64 at the most", counts=np.ones((1, 70)), group=list(range(65)) + [0] * 5)
    bad("permutations", perms=0)
    bad("permutations", perms=10 ** 7 + 1)
    bad("chunk", chunk=-1)
    bad("min_prevalence", min_prevalence=-1)
    for v in (-1.0, np.nan, np.inf):
        x = c.copy(); x[1, 3] = v
        bad("OTU 1 and sample 3 is negative or not finite", counts=x)
    x = c.copy(); x[:, 2] = 0
    bad("sample 2 has no reads", counts=x)
    assert E.diffabund(x, g, perms=9, rank_by="count", host=True)["rec"]["tested"].sum() > 0
    bad("no OTU is left to test", counts=np.ones((3, 5)))
    bad("no OTU is left to test", min_prevalence=6)
    for dev in (False, True):                                                     # every refusal comes before a device is asked for
        bad("chunk", chunk=-1, host=not dev)
        bad("no OTU is left to test", counts=np.ones((3, 5)), host=not dev)
    with pytest.raises(E.EngineError, match="counts"):
        E.diffabund(c, [0, 1])
    with pytest.raises(E.EngineError, match="rank_by"):
        E.diffabund(c, g, rank_by="clr")


def test_memory_refusal_names_both_numbers(cases):
    y = cases(9, 65, 3, 99)
    m = len(y.rows); cells = int(sum((values(y.counts, "fraction")[i] > 0).sum() for i in y.rows))
    with pytest.raises(E.EngineError, match=r"need (\d+) bytes .*, 1048576 bytes are free") as ei:
        call(y, host=False, mem_budget=1 << 20)
    assert "error -4" in str(ei.value) and "device" not in str(ei.value)
    assert int(str(ei.value).split("need ")[1].split(" ")[0]) == E.diffabund_need(65, 3, m, cells, 1)
    with pytest.raises(E.EngineError, match=r"chunk of 99 permutations need %d bytes" % E.diffabund_need(65, 3, m, cells, 99)):
        call(y, host=False, mem_budget=1 << 20, chunk=300)                          # a chunk is never more than the permutations


# ---- scipy, where it imports ----

def test_observed_H_against_scipy():
    st = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(3)
    worst = 0.0
    for n, a in ((7, 2), (24, 2), (24, 3), (65, 5)):
        g = groups(n, a, 2)
        free = np.array([rng.permutation(n) + 1.0 for _ in range(4)])             # tie-free
        tied = rng.integers(0, 4, (4, n)).astype(np.float64)                      # heavy ties, tc >= 1/2
        c = np.vstack([free, tied])
        rec = E.diffabund(c, g, perms=1, rank_by="count", host=True)["rec"]
        for i, row in enumerate(c):
            assert rec["tested"][i] == 1
            parts = [row[np.asarray(g) == k] for k in range(a)]
            want = st.kruskal(*parts).statistic
            _, t = np.unique(row, return_counts=True)
            tc = 1 - float((t ** 3 - t).sum()) / (n ** 3 - n)
            assert tc >= 0.5
            bound = 8 * 2.0 ** -53 * want + (a + 6) * 2.0 ** -53 * (want * tc + 3 * (n + 1)) / tc
            worst = max(worst, abs(rec["H"][i] - want) / bound)
            assert abs(rec["H"][i] - want) <= bound, (n, a, i, rec["H"][i], want, bound)
            if a == 2:
                n0, n1 = len(parts[0]), len(parts[1])
                U = st.mannwhitneyu(parts[0], parts[1], alternative="two-sided", method="asymptotic", use_continuity=False).statistic
                hu = (U - n0 * n1 / 2) ** 2 / (n0 * n1 * (n + 1) * tc / 12)
                assert abs(rec["H"][i] - hu) <= 16 * 2.0 ** -53 * hu, (n, i, rec["H"][i], hu)
    print("largest difference from scipy.stats.kruskal, as a share of the bound: %.3g" % worst)


# ---- the program ----

NAMES6 = ["s1", "s2", "s3", "s4", "s5", "s6"]


def _write_table(path, counts, names, taxa=None):
    with open(path, "w") as f:
        f.write("# HmmUFOtu v1.5.1 OTU table generated by test\notuID\t" + "\t".join(names) + "\ttaxonomy\n")
        for i, row in enumerate(counts):
            f.write("%d\t%s\t%s\n" % (100 + i, "\t".join("%.15g" % v for v in row), taxa[i] if taxa else "taxon %d" % i))
    return path


def _write_groups(path, names, labels, extra=""):
    with open(path, "w") as f:
        f.write("# sample\tgroup\n\n" + extra + "".join("%s\t%s\n" % (s, l) for s, l in zip(names, labels)))
    return path


def _parse(text):
    lines = text.split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    body = [l for l in lines[1:-1] if not l.startswith("#")]
    foot = [l for l in lines[1:-1] if l.startswith("#")]
    assert lines[1:-1] == body + foot
    return [l.split("\t") for l in body], foot


def _hold_program(rows, foot, y, gnames, perms, seed):
    assert foot == ["# tested: %d of %d" % (len(y.rows), len(y.tested)), "# perms: %d" % perms, "# seed: %d" % seed]
    for i, f in enumerate(rows):
        assert f[0] == str(100 + i) and int(f[1]) == y.prevalence[i] and f[7] == "taxon %d" % i
        if y.tested[i]:
            assert [float(v) for v in f[2:6]] == [y.H[i], y.p[i], y.p_maxT[i], y.q[i]] and f[6] == gnames[y.best[i]]
            assert all(v == "%.17g" % float(v) for v in f[2:6])
        else:
            assert f[2:7] == ["NA"] * 5


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    t = tmp_path_factory.mktemp("diffabund")
    n = 11
    names = ["sample %d" % j for j in range(n)]
    c = table(9, n, 4)
    g = groups(n, 3, 9)
    gnames = ["soil", "gut", "sea water"]
    first = []                                                                    # groups are numbered by first appearance among the table's samples
    for v in g:
        if v not in first:
            first.append(v)
    lab = [first.index(v) for v in g]
    _write_table(t / "table.txt", c, names)
    _write_groups(t / "groups.txt", names[::-1], [gnames[v] for v in lab[::-1]], extra="elsewhere\tgut\nelsewhere 2\tmoon\n")
    return dict(dir=t, counts=c, names=names, labels=lab, gnames=gnames)


def test_program_on_the_host(study):
    t = study["dir"]
    y = Yard(study["counts"], study["labels"], 199, 7)
    r = _run([_bin(), t / "table.txt", t / "groups.txt", "-n", 199, "-S", 7, "--host", "-o", t / "host.txt", "--perm-out", t / "host_perm.txt", "-v"])
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert "2 line(s)" in r.stderr and "%d OTU(s) tested, %d not tested" % (len(y.rows), 9 - len(y.rows)) in r.stderr
    rows, foot = _parse((t / "host.txt").read_text())
    assert len(rows) == 9 and sum(1 for f in rows if f[2] == "NA") == 9 - len(y.rows) >= 1
    _hold_program(rows, foot, y, study["gnames"], 199, 7)
    perm = (t / "host_perm.txt").read_text().split("\n")
    assert perm[0] == "perm\tmax_H" and perm[-1] == "" and len(perm) == 201
    assert [l.split("\t")[0] for l in perm[1:-1]] == [str(p) for p in range(199)] and [float(l.split("\t")[1]) for l in perm[1:-1]] == y.max_H
    s = _run([_bin(), t / "table.txt", t / "groups.txt", "--perms", 199, "--seed", 7, "--host", "--chunk", 7])
    assert s.returncode == 0 and s.stdout == (t / "host.txt").read_text()           # without -o: the standard output
    yc = Yard(study["counts"], study["labels"], 99, 1, rank_by="count", min_prevalence=3)
    r = _run([_bin(), t / "table.txt", t / "groups.txt", "-n", 99, "--rank-by", "count", "--min-prevalence", 3, "--host"])
    assert r.returncode == 0, r.stderr
    assert yc.tested[3] is False and yc.tested.count(False) > y.tested.count(False)   # the row of equal counts, and the rows below the floor
    _hold_program(*_parse(r.stdout), yc, study["gnames"], 99, 1)


def test_program_ignore_missing(study, tmp_path):
    """two groups of a larger study: the samples without a line are left out, totals included"""
    t = study["dir"]
    keep = [j for j, v in enumerate(study["labels"]) if v != 1]
    names = [study["names"][j] for j in keep]
    lab = [0 if study["labels"][j] == study["labels"][keep[0]] else 1 for j in keep]
    gn = [study["gnames"][study["labels"][keep[0]]]]; gn.append([study["gnames"][study["labels"][j]] for j in keep if study["gnames"][study["labels"][j]] != gn[0]][0])
    _write_groups(tmp_path / "g.txt", names, [gn[v] for v in lab])
    r = _run([_bin(), t / "table.txt", tmp_path / "g.txt", "-n", 99, "--host", "-o", tmp_path / "o.txt"])
    assert r.returncode != 0 and "of the table has no line" in r.stderr and "device" not in r.stderr and not (tmp_path / "o.txt").exists()
    r = _run([_bin(), t / "table.txt", tmp_path / "g.txt", "-n", 99, "--host", "--ignore-missing", "-v"])
    assert r.returncode == 0 and "%d sample(s) of the table have no line" % (11 - len(keep)) in r.stderr, r.stderr
    _hold_program(*_parse(r.stdout), Yard(study["counts"][:, keep], lab, 99, 1), gn, 99, 1)


def test_program_reads_what_subset_writes(study, tmp_path):
    t = study["dir"]
    big = study["counts"] * 10 + 1
    _write_table(tmp_path / "big.txt", big, study["names"])
    s = _run([_bin("hmmufotu-amd-subset"), tmp_path / "big.txt", tmp_path / "sub.txt", "-s", 30, "-S", 5, "--host"])
    assert s.returncode == 0, s.stderr
    sub = E.otu_table_read(tmp_path / "sub.txt")
    assert sub["samples"] == study["names"] and (np.asarray(sub["counts"]).sum(0) == 30).all()
    r = _run([_bin(), tmp_path / "sub.txt", t / "groups.txt", "-n", 99, "--rank-by", "count", "--host"])
    assert r.returncode == 0, r.stderr
    y = Yard(sub["counts"], study["labels"], 99, 1, rank_by="count")
    rows, foot = _parse(r.stdout)
    assert [f[0] for f in rows] == sub["otus"] and foot[0] == "# tested: %d of %d" % (len(y.rows), len(y.tested))
    for i, f in enumerate(rows):
        if y.tested[i]:
            assert [float(v) for v in f[2:6]] == [y.H[i], y.p[i], y.p_maxT[i], y.q[i]]
        else:
            assert f[2:7] == ["NA"] * 5


GOODT = "# HmmUFOtu v1.5.1 OTU table generated by test\notuID\ta\tb\tc\td\ttaxonomy\n1\t1\t2\t3\t4\tx\n2\t4\t0\t2\t1\ty\n"
GOODG = "a\tg1\nb\tg1\nc\tg2\nd\tg2\n"


@pytest.mark.parametrize("tab,grp,args,why", [
    (GOODT, "a\tg1\nb\tg1\nc\tg2\n", [], "Sample 'd' of the table has no line"),
    (GOODT, GOODG + "a\tg2\n", [], "Sample 'a' is named twice"),
    (GOODT, "a g1\n" + GOODG, [], "line 1: expected sample<TAB>group"),
    (GOODT, "a\tg\nb\tg\nc\tg\nd\tg\n", [], "one group"),
    (GOODT, "a\t1\nb\t2\nc\t3\nd\t4\n", [], "every group is a single sample"),
    (GOODT, "a\tg1\nb\tg2\n", ["--ignore-missing"], "2 samples: a test needs 3"),
    (GOODT.replace("\t4\tx", "\t-4\tx"), GOODG, [], "OTU '1' has a negative or non-finite cell in sample 'd'"),
    (GOODT.replace("1\t2\t3\t4", "0\t2\t3\t4").replace("4\t0\t2\t1", "0\t0\t2\t1"), GOODG, [], "Sample 'a' has no reads"),
    (GOODT.replace("1\t2\t3\t4", "5\t5\t5\t5").replace("4\t0\t2\t1", "0\t0\t0\t0"), GOODG, ["--rank-by", "count"], "no OTU is left to test"),
    (GOODT, GOODG, ["--min-prevalence", "5"], "no OTU is left to test"),
    (GOODT, GOODG, ["-n", "0"], "--perms must lie between"),
    (GOODT, GOODG, ["--chunk", "0"], "--chunk must be at least 1"),
    (GOODT, GOODG, ["--rank-by", "clr"], "--rank-by must be"),
    (GOODT, GOODG, ["--mem", "-1"], "--mem must be"),
])
def test_what_the_program_refuses(tmp_path, tab, grp, args, why):
    """every refusal comes before a device is asked for (no --host here), names its reason and leaves no file"""
    (tmp_path / "t.txt").write_text(tab); (tmp_path / "g.txt").write_text(grp)
    r = _run([_bin(), tmp_path / "t.txt", tmp_path / "g.txt", "-o", tmp_path / "o.txt", "--perm-out", tmp_path / "p.txt"] + args)
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert "device" not in r.stderr and r.stdout == ""
    assert not (tmp_path / "o.txt").exists() and not (tmp_path / "p.txt").exists()


def test_program_usage_and_missing_files(tmp_path):
    assert "Usage" in _run([_bin()]).stderr and _run([_bin(), "-h"]).returncode == 0
    (tmp_path / "t.txt").write_text(GOODT)
    r = _run([_bin(), tmp_path / "t.txt", tmp_path / "none.txt", "--host"])
    assert r.returncode != 0 and "Unable to open group file" in r.stderr
    r = _run([_bin(), tmp_path / "none.txt", tmp_path / "none.txt", "--host"])
    assert r.returncode != 0 and r.stderr.strip()
    assert _run([_bin(), tmp_path / "t.txt", "--host"]).returncode != 0 and _run([_bin(), tmp_path / "t.txt", "g", "--frobnicate"]).returncode != 0


def test_program_memory_refusal_names_both_numbers(tmp_path):
    (tmp_path / "t.txt").write_text(GOODT); (tmp_path / "g.txt").write_text(GOODG)
    r = _run([_bin(), tmp_path / "t.txt", tmp_path / "g.txt", "--mem", "0.0005", "-o", tmp_path / "o.txt"])
    assert r.returncode != 0 and len(r.stderr.strip().split("\n")) == 1
    assert "need %d bytes" % E.diffabund_need(4, 2, 2, 7, 1) in r.stderr and ", 536870 bytes are free" in r.stderr and "device" not in r.stderr
    assert not (tmp_path / "o.txt").exists()


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_diffabund_host.cpp (the checks, the totals, the ranking, L, the cells, the host path, maxT and BH; no HIP headers) with
    tests/san/diffabund_driver.cpp under AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "diffabund_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "diffabund_driver.cpp"), os.path.join(CSRC, "hu_diffabund_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "24 cases" in r.stdout


# ---- the device ----

def _device(y, what, chunks=(0,)):
    """the device against the restatement and, byte for byte, against the host path; every chunk gives the same bytes"""
    host = call(y)
    hold(host, y, what + " host")
    for chunk in chunks:
        dev = call(y, host=False, chunk=chunk)
        assert [int(v) for v in dev["rec"]["count_ge"][y.rows]] == [y.count_ge[i] for i in y.rows], "%s chunk %d: count_ge" % (what, chunk)
        assert same_bytes(dev, host), "%s chunk %d: device and host differ" % (what, chunk)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("n,a", [(3, 2), (4, 3), (63, 2), (64, 3), (65, 64), (257, 2), (257, 3), (257, 64)])
def test_device_sample_sizes(cases, n, a):
    """two groups (the register instance), three and sixty-four (the LDS instance); below, at and above a wave of samples"""
    _need_gpu()
    _device(cases(9, n, a, 257), "n %d a %d" % (n, a))


@pytest.mark.gpu
@pytest.mark.parametrize("n_otu", [1, BLOCK - 1, BLOCK, BLOCK + 1])
@pytest.mark.parametrize("a", [2, 3])
def test_device_otu_counts(n_otu, a):
    """one tested OTU, and one below, at and above the OTUs of a workgroup: every row is tested (no special rows)"""
    _need_gpu()
    y = Yard(table(n_otu, 65, 12, special=False), groups(65, a, 2), 257, 3, rank_by="count")      # one OTU alone has the fraction 1 everywhere
    assert len(y.rows) == n_otu
    _device(y, "OTUs %d a %d" % (n_otu, a))


@pytest.mark.gpu
@pytest.mark.parametrize("a", [2, 3])
def test_device_rows_around_the_staging_size(a):
    """rows with one cell below, exactly and one cell above the cells staged in LDS at a time, and one of two pieces and a part"""
    _need_gpu()
    n = 2 * STAGE + 100
    rng = np.random.default_rng(6)
    c = np.zeros((5, n))
    for i, k in enumerate((STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 9)):
        c[i, rng.permutation(n)[:k]] = rng.integers(1, 50, k)
    c[4] = 1
    y = Yard(c, groups(n, a, 4), 60, 2, rank_by="count")
    assert y.tested == [True] * 4 + [False] and y.prevalence.tolist()[:4] == [STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 9]
    _device(y, "staging a %d" % a)


@pytest.mark.gpu
@pytest.mark.parametrize("perms", [1, 255, 256, 257, 999])
def test_device_permutation_counts_and_chunks(cases, perms):
    """the 256-permutation workgroup's edge, and chunks of one, of a workgroup, of a workgroup and a part, and the default"""
    _need_gpu()
    _device(cases(9, 65, 3, perms), "P %d" % perms, chunks=(256, 300, 0) + ((1,) if perms <= 257 else ()))


@pytest.mark.gpu
def test_device_is_deterministic(cases):
    _need_gpu()
    y = cases(9, 65, 3, 257)
    x = call(y, host=False, chunk=100); z = call(y, host=False, chunk=100)
    assert same_bytes(x, z)
    t = E.diffabund_timing()
    assert t["to_device"] > 0 and t["shuffle"] > 0 and t["sums"] > 0 and t["finish"] > 0


@pytest.mark.gpu
def test_device_ties(cases):
    _need_gpu()
    for n, a in ((3, 2), (4, 2)):
        _device(cases(9, n, a, 99), "ties n %d" % n)
    g = [0, 0, 0, 1, 1, 1, 2, 2, 2]
    c = np.zeros((3, 9)); c[0, 1] = 4; c[0, 5] = 9; c[1] = [3, 1, 4, 1, 5, 9, 2, 6, 5]; c[2] = 1
    _device(Yard(c, g, 299, 4), "swaps")
    primes = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47]
    _device(Yard(table(6, 328, 2, special=False), [k for k, s in enumerate(primes) for _ in range(s)], 9, 1), "large L")


@pytest.mark.gpu
def test_program_on_the_device(study):
    _need_gpu()
    t = study["dir"]
    args = [_bin(), t / "table.txt", t / "groups.txt", "-n", 299, "-S", 7]
    r = _run(args + ["-o", t / "dev.txt", "--perm-out", t / "dev_perm.txt", "-v"])
    assert r.returncode == 0, r.stderr
    assert "sums" in r.stderr
    h = _run(args + ["-o", t / "host2.txt", "--perm-out", t / "host2_perm.txt", "--host"])
    assert h.returncode == 0, h.stderr
    assert (t / "dev.txt").read_bytes() == (t / "host2.txt").read_bytes()
    assert (t / "dev_perm.txt").read_bytes() == (t / "host2_perm.txt").read_bytes()
    c = _run(args + ["--chunk", 100])
    assert c.returncode == 0 and c.stdout == (t / "dev.txt").read_text()


@pytest.mark.gpu
def test_device_memory_refusal_and_a_budget_that_shrinks_the_chunk(cases):
    _need_gpu()
    y = cases(9, 65, 3, 999)
    m = len(y.rows); cells = int(sum((values(y.counts, "fraction")[i] > 0).sum() for i in y.rows))
    budget = E.diffabund_need(65, 3, m, cells, 256) + 1000                         # room for one workgroup of permutations
    with pytest.raises(E.EngineError, match=r"chunk of 999 permutations need %d bytes .*, %d bytes are free" % (E.diffabund_need(65, 3, m, cells, 999), budget)) as ei:
        call(y, host=False, mem_budget=budget, chunk=999)
    assert "error -4" in str(ei.value)
    assert same_bytes(call(y, host=False, mem_budget=budget), call(y))              # chunk 0: the largest that fits, 256 here
    with pytest.raises(E.EngineError, match=r", 1048576 bytes are free"):
        call(y, host=False, mem_budget=1 << 20)
