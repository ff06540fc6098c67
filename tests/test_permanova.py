"""hmmufotu-amd-permanova: PERMANOVA of sample groups on a distance matrix, hu_permanova on the host and on the device,
and the program.

The yardstick is a restatement that shares no code with the library: Philox4x32-10 and the Fisher-Yates shuffle in plain Python
integers (checked against hu_sim_philox on a few counters), every D2 as the exact square of its double (an integer over a common power
of two), and SS_T and SS_W of the observed labelling and of every permutation as fractions.Fraction.

The bound (derived there): every D2 is one rounded product, every 1 / n_g one rounded division, all terms are
non-negative, a fixed-order sum of m <= n (n-1) / 2 of them adds at most (m - 1) u relatively and the fma no rounding of its own, so
|SS_W got - exact| <= (n (n-1) / 2 + 8) x 2^-52 x exact, and the same for SS_T.  F and R2 are held to the interval that follows from
the two by interval arithmetic, widened by 2^-50 relatively for their own subtraction and divisions.

The condition on the fixtures, asserted from the restatement before anything is compared: every permutation either induces the
observed partition (then the library's SS_W must equal the observed one bit for bit) or has an exact SS_W further than twice the bound
from the observed one.  Under it count_le and p are compared exactly."""
import functools
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
HEADER = "test\tn\tgroups\tperms\tSS_total\tSS_within\tSS_among\tF\tR2\tp"
M32 = 0xffffffff


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


def shuffled(labels, seed, p):
    g = list(labels)
    for i in range(len(g) - 1, 0, -1):
        w = philox((i & M32, i >> 32, p & M32, p >> 32), (seed & M32, (seed >> 32) & M32))
        j = ((((w[1] << 32) | w[0]) * (i + 1)) >> 64)
        g[i], g[j] = g[j], g[i]
    return g


def partition(g):
    first = {}
    return tuple(first.setdefault(x, len(first)) for x in g)


class Yard:
    """the exact sums of a matrix: D2 as integers over 4^k, k the largest binary exponent of a denominator among the cells"""

    def __init__(self, dist):
        d = np.asarray(dist, np.float64)
        self.n = n = d.shape[0]
        fr = [[Fraction(float(x)) for x in row] for row in d]
        k = max(f.denominator for row in fr for f in row).bit_length() - 1
        self.den = 1 << (2 * k)
        self.D2 = np.array([[int(f * (1 << k)) ** 2 for f in row] for row in fr], dtype=object)
        self.ss_total = Fraction(int(sum(self.D2[i, j] for i in range(n) for j in range(i + 1, n))), self.den * n)
        self.eps = Fraction(n * (n - 1) // 2 + 8, 2 ** 52)

    def ssw(self, g):
        g = np.asarray(g)
        tot = Fraction(0)
        for lab in set(g.tolist()):
            idx = np.nonzero(g == lab)[0]
            if len(idx) > 1:
                full = int(self.D2[np.ix_(idx, idx)].sum())                      # every pair twice: the matrix is symmetric, its diagonal 0
                assert full % 2 == 0
                tot += Fraction(full // 2, self.den * len(idx))
        return tot


class Case:
    def __init__(self, dist, group, perms, seed):
        self.dist = np.ascontiguousarray(dist, np.float64); self.group = [int(x) for x in group]; self.perms = perms; self.seed = seed
        self.n = len(self.group); self.a = len(set(self.group))
        self.yard = y = Yard(self.dist)
        self.obs = y.ssw(self.group)
        part = partition(self.group)
        self.labels = [shuffled(self.group, seed, p) for p in range(perms)]
        self.same = [partition(g) == part for g in self.labels]
        memo = {}
        self.ssw = []
        for g, same in zip(self.labels, self.same):
            key = partition(g)
            if key not in memo:
                memo[key] = self.obs if same else y.ssw(g)
            self.ssw.append(memo[key])
        # the condition on the fixture
        for p, (w, same) in enumerate(zip(self.ssw, self.same)):
            assert same or abs(w - self.obs) > 2 * y.eps * max(w, self.obs), "permutation %d lies within twice the bound of the observed SS_W" % p
        self.count_le = sum(1 for w in self.ssw if w <= self.obs)


def points(n, seed, dims=3, clusters=None):
    """the distances of n random points; clusters: a label per point, whose centre lies 100 away per unit of label"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dims))
    if clusters is not None:
        x[:, 0] += 100.0 * np.asarray(clusters)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = float(np.sqrt(((x[i] - x[j]) ** 2).sum()))
    return d


def groups(n, a, seed):
    """labels 0 .. a-1, dense, every group used, unbalanced: a label is drawn in proportion to its number plus one"""
    rng = np.random.default_rng(seed + 1000)
    g = list(range(a)) + rng.choice(a, n - a, p=np.arange(1, a + 1) / (a * (a + 1) / 2)).tolist()
    return [int(x) for x in rng.permutation(g)]


@functools.lru_cache(maxsize=None)
def case(n, a, perms, seed=5, dseed=11):
    return Case(points(n, dseed), groups(n, a, dseed), perms, seed)


def _iv_div(a, b):
    (alo, ahi), (blo, bhi) = a, b
    assert blo > 0
    return (alo / bhi if alo >= 0 else alo / blo, ahi / blo if ahi >= 0 else ahi / bhi)


def _widen(iv):
    w = Fraction(1, 2 ** 50)
    return (iv[0] - abs(iv[0]) * w, iv[1] + abs(iv[1]) * w)


def hold(res, c, what=""):
    """a result of the library against the restatement of its case"""
    y = c.yard; e = y.eps
    assert (res["n"], res["a"], res["perms"]) == (c.n, c.a, c.perms), what
    T = Fraction(res["ss_total"]); W = Fraction(res["ss_within"])
    assert abs(T - y.ss_total) <= e * y.ss_total, (what, "SS_T", float(abs(T - y.ss_total) / y.ss_total))
    assert abs(W - c.obs) <= e * c.obs, (what, "SS_W", float(W), float(c.obs))
    ssw = res["ssw_perm"]
    assert len(ssw) == c.perms
    for p in range(c.perms):
        got = Fraction(float(ssw[p]))
        if c.same[p]:
            assert float(ssw[p]).hex() == float(res["ss_within"]).hex(), (what, "permutation %d keeps the partition and not the bits" % p)
        assert abs(got - c.ssw[p]) <= e * c.ssw[p], (what, "SS_W of permutation %d" % p, float(got), float(c.ssw[p]))
    assert res["count_le"] == c.count_le, what
    assert res["p"] == (1 + c.count_le) / (c.perms + 1), what
    assert res["ss_among"] == res["ss_total"] - res["ss_within"]
    tiv = (y.ss_total * (1 - e), y.ss_total * (1 + e)); wiv = (c.obs * (1 - e), c.obs * (1 + e))
    aiv = _widen((tiv[0] - wiv[1], tiv[1] - wiv[0]))
    r2 = _widen(_iv_div(aiv, tiv))
    assert r2[0] <= Fraction(res["R2"]) <= r2[1], (what, "R2")
    if c.obs > 0:
        f = _widen(_iv_div((aiv[0] / (c.a - 1), aiv[1] / (c.a - 1)), (wiv[0] / (c.n - c.a), wiv[1] / (c.n - c.a))))
        assert f[0] <= Fraction(res["F"]) <= f[1], (what, "F")
    else:
        assert res["F"] == float("inf"), what


def call(c, **kw):
    return E.permanova(c.dist, c.group, perms=c.perms, seed=c.seed, **kw)


def same_bits(x, y):
    return all(np.float64(x[k]).tobytes() == np.float64(y[k]).tobytes() for k in ("ss_total", "ss_within", "ss_among", "F", "R2", "p")) and \
        x["count_le"] == y["count_le"] and x["ssw_perm"].tobytes() == y["ssw_perm"].tobytes()


# ---- the restatement against known answers ----

def test_the_restated_philox_is_the_librarys():
    assert philox((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]      # Random123's known answers
    assert philox((M32, M32, M32, M32), (M32, M32)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((1, 2, 3, 4), (5, 6)), ((64, 0, 998, 0), (1, 0)), ((M32, 1, M32, 7), (0x9abcdef0, 0x12345678))):
        assert E.sim_philox(ctr, key).tolist() == philox(ctr, key)


def test_labels_are_the_restated_shuffle():
    for n, a, seed in ((3, 2, 1), (7, 3, 2), (65, 5, (1 << 63) + 12345), (300, 64, 99)):
        g = groups(n, a, 3)
        got = E.permanova_labels(g, seed=seed, first=0, count=12)
        assert got.tolist() == [shuffled(g, seed, p) for p in range(12)]
        assert all(sorted(row) == sorted(g) for row in got.tolist())
        later = E.permanova_labels(g, seed=seed, first=7, count=5)
        assert later.tolist() == got[7:12].tolist()                                # first > 0; a longer run's first are a shorter run's
        assert E.permanova_labels(g, seed=seed, first=0, count=3).tolist() == got[:3].tolist()
    big = E.permanova_labels([0, 1, 1, 0], seed=4, first=(1 << 33) + 1, count=1)       # the high word of p is in the counter
    assert big.tolist() == [shuffled([0, 1, 1, 0], 4, (1 << 33) + 1)]


def test_six_samples_by_hand():
    """groups {0,1} and {2,3,4,5}; d = 2 within the first, 1 within the second, 4 across: the squares add to 4 + 6 + 128 = 138, so
    SS_T = 138 / 6 = 23, SS_W = 4 / 2 + 6 / 4 = 3.5, SS_A = 19.5, F = 19.5 / (3.5 / 4) = 156 / 7, R2 = 19.5 / 23"""
    g = [0, 0, 1, 1, 1, 1]
    d = np.array([[0.0 if i == j else (2.0 if g[i] == g[j] == 0 else 1.0 if g[i] == g[j] else 4.0) for j in range(6)] for i in range(6)])
    r = E.permanova(d, g, perms=99, host=True)
    assert (r["ss_total"], r["ss_within"], r["ss_among"]) == (23.0, 3.5, 19.5)
    assert r["F"] == 156 / 7 and r["R2"] == 19.5 / 23
    assert (r["n"], r["a"], r["perms"]) == (6, 2, 99)
    hold(r, Case(d, g, 99, 1))


# ---- the host path ----

@pytest.mark.parametrize("n,a", [(3, 2), (4, 2), (4, 3), (7, 2), (7, 3), (7, 6), (65, 2), (65, 3), (65, 64)])
@pytest.mark.parametrize("perms", [1, 99])
def test_host_against_the_restatement(n, a, perms):
    c = case(n, a, perms)
    hold(call(c, host=True), c, "n %d a %d P %d" % (n, a, perms))


def test_host_999_permutations_and_the_chunk():
    c = case(7, 3, 999)
    r = call(c, host=True)
    hold(r, c)
    for chunk in (1, 7):
        assert same_bits(r, call(c, host=True, chunk=chunk))
    assert same_bits(r, E.permanova(c.dist, c.group, perms=999, seed=c.seed, device=-1))          # device < 0 is the host path too


def test_ties_decide_p_at_three_and_four_samples():
    """at n = 3 a third, at n = 4 with two pairs a third of the permutations repeat the observed partition: p comes from exact ties"""
    for n, g in ((3, [0, 0, 1]), (4, [0, 1, 0, 1]), (4, [0, 0, 0, 1])):
        c = Case(points(n, 21), g, 99, 3)
        assert 10 < sum(c.same) < 70
        r = call(c, host=True)
        hold(r, c)
        assert r["count_le"] >= sum(c.same)


def test_a_group_of_one_and_unbalanced_groups():
    for g in ([0] * 6 + [1], [0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2], [2, 0, 0, 1, 0, 0]):
        g = [int(x) for x in partition(g)]
        c = Case(points(len(g), 8), g, 99, 17)
        hold(call(c, host=True), c)


def test_separated_clusters_and_random_labels():
    """labels that follow two well-separated clusters: SS_W(p) <= the observed one only where the partition is the observed one, so p is
    1 / (P + 1) only when the restatement finds no such permutation; labels at random on the same matrix give a larger p and a smaller F"""
    cl = [0, 0, 0, 0, 1, 1, 1, 1]
    d = points(8, 31, clusters=cl)
    block = Case(d, cl, 99, 2)
    r = call(block, host=True)
    hold(r, block)
    assert r["count_le"] == sum(block.same) and r["p"] == (1 + sum(block.same)) / 100
    few = Case(d, cl, 1, 2)
    assert call(few, host=True)["p"] == (1.0 if few.same[0] else 0.5)
    rand = Case(d, [0, 1, 0, 1, 1, 0, 1, 0], 99, 2)
    q = call(rand, host=True)
    hold(q, rand)
    assert q["p"] > r["p"] and q["F"] < r["F"] and q["R2"] < r["R2"]


def test_no_variation_within_gives_inf():
    d = np.array([[0.0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]])
    c = Case(d, [0, 0, 1, 1], 99, 1)
    assert c.obs == 0
    r = call(c, host=True)
    hold(r, c)
    assert r["ss_within"] == 0.0 and r["F"] == float("inf") and r["R2"] == 1.0 and r["count_le"] == sum(c.same)


def test_need_is_the_documented_function():
    for n, a, chunk in ((3, 2, 1), (65, 3, 256), (129, 64, 257), (16384, 8, 9999)):
        c = -(-chunk // 256) * 256; nt = -(-n // 64)
        assert E.permanova_need(n, a, chunk) == 8 * n * n + 2 * n * c + 8 * (nt * (nt + 1) // 2) * c + 8 * c + 8 * a + 2 * n + (1 << 20)
    assert E.permanova_need(0, 2, 1) == -1


def test_what_the_library_refuses():
    d = points(5, 1); g = [0, 1, 0, 1, 1]

    def bad(why, dist=d, group=g, **kw):
        with pytest.raises(E.EngineError, match=why) as ei:
            E.permanova(dist, group, **kw)
        assert "error -1" in str(ei.value) and "device" not in str(ei.value)
    bad("3 at the least", dist=d[:2, :2], group=[0, 1])
    bad("negative label", group=[0, -1, 0, 1, 1])
    bad("not dense", group=[0, 2, 0, 2, 2])
    bad("not dense", group=[0, 7, 0, 1, 1])
    bad("one group", group=[0] * 5)
    bad("every group is a single sample", group=[0, 1, 2, 3, 4])
    bad("permutations", perms=0)
    bad("permutations", perms=10 ** 7 + 1)
    bad("chunk", chunk=-1)
    for v in (-1.0, np.nan, np.inf):
        x = d.copy(); x[1, 3] = x[3, 1] = v
        bad("samples 1 and 3 is negative or not finite", dist=x)
    x = d.copy(); x[1, 3] = x[3, 1] = 1e200
    bad("samples 1 and 3 is 1e\\+200: its square is not finite", dist=x)
    x = d.copy(); x[3, 1] += 0.5
    bad(r"not symmetric: d\(1, 3\) = .*, d\(3, 1\) = ", dist=x)
    x = d.copy(); x[2, 2] = 1e-9
    bad("sample 2 is at the distance", dist=x)
    bad("every distance is 0", dist=np.zeros((5, 5)))
    with pytest.raises(E.EngineError, match="dist"):
        E.permanova(d, [0, 1])


def test_too_many_groups_are_refused(tmp_path):
    """65,536 groups need 65,538 samples: the labels are refused before a cell is read, so the matrix is a sparse file that is never touched"""
    n = 65538
    d = np.memmap(tmp_path / "sparse.bin", dtype=np.float64, mode="w+", shape=(n, n))
    g = np.arange(n, dtype=np.int32); g[-1] = 0; g[-2] = 1
    with pytest.raises(E.EngineError, match="65536 groups: 65535 at the most") as ei:
        E.permanova(d, g, perms=1)
    assert "device" not in str(ei.value)


def test_memory_refusal_names_both_numbers():
    c = case(65, 3, 99)
    with pytest.raises(E.EngineError, match=r"need (\d+) bytes of device memory .*, 1048576 bytes are free") as ei:
        call(c, mem_budget=1 << 20)
    assert "error -4" in str(ei.value)
    assert int(str(ei.value).split("need ")[1].split(" ")[0]) == E.permanova_need(65, 3, 1)
    with pytest.raises(E.EngineError, match=r"chunk of 99 permutations need %d bytes" % E.permanova_need(65, 3, 99)):
        call(c, mem_budget=1 << 20, chunk=300)                                  # a chunk is never more than the permutations


def test_the_reader(tmp_path):
    d = points(4, 2)
    r = E.dist_matrix_read(_write_matrix(tmp_path / "d.txt", ["a", "b c", "d", "e"], d))
    assert r["samples"] == ["a", "b c", "d", "e"] and r["dist"].tobytes() == d.tobytes()
    with pytest.raises(E.EngineError, match="error -3: Unable to open distance matrix"):
        E.dist_matrix_read(tmp_path / "none.txt")


# ---- the program ----

def _write_matrix(path, names, d):
    with open(path, "w") as f:
        f.write("".join("\t" + s for s in names) + "\n")
        for i, s in enumerate(names):
            f.write(s + "".join("\t%.17g" % v for v in d[i]) + "\n")
    return path


def _write_groups(path, names, labels, extra=""):
    with open(path, "w") as f:
        f.write("# sample\tgroup\n\n" + extra)
        for s, g in zip(names, labels):
            f.write("%s\t%s\n" % (s, g))
    return path


def _parse(text):
    lines = text.rstrip("\n").split("\n")
    assert lines[0] == HEADER
    return [ln.split("\t") for ln in lines[1:]]


def _fmt(r):
    return [str(r["n"]), str(r["a"]), str(r["perms"])] + ["%.17g" % r[k] for k in ("ss_total", "ss_within", "ss_among", "F", "R2", "p")]


STUDY_GROUPS = ["gut", "skin", "gut", "oral", "skin", "gut", "soil", "skin", "gut", "oral", "air", "gut"]        # soil and air: groups of one


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    d = tmp_path_factory.mktemp("permanova")
    names = ["s %d" % i for i in range(len(STUDY_GROUPS))]
    dist = points(len(names), 41)
    _write_matrix(d / "dist.txt", names, dist)
    _write_groups(d / "groups.txt", names[::-1], STUDY_GROUPS[::-1], extra="elsewhere\tgut\nnowhere\tsea\n")
    return dict(dir=d, names=names, dist=dist, labels=list(partition(STUDY_GROUPS)))


def _pairwise_lines(study, perms, seed, **kw):
    """the lines of --pairwise from separate library calls on the sub-matrices"""
    order = list(dict.fromkeys(STUDY_GROUPS)); out = []
    for x in range(len(order)):
        for y in range(x + 1, len(order)):
            idx = [i for i, g in enumerate(STUDY_GROUPS) if g in (order[x], order[y])]
            sizes = [sum(1 for i in idx if STUDY_GROUPS[i] == o) for o in (order[x], order[y])]
            name = order[x] + ":" + order[y]
            if len(idx) < 3 or max(sizes) < 2:
                out.append([name, str(len(idx)), "2", str(perms)] + ["NA"] * 6)
                continue
            sub = study["dist"][np.ix_(idx, idx)]
            out.append([name] + _fmt(E.permanova(sub, list(partition([STUDY_GROUPS[i] for i in idx])), perms=perms, seed=seed, **kw)))
    return out


def test_program_on_the_host(study):
    t = study["dir"]
    r = _run([_bin(), t / "dist.txt", t / "groups.txt", "--host", "-n", 99, "-S", 7, "--pairwise", "--perm-out", t / "perm.txt", "-v"])
    assert r.returncode == 0, r.stderr
    assert "2 line(s)" in r.stderr and "name no sample of the matrix" in r.stderr and "1 pair(s) of groups too small to test" in r.stderr
    rows = _parse(r.stdout)
    lib = E.permanova(study["dist"], study["labels"], perms=99, seed=7, host=True)
    hold(lib, Case(study["dist"], study["labels"], 99, 7))
    assert rows[0] == ["all"] + _fmt(lib)
    want = _pairwise_lines(study, 99, 7, host=True)
    assert rows[1:] == want and len(want) == 10
    assert [w for w in want if w[4] == "NA"] == [["soil:air", "2", "2", "99"] + ["NA"] * 6]          # oral:soil has three samples and is tested
    perm = (t / "perm.txt").read_text().rstrip("\n").split("\n")
    assert perm[0] == "perm\tSS_within\tF" and len(perm) == 100
    for p, ln in enumerate(perm[1:]):
        f = ln.split("\t")
        w = float(lib["ssw_perm"][p])
        assert f[0] == str(p) and f[1] == "%.17g" % w
        assert f[2] == "%.17g" % (((lib["ss_total"] - w) / (lib["a"] - 1)) / (w / (lib["n"] - lib["a"])))
    # -o writes what stdout got; the defaults are 999 permutations under seed 1
    o = _run([_bin(), t / "dist.txt", t / "groups.txt", "--host", "-o", t / "out.txt"])
    assert o.returncode == 0 and o.stdout == "" and o.stderr == ""
    assert _parse((t / "out.txt").read_text()) == [["all"] + _fmt(E.permanova(study["dist"], study["labels"], host=True))]


def test_program_prints_inf(tmp_path):
    d = np.array([[0.0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]])
    _write_matrix(tmp_path / "d.txt", list("abcd"), d); _write_groups(tmp_path / "g.txt", list("abcd"), ["x", "x", "y", "y"])
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "g.txt", "--host", "--perms", 9])
    assert r.returncode == 0, r.stderr
    row = _parse(r.stdout)[0]
    assert row[5] == "0" and row[7] == "inf" and row[8] == "1"


def test_program_reads_what_unifrac_writes(tmp_path):
    rng = np.random.default_rng(4)
    counts = rng.integers(0, 40, (9, 7)); counts[0] += 1
    names = ["site %d" % j for j in range(7)]
    with open(tmp_path / "t.txt", "w") as f:
        f.write("# HmmUFOtu v1.5.1 OTU table generated by test\notuID\t" + "\t".join(names) + "\ttaxonomy\n")
        for i, row in enumerate(counts):
            f.write("%d\t%s\t\n" % (i, "\t".join(str(v) for v in row)))
    u = _run([_bin("hmmufotu-amd-unifrac"), tmp_path / "t.txt", "--method", "bray-curtis", "--host", "-o", tmp_path / "d.txt"])
    assert u.returncode == 0, u.stderr
    m = E.dist_matrix_read(tmp_path / "d.txt")
    assert m["samples"] == names
    assert m["dist"].tobytes() == E.unifrac(counts.astype(float), method="bray-curtis", host=True).tobytes()
    g = [0, 1, 0, 1, 2, 2, 0]
    _write_groups(tmp_path / "g.txt", names, ["g%d" % x for x in g])
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "g.txt", "--host", "-n", 99])
    assert r.returncode == 0, r.stderr
    c = Case(m["dist"], g, 99, 1)
    lib = call(c, host=True)
    hold(lib, c)
    assert _parse(r.stdout) == [["all"] + _fmt(lib)]


GOOD = "\ta\tb\tc\td\na\t0\t1\t2\t3\nb\t1\t0\t1.5\t2\nc\t2\t1.5\t0\t1\nd\t3\t2\t1\t0\n"
GOODG = "a\tx\nb\tx\nc\ty\nd\ty\n"


@pytest.mark.parametrize("dist,grp,args,why", [
    (GOOD, "a\tx\nb\tx\nc\ty\n", [], "Sample 'd' of the matrix has no line in"),
    (GOOD, GOODG + "b\ty\n", [], "Sample 'b' is named twice in"),
    (GOOD, "a\tx\nb\nc\ty\nd\ty\n", [], "line 2: expected sample<TAB>group"),
    (GOOD, GOODG, ["-n", "0"], "--perms must lie between 1 and 10000000"),
    (GOOD, GOODG, ["--perms", "10000001"], "--perms must lie between 1 and 10000000"),
    (GOOD, GOODG, ["--chunk", "0"], "--chunk must be at least 1"),
    (GOOD, GOODG, ["--mem", "-1"], "--mem must be a positive number of GB"),
    (GOOD, GOODG, ["--bogus"], "unknown option --bogus"),
    (GOOD, "a\tx\nb\tx\nc\tx\nd\tx\n", [], "one group"),
    (GOOD, "a\tw\nb\tx\nc\ty\nd\tz\n", [], "every group is a single sample"),
    (GOOD.replace("\t3\n", "\t4\n", 1), GOODG, [], "not symmetric: d(0, 3) = 4, d(3, 0) = 3"),
    (GOOD.replace("1.5", "-1.5"), GOODG, [], "samples 1 and 2 is negative or not finite"),
    (GOOD.replace("1.5", "nan"), GOODG, [], "samples 1 and 2 is negative or not finite"),
    (GOOD.replace("c\t2\t1.5\t0", "c\t2\t1.5\t0.25"), GOODG, [], "sample 2 is at the distance 0.25 from itself"),
    (GOOD.replace("1.5", "x"), GOODG, [], "line 3: 'x' is not a number"),
    (GOOD.replace("\nd\t3\t2\t1\t0", ""), GOODG, [], "3 rows for 4 samples"),
    (GOOD.replace("\nc\t", "\nq\t"), GOODG, [], "line 4: row 'q' where the header has 'c'"),
    ("\ta\tb\na\t0\t1\nb\t1\t0\n", "a\tx\nb\ty\n", [], "2 samples: a test needs 3 at the least"),
    ("\ta\tb\tc\na\t0\t0\t0\nb\t0\t0\t0\nc\t0\t0\t0\n", "a\tx\nb\ty\nc\ty\n", [], "every distance is 0"),
])
def test_what_the_program_refuses(tmp_path, dist, grp, args, why):
    (tmp_path / "d.txt").write_text(dist); (tmp_path / "g.txt").write_text(grp)
    out = tmp_path / "o.txt"; perm = tmp_path / "p.txt"
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "g.txt", "-o", out, "--perm-out", perm, "--pairwise"] + args)    # no --host: refused before a device
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert len(r.stderr.strip().split("\n")) == 1
    assert "device" not in r.stderr
    assert not out.exists() and not perm.exists()


def test_program_usage_and_missing_files(tmp_path):
    (tmp_path / "d.txt").write_text(GOOD)
    r = _run([_bin(), tmp_path / "d.txt"])
    assert r.returncode != 0 and "Usage:" in r.stderr
    assert _run([_bin()]).returncode == 0 and _run([_bin(), "--help"]).returncode == 0
    v = _run([_bin(), "--version"])
    assert v.returncode == 0 and "v1.5.1" in v.stderr
    r = _run([_bin(), tmp_path / "none.txt", tmp_path / "g.txt", "--host"])
    assert r.returncode != 0 and "Unable to open distance matrix" in r.stderr
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "g.txt", "--host"])
    assert r.returncode != 0 and "Unable to open group file" in r.stderr


def test_program_memory_refusal_names_both_numbers(tmp_path):
    (tmp_path / "d.txt").write_text(GOOD); (tmp_path / "g.txt").write_text(GOODG)
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "g.txt", "--mem", "0.0005", "-o", tmp_path / "o.txt"])
    assert r.returncode != 0 and len(r.stderr.strip().split("\n")) == 1
    assert "need %d bytes of device memory" % E.permanova_need(4, 2, 1) in r.stderr and ", 536870 bytes are free" in r.stderr
    assert not (tmp_path / "o.txt").exists()


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_permanova_host.cpp (the checks, the plan, the shuffle, the host path and the matrix reader; no HIP headers) with
    tests/san/permanova_driver.cpp under AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "permanova_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "permanova_driver.cpp"), os.path.join(CSRC, "hu_permanova_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path / "matrix.txt")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "40 cases" in r.stdout


# ---- the device ----

def _device(c, what, chunks=(0,)):
    """the device against the restatement and, bit for bit, against the host path; every chunk gives the same bits"""
    host = call(c, host=True)
    for chunk in chunks:
        dev = call(c, chunk=chunk)
        hold(dev, c, "%s chunk %d" % (what, chunk))
        assert same_bits(dev, host), "%s chunk %d: device and host differ" % (what, chunk)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("n,a", [(3, 2), (4, 3), (63, 2), (64, 3), (65, 64), (129, 2), (129, 3), (129, 64), (280, 256), (280, 257)])
def test_device_sample_sizes(n, a):
    """one tile, the tile's edge, an off-diagonal tile with a ragged edge, three tiles per side; two, three and sixty-four groups; 256
    groups, the last count whose labels the kernel keeps as bytes, and 257, the first that it keeps as halfwords"""
    _need_gpu()
    _device(case(n, a, 257), "n %d a %d" % (n, a))


@pytest.mark.gpu
@pytest.mark.parametrize("perms", [1, 255, 256, 257, 999])
def test_device_permutation_counts_and_chunks(perms):
    """the 256-permutation workgroup's edge, and chunks of one, of a workgroup, of a workgroup and a part, and the default"""
    _need_gpu()
    c = case(65, 3, perms)
    _device(c, "P %d" % perms, chunks=(256, 300, 0) + ((1,) if perms <= 257 else ()))


@pytest.mark.gpu
def test_device_is_deterministic():
    _need_gpu()
    c = case(129, 3, 257)
    x = call(c, chunk=100); y = call(c, chunk=100)
    assert same_bits(x, y)
    t = E.permanova_timing()
    assert t["to_device"] > 0 and t["shuffle"] > 0 and t["pairs"] > 0 and t["finish"] > 0


@pytest.mark.gpu
def test_device_ties_and_inf():
    _need_gpu()
    c = Case(points(4, 21), [0, 1, 0, 1], 99, 3)
    assert sum(c.same) > 10
    _device(c, "ties")
    d = np.array([[0.0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]])
    r = _device(Case(d, [0, 0, 1, 1], 99, 1), "no variation within")
    assert r["F"] == float("inf")


@pytest.mark.gpu
def test_program_on_the_device(study):
    _need_gpu()
    t = study["dir"]
    args = [_bin(), t / "dist.txt", t / "groups.txt", "-n", 299, "-S", 7, "--pairwise"]
    r = _run(args + ["-o", t / "dev.txt", "--perm-out", t / "dev_perm.txt", "-v"])
    assert r.returncode == 0, r.stderr
    assert "pair kernel" in r.stderr
    h = _run(args + ["-o", t / "host.txt", "--perm-out", t / "host_perm.txt", "--host"])
    assert h.returncode == 0, h.stderr
    assert (t / "dev.txt").read_bytes() == (t / "host.txt").read_bytes()
    assert (t / "dev_perm.txt").read_bytes() == (t / "host_perm.txt").read_bytes()
    rows = _parse((t / "dev.txt").read_text())
    assert rows[1:] == _pairwise_lines(study, 299, 7) and len(rows) == 11
    c = _run(args + ["--chunk", 100])
    assert c.returncode == 0 and c.stdout == (t / "dev.txt").read_text()


@pytest.mark.gpu
def test_device_memory_refusal_and_a_budget_that_shrinks_the_chunk():
    _need_gpu()
    c = case(129, 3, 999)
    budget = E.permanova_need(129, 3, 256) + 1000                                 # room for one workgroup of permutations
    with pytest.raises(E.EngineError, match=r"chunk of 999 permutations need %d bytes of device memory .*, %d bytes are free" % (E.permanova_need(129, 3, 999), budget)) as ei:
        call(c, mem_budget=budget, chunk=999)
    assert "error -4" in str(ei.value)
    assert same_bits(call(c, mem_budget=budget), call(c))                           # chunk 0: the largest that fits, 256 here
    with pytest.raises(E.EngineError, match=r", 1048576 bytes are free"):
        call(c, mem_budget=1 << 20)
