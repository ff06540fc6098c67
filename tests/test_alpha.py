"""hmmufotu-amd-alpha: alpha diversity of the samples of an OTU table and rarefaction curves, hu_alpha on the host and
on the device, and the program.

The yardstick is a restatement of the definitions in include/hmmufotu_amd.h that shares no code with the library: Python integers for
S, F1, F2 and Q; the walk from every OTU with a read to the root (as tests/test_unifrac.py walks) and exact rational sums for PD;
`decimal` at 50 digits for ln, so A and the Shannon index come out to 50 digits.  It is applied to the table's columns, and for the
draw (j, m, r) to column j of engine.otu_subset(counts, m, seed=seed + r, device=-1), which tests/test_otu_tools.py pins.

Bounds.  The integer statistics are exact.  The metrics are the documented double expressions of them, bit for bit.  PD lies within
(B + 8) x 2^-52 x PD of the exact value (DESIGN.md §20 derives it for the same sum; B the kept branches).  shannon: the largest
|H - H_exact| / max(1, ln N) measured over all CPU and GPU cases of this file is 4.54e-16 on the host path (the 64 samples on the unbalanced
tree; 1.85e-16 over the CPU cases) and 2.09e-16 on the device (test_zz_the_shannon_bar_covers_what_was_measured and the device cases
print the figure of a run); four times the larger, 1.82e-15, rounded up to a power of two is SHANNON_BAR = 2^-48 = 3.6e-15.  Host and device each meet it; nothing is claimed about their bits agreeing.  A is held through the
same bar: |A - A_exact| / (N max(1, ln N)), since A enters H as A / N."""
import math
import os
import shutil
import subprocess
import sys
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_shapes  # noqa: E402
from hmmufotu_amd import engine as E, synth  # noqa: E402

getcontext().prec = 50
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")
U = Fraction(1, 2 ** 52)
SHANNON_BAR = 2.0 ** -48
assert SHANNON_BAR <= 1e-12
INTS = ("reads", "S", "F1", "F2", "Q")
WORST = {"host": 0.0, "device": 0.0}


def _bin(name="hmmufotu-amd-alpha"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ---- the yardstick ----

_LN = {}


def ln(n):
    if n not in _LN:
        _LN[n] = Decimal(n).ln()
    return _LN[n]


class Tree:
    """parent [nodes] (-1: the root), blen [nodes]; nodes [rows] the node of every OTU row"""

    def __init__(self, parent, blen, nodes):
        self.parent = np.asarray(parent, np.int32); self.blen = np.asarray(blen, np.float64); self.nodes = np.asarray(nodes, np.int32)
        par = [int(p) for p in self.parent]
        self.path = []                                              # per row: the branches (named by the node below) from it to the root
        kept = set()
        for u in self.nodes:
            v = int(u); p = []
            while par[v] >= 0:
                p.append(v); v = par[v]
            self.path.append(p); kept.update(p)
        self.B = len(kept)
        self.len = {v: Fraction(float(self.blen[v])) for v in kept}

    def pd(self, col):
        """exact: the branches below which the column has a read"""
        seen = set()
        for i, n in enumerate(col):
            if n > 0:
                seen.update(self.path[i])
        return sum((self.len[v] for v in seen), Fraction(0))

    def entries(self, col):
        return len({v for i, n in enumerate(col) if n > 0 for v in self.path[i]})

    def args(self):
        return dict(otu_node=self.nodes, parent=self.parent, blen=self.blen)


def yard(col, tree=None):
    """the statistics and the metrics of one column of integers"""
    col = [int(x) for x in col]
    N = sum(col)
    S = sum(n > 0 for n in col); F1 = sum(n == 1 for n in col); F2 = sum(n == 2 for n in col); Q = sum(n * n for n in col)
    A = sum((n * ln(n) for n in col if n >= 2), Decimal(0))
    H = ln(N) - A / N if S > 1 else Decimal(0)
    out = dict(reads=N, S=S, F1=F1, F2=F2, Q=Q, A=A, H=H, PD=tree.pd(col) if tree is not None else None)
    out.update(observed=float(S), singles=float(F1), doubles=float(F2), chao1=float(S) + float(F1) * float(F1 - 1) / (2.0 * float(F2 + 1)),
               simpson=1.0 - float(Q) / (float(N) * float(N)), goods_coverage=1.0 - float(F1) / float(N))
    return out


def shannon_of(A, N, S):
    """the documented double expression, from the library's own A"""
    return 0.0 if S <= 1 else max(0.0, math.log(float(N)) - float(A) / float(N))


def hold(rec, at, y, tree, path, exact_ints=True):
    """one record of a result (rec: the dict of arrays, at: its index) against the yardstick of its column"""
    N = y["reads"]
    if exact_ints:
        for f in INTS:
            assert int(rec[f][at]) == y[f], (path, at, f, int(rec[f][at]), y[f])
        for f in ("observed", "singles", "doubles", "chao1", "simpson", "goods_coverage"):
            assert float(rec[f][at]).hex() == y[f].hex(), (path, at, f, rec[f][at], y[f])
    scale = max(1.0, math.log(N))
    dev = float(abs(Decimal(float(rec["shannon"][at])) - y["H"])) / scale
    devA = float(abs(Decimal(float(rec["A"][at])) - y["A"])) / (N * scale)
    WORST[path] = max(WORST[path], dev)
    assert dev <= SHANNON_BAR and devA <= SHANNON_BAR, (path, at, "shannon", rec["shannon"][at], float(y["H"]), dev, devA)
    if y["S"] <= 1:
        assert rec["shannon"][at] == 0.0
    if path == "host":                                              # libm's log on both sides: the same expression gives the same bits
        assert float(rec["shannon"][at]).hex() == shannon_of(rec["A"][at], N, y["S"]).hex()
    if tree is None:
        assert math.isnan(rec["PD"][at]) and math.isnan(rec["faith_pd"][at])
    elif y["PD"] is not None:
        assert abs(Fraction(float(rec["PD"][at])) - y["PD"]) <= (tree.B + 8) * U * y["PD"], (path, at, rec["PD"][at], float(y["PD"]))
        assert float(rec["faith_pd"][at]).hex() == float(rec["PD"][at]).hex()


def absent(rec, at):
    assert int(rec["reads"][at]) == 0 and all(int(rec[f][at]) == 0 for f in INTS)
    assert all(math.isnan(rec[f][at]) for f in rec if f not in INTS)


_SUB = {}


def subset(key, counts, m, seed, key_bits):
    """the pinned entry's columns at depth m under one seed, made once per table"""
    k = (key, m, seed & (2 ** 64 - 1), key_bits)
    if k not in _SUB:
        _SUB[k] = E.otu_subset(counts, m, seed=seed, device=-1, key_bits=key_bits)
    return _SUB[k]


def hold_all(res, key, counts, tree, depths, reps, seed, key_bits, path, pd_yard=True):
    """every whole sample and every draw of a result against the yardstick"""
    S = counts.shape[1]
    tot = counts.sum(0)
    for j in range(S):
        hold(res["whole"], j, yard(counts[:, j], tree if pd_yard else None), tree, path)
    for d, m in enumerate(depths):
        for r in range(reps):
            sub = subset(key, counts, m, seed + r, key_bits)
            for j in range(S):
                if m > tot[j]:
                    absent(res["draws"], (j, d, r))
                else:
                    assert sub[:, j].sum() == m
                    hold(res["draws"], (j, d, r), yard(sub[:, j], tree if pd_yard else None), tree, path)


def same(a, b, skip=()):
    for part in ("whole", "draws"):
        for f in a[part]:
            if f not in skip:
                assert a[part][f].tobytes() == b[part][f].tobytes(), (part, f)


# ---- trees and tables ----

def chain(B, seed=3):
    """B + 1 nodes, node v on node v - 1: B branches once a row sits on the last node"""
    rng = np.random.default_rng(seed)
    return np.arange(-1, B, dtype=np.int32), np.r_[0.0, rng.exponential(0.05, B) + 1e-5]


def star(k, seed=4):
    rng = np.random.default_rng(seed)
    return np.r_[-1, np.zeros(k, np.int32)].astype(np.int32), np.r_[0.0, rng.exponential(0.05, k) + 1e-5]


def rows_on(parent, M, seed, root=True):
    """M rows: the last node (the deepest of a chain), the root, then nodes in turn: leaves and inner nodes, two rows on one node when
    the tree is smaller than the table"""
    n = len(parent)
    rng = np.random.default_rng(seed)
    nodes = [n - 1] + ([0] if root and M > 1 else [])
    rest = rng.permutation(np.arange(1, n))
    while len(nodes) < M:
        nodes.append(int(rest[len(nodes) % len(rest)]))
    return np.array(nodes[:M], np.int32)


# (nonzero cells, reads): with chunks of 64 and of 256 reads a sample's reads lie within one chunk (40; 200), fill one exactly (64; 256),
# spill one read into a second (65; 257) and span several (the rest); the cells are the edges of a wave and of the 256-thread strides
SPEC = [(1, 40), (63, 64), (64, 256), (65, 257), (257, 1500), (63, 200), (64, 65), (257, 257), (1, 256), (65, 3000)]


def spec_table(M, S, seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((M, S))
    for j in range(S):
        nnz, N = SPEC[j % len(SPEC)]
        nnz = min(nnz, M)
        rows = rng.choice(M, nnz, replace=False)
        c[rows, j] = 1 + rng.multinomial(N - nnz, rng.dirichlet(np.full(nnz, 0.3)))
        assert c[:, j].sum() == N
    return c


def spec_depths(counts):
    tot = sorted({int(t) for t in counts.sum(0)})
    return sorted({1} | {t - 1 for t in tot if t > 1} | set(tot) | {tot[0] + 1})


def small_case(seed=5, S=3, M=12):
    rng = np.random.default_rng(seed)
    parent, blen, _ = tree_shapes.tree(8, 3, 1, seed)
    tr = Tree(parent, blen, rows_on(parent, M, seed))
    counts = rng.integers(0, 9, (M, S)).astype(np.float64) * (rng.random((M, S)) < 0.6)
    counts[rng.integers(0, M, S), np.arange(S)] += 2
    return tr, counts


# ---- the host path ----

@pytest.mark.parametrize("key_bits, reps", [(64, 3), (64, 1), (4, 3)])
def test_host_whole_samples_and_every_draw(key_bits, reps):
    """depths 1, 2, N_j - 1, N_j of every sample and one beyond the largest; key_bits 4: sixteen keys, so the cut key always ties"""
    tr, counts = small_case()
    tot = [int(t) for t in counts.sum(0)]
    depths = sorted({1, 2} | {t - 1 for t in tot} | set(tot) | {max(tot) + 1})
    res = E.alpha_diversity(counts, depths=depths, reps=reps, seed=11, host=True, key_bits=key_bits, **tr.args())
    assert res["draws"]["S"].shape == (3, len(depths), reps)
    hold_all(res, "small", counts, tr, depths, reps, 11, key_bits, "host")
    for j, t in enumerate(tot):                                     # m = N_j is the whole sample
        for f in res["whole"]:
            assert (res["draws"][f][j, depths.index(t)] == res["whole"][f][j]).all()
    again = E.alpha_diversity(counts, depths=depths, reps=reps, seed=11, device=-1, key_bits=key_bits, chunk=7, draw_chunk=2, **tr.args())
    same(res, again)
    pd = E.unifrac(counts, tr.nodes, tr.parent, tr.blen, method="unweighted", pd=True, host=True)[1]
    for j in range(3):
        e = tr.pd(counts[:, j])
        assert abs(Fraction(float(pd[j])) - Fraction(float(res["whole"]["faith_pd"][j]))) <= 2 * (tr.B + 8) * U * e


def test_host_the_seed_wraps_and_the_tree_is_optional():
    tr, counts = small_case(6)
    seed = 2 ** 64 - 1                                              # repeat 1 draws under the seed 0
    res = E.alpha_diversity(counts, depths=(3,), reps=2, seed=seed, host=True)
    hold_all(res, "small6", counts, None, [3], 2, seed, 64, "host")
    assert math.isnan(res["whole"]["PD"][0])
    with_tree = E.alpha_diversity(counts, depths=(3,), reps=2, seed=seed, host=True, **tr.args())
    for f in INTS + ("chao1", "simpson"):                           # a tree reorders the cells of a draw, not the reads it keeps
        assert (with_tree["draws"][f] == res["draws"][f]).all()


def test_cases_by_hand():
    one = E.alpha_diversity([[7.0]], host=True)["whole"]
    assert one["S"][0] == 1 and one["shannon"][0] == 0.0 and one["simpson"][0] == 0.0 and one["chao1"][0] == 1.0 and one["goods_coverage"][0] == 1.0
    ones = E.alpha_diversity(np.ones((5, 1)), host=True)["whole"]                # all singletons: F1 = S = N
    assert ones["F1"][0] == 5 and ones["F2"][0] == 0 and ones["chao1"][0] == 5 + 5 * 4 / 2.0 and ones["goods_coverage"][0] == 0.0 and ones["A"][0] == 0.0
    assert ones["simpson"][0] == 1.0 - 5.0 / 25.0 and abs(ones["shannon"][0] - math.log(5)) <= SHANNON_BAR * math.log(5)
    big = E.alpha_diversity([[2.0 ** 32 - 1, 3.0], [0.0, 1.0]], host=True)["whole"]   # Q near 2^64
    assert int(big["Q"][0]) == (2 ** 32 - 1) ** 2 and big["simpson"][0] == 0.0 and big["shannon"][0] == 0.0 and int(big["Q"][1]) == 10
    hold(big, 0, yard([2 ** 32 - 1, 0]), None, "host")
    # a five-node tree: 0 the root, 1 and 2 below it, 3 and 4 below 1
    parent = [-1, 0, 0, 1, 1]; blen = [9.0, 1.0, 2.0, 0.5, 0.25]
    root_only = E.alpha_diversity([[4.0], [0.0]], otu_node=[0, 3], parent=parent, blen=blen, host=True)["whole"]
    assert root_only["PD"][0] == 0.0 and root_only["S"][0] == 1                   # the OTU that is the root lies below no branch
    inner = E.alpha_diversity([[2.0, 0.0], [1.0, 1.0], [0.0, 5.0]], otu_node=[1, 3, 2], parent=parent, blen=blen, host=True)["whole"]
    assert inner["PD"][0] == 1.5 and inner["PD"][1] == 3.5                        # an inner node and a leaf below it share the inner branch
    none = E.alpha_diversity([[2.0], [1.0]], host=True)["whole"]
    assert math.isnan(none["faith_pd"][0]) and none["S"][0] == 2


def comb_ratio(N, n, m):
    """C(N - n, m) / C(N, m): the chance that m reads out of N miss all of n"""
    return Fraction(math.comb(N - n, m), math.comb(N, m))


def test_the_draws_have_the_hypergeometric_means():
    """The mean observed OTUs and the mean PD of 200 draws of 150 reads from a planted sample of 1,000 against their exact expectations,
    sum [1 - C(N - n, m) / C(N, m)] over the OTUs and over the branches (n then the reads below the branch), within 4 standard errors of
    the 200 draws.  Seed 1, the program's default, the first tried; it holds on the host path.  A check of the plumbing (that a draw's
    statistics belong to the draw they are filed under, and that the repeats differ), not of the generator: Philox has its own tests,
    and 4 standard errors of 200 draws would not see a subtle bias."""
    rng = np.random.default_rng(2)
    M, N, m, R = 40, 1000, 150, 200
    parent, blen, _ = tree_shapes.tree(24, 2, 0, 2)
    tr = Tree(parent, blen, rows_on(parent, M, 2))
    col = 1 + rng.multinomial(N - M, rng.dirichlet(np.full(M, 0.25)))
    res = E.alpha_diversity(col.reshape(M, 1).astype(float), depths=(m,), reps=R, seed=1, host=True, **tr.args())["draws"]
    below = {}
    for i, n in enumerate(col):
        for v in tr.path[i]:
            below[v] = below.get(v, 0) + int(n)
    e_obs = float(sum(1 - comb_ratio(N, int(n), m) for n in col))
    e_pd = float(sum(tr.len[v] * (1 - comb_ratio(N, n, m)) for v, n in below.items()))
    for f, e in (("observed", e_obs), ("faith_pd", e_pd)):
        x = res[f][0, 0]
        se = x.std(ddof=1) / math.sqrt(R)
        print("%s: mean %.6g, expected %.6g, standard error %.3g" % (f, x.mean(), e, se))
        assert se > 0 and abs(x.mean() - e) <= 4 * se


def test_need_is_the_documented_function():
    tr, counts = small_case(7, S=4, M=20)
    for chunk in (None, 5):
        z = E.alpha_sizes(counts, depths=(1, 4, 10 ** 6), reps=3, chunk=chunk, **tr.args())
        tot = counts.sum(0)
        assert z["n_cell"] == int((counts > 0).sum()) and z["max_nnz"] == int((counts > 0).sum(0).max()) and z["n_branch"] == tr.B
        assert z["n_entry"] == sum(tr.entries(counts[:, j]) for j in range(4))
        assert z["max_chunk"] == int(max(-(-int(t) // (chunk or 16384)) for t in tot))
        assert z["n_draw"] == 4 + 3 * int((tot >= 1).sum() + (tot >= 4).sum())
        for n_draw in (0, 1, z["n_draw"]):
            want = 32 * 4 + 4 * (2 * z["n_cell"] + 4) + 16 * z["n_entry"] + n_draw * (1136 + 4 * z["max_nnz"] + 24 * z["max_chunk"]) + 2 ** 20
            assert E.alpha_need(4, z["n_cell"], z["n_entry"], z["max_nnz"], z["max_chunk"], n_draw) == want
    assert E.alpha_need(4, -1, 0, 0, 0, 0) == -1 and E.alpha_need(4, 0, 0, 0, 0, -2) == -1
    need = E.alpha_need(4, z["n_cell"], z["n_entry"], z["max_nnz"], z["max_chunk"], 1)
    with pytest.raises(E.EngineError, match=r"1 resident draw\(s\) of 4 samples need %d bytes of device memory, the budget is %d bytes" % (need, need - 1)):
        E.alpha_diversity(counts, depths=(1,), reps=1, chunk=5, mem_budget=need - 1, **tr.args())


def test_what_the_library_refuses():
    tr, counts = small_case()
    a = tr.args()
    for kw, why in ((dict(depths=(0, 3), reps=1), "depth 0 is 0"), (dict(depths=(3, 3), reps=1), "ascend strictly: 3 follows 3"), (dict(depths=(4, 2), reps=1), "ascend strictly"),
                    (dict(reps=-1), "reps -1 below 0"), (dict(depths=(2,), reps=0), "reps must be at least 1"), (dict(key_bits=0), "key_bits 0: 1 .. 64"),
                    (dict(key_bits=65), "key_bits 65"), (dict(chunk=0), "chunk 0: 1 .. 16777216"), (dict(chunk=2 ** 24 + 1), "chunk"), (dict(draw_chunk=-1), "draw_chunk -1 below 0"),
                    (dict(mem_budget=-5), "mem_budget -5 below 0")):
        with pytest.raises(E.EngineError, match=why):
            E.alpha_diversity(counts, **kw, **a)                     # device 0: refused before a device is asked for
    big = np.ones((1, 2 ** 11 + 1))
    with pytest.raises(E.EngineError, match="more than 2\\^31 draws"):
        E.alpha_diversity(big, depths=range(1, 1025), reps=1024)
    for bad, why in ((-1.0, "not a non-negative integer"), (1.5, "not a non-negative integer"), (float("nan"), "not a non-negative integer"), (2.0 ** 32, "below 2\\^32")):
        c = counts.copy(); c[1, 1] = bad
        with pytest.raises(E.EngineError, match=why):
            E.alpha_diversity(c, **a)
    c = counts.copy(); c[:, 0] = 2.0 ** 31
    with pytest.raises(E.EngineError, match="sample 0 holds 2\\^32 reads or more"):
        E.alpha_diversity(c, **a)
    c = counts.copy(); c[:, 2] = 0
    with pytest.raises(E.EngineError, match="sample 2 has no reads"):
        E.alpha_diversity(c, **a)
    with pytest.raises(E.EngineError, match="names node 99"):
        E.alpha_diversity(counts, otu_node=np.full(12, 99), parent=tr.parent, blen=tr.blen)
    par = tr.parent.copy(); par[0] = 1
    with pytest.raises(E.EngineError, match="no root|cycle|has the parent"):
        E.alpha_diversity(counts, otu_node=tr.nodes, parent=par, blen=tr.blen)
    bl = tr.blen.copy(); bl[tr.nodes[0]] = -1.0
    with pytest.raises(E.EngineError, match="has the length -1"):
        E.alpha_diversity(counts, otu_node=tr.nodes, parent=tr.parent, blen=bl)


# ---- the program ----

def _write_table(path, ids, samples, counts):
    E.otu_table_write(path, dict(otus=[str(i) for i in ids], taxa=[""] * len(ids), samples=samples, counts=counts), " OTU table generated by test")


def _rows(text, tail=0):
    lines = text.rstrip("\n").split("\n")
    body = lines[1:len(lines) - tail]
    return lines[0].split("\t"), [ln.split("\t") for ln in body], lines[len(lines) - tail:]


def _val(s):
    return float("nan") if s == "NA" else float(s)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """a small table on a tree written as a database, and the library's host result for it"""
    d = tmp_path_factory.mktemp("alpha")
    db = synth.make_db(20, 64, seed=4)
    synth.write_ptu(db, str(d / "db.ptu"))
    rng = np.random.default_rng(8)
    tr = Tree(db.parent, db.blen, rows_on(db.parent, 10, 8))
    counts = rng.integers(0, 30, (10, 4)).astype(np.float64) * (rng.random((10, 4)) < 0.7)
    counts[rng.integers(0, 10, 4), np.arange(4)] += 3
    counts[:, 3] = 0; counts[2, 3] = 6                             # a small sample: depths beyond it
    samples = ["s0", "a sample of two words", "s2", "tiny"]
    _write_table(d / "t.txt", tr.nodes, samples, counts)
    return dict(dir=d, db=str(d / "db"), table=d / "t.txt", tree=tr, counts=counts, samples=samples)


def _check_files(p, out, curve, draws, depths, reps, seed, with_tree, lib):
    tr = p["tree"] if with_tree else None
    names = ["observed", "singles", "doubles", "chao1", "shannon", "simpson", "goods_coverage"] + (["faith_pd"] if with_tree else [])
    head, rows, _ = _rows(out)
    assert head == ["sample", "reads"] + names and [r[0] for r in rows] == p["samples"]
    for j, r in enumerate(rows):
        assert int(r[1]) == int(p["counts"][:, j].sum()) and [int(x) for x in r[2:5]] == [int(lib["whole"][f][j]) for f in ("S", "F1", "F2")]
        assert [float(x).hex() for x in r[5:]] == [float(lib["whole"][f][j]).hex() for f in names[3:]]     # 17 digits parse back to the library's doubles
    head, rows, tail = _rows(draws, 1)
    assert head == ["sample", "depth", "rep"] + names and tail == ["# seed: %d" % seed] and len(rows) == 4 * len(depths) * reps
    at = 0
    for j in range(4):
        for d, m in enumerate(depths):
            for r in range(reps):
                row = rows[at]; at += 1
                assert row[:3] == [p["samples"][j], str(m), str(r)]
                if m > p["counts"][:, j].sum():
                    assert row[3:] == ["NA"] * len(names)
                else:
                    assert [int(x) for x in row[3:6]] == [int(lib["draws"][f][j, d, r]) for f in ("S", "F1", "F2")]
                    assert [float(x).hex() for x in row[6:]] == [float(lib["draws"][f][j, d, r]).hex() for f in names[3:]]
    cn = ["observed", "chao1", "shannon", "simpson", "goods_coverage"] + (["faith_pd"] if with_tree else [])
    head, rows, _ = _rows(curve)
    assert head == ["sample", "depth", "reps"] + [c + s for c in cn for s in ("_mean", "_sd")] and len(rows) == 4 * len(depths)
    at = 0
    for j in range(4):
        for d, m in enumerate(depths):
            row = rows[at]; at += 1
            exists = m <= p["counts"][:, j].sum()
            assert row[:3] == [p["samples"][j], str(m), str(reps if exists else 0)]
            for k, c in enumerate(cn):
                mean, sd = row[3 + 2 * k], row[4 + 2 * k]
                if not exists:
                    assert mean == "NA" and sd == "NA"
                    continue
                x = [float(v) for v in lib["draws"][c][j, d]]
                s = 0.0
                for v in x:
                    s += v
                mu = s / reps
                assert float(mean).hex() == mu.hex()
                if reps == 1:
                    assert sd == "NA"
                else:
                    q = 0.0
                    for v in x:
                        q += (v - mu) * (v - mu)
                    assert float(sd).hex() == math.sqrt(q / (reps - 1)).hex()


@pytest.mark.parametrize("with_tree, reps", [(True, 3), (False, 3), (True, 1)])
def test_program_on_the_host(tmp_path, prog, with_tree, reps):
    depths = [1, 2, 6, 7, 40]
    a = [_bin(), prog["table"], "--host", "-o", tmp_path / "o.txt", "--curve-out", tmp_path / "c.txt", "--draws-out", tmp_path / "d.txt", "--depths", "1,2,6,7,40",
         "--reps", reps, "-S", 9, "-v"] + (["--db", prog["db"]] if with_tree else [])
    r = _run(a)
    assert r.returncode == 0, r.stderr
    assert "seed 9, " in r.stderr and " draws and 4 whole samples" in r.stderr and "chunks of 16384 reads" in r.stderr
    lib = E.alpha_diversity(prog["counts"], depths=depths, reps=reps, seed=9, host=True, **(prog["tree"].args() if with_tree else {}))
    hold_all(lib, "prog", prog["counts"], prog["tree"] if with_tree else None, depths, reps, 9, 64, "host")
    _check_files(prog, (tmp_path / "o.txt").read_text(), (tmp_path / "c.txt").read_text(), (tmp_path / "d.txt").read_text(), depths, reps, 9, with_tree, lib)
    r = _run([_bin(), prog["table"], "--host"] + (["--db", prog["db"]] if with_tree else []))     # no depth option, no curve file: the whole samples, on the standard output
    assert r.returncode == 0 and r.stdout == (tmp_path / "o.txt").read_text()


def test_program_spaces_the_depths(tmp_path, prog):
    top = int(prog["counts"].sum(0).max())
    r = _run([_bin(), prog["table"], "--host", "--curve-out", tmp_path / "c.txt", "--steps", 4, "--reps", 1, "-o", tmp_path / "o.txt"])
    assert r.returncode == 0, r.stderr
    _, rows, _ = _rows((tmp_path / "c.txt").read_text())
    assert [int(x[1]) for x in rows[:4]] == [i * top // 4 for i in range(1, 5)]
    r = _run([_bin(), prog["table"], "--host", "--draws-out", tmp_path / "d.txt", "--steps", 7, "--max-depth", 3, "--reps", 2, "-o", tmp_path / "o.txt"])
    assert r.returncode == 0, r.stderr
    _, rows, tail = _rows((tmp_path / "d.txt").read_text(), 1)
    assert sorted({int(x[1]) for x in rows}) == [1, 2, 3] and tail == ["# seed: 1"]   # floor(i * 3 / 7): 0, 0, 1, 1, 2, 2, 3 with zeros and repeats dropped
    r = _run([_bin(), prog["table"], "--host", "--curve-out", tmp_path / "c10.txt", "-o", tmp_path / "o.txt"])    # neither: ten steps, ten repeats
    assert r.returncode == 0 and len(_rows((tmp_path / "c10.txt").read_text())[1]) == 4 * 10 and _rows((tmp_path / "c10.txt").read_text())[1][0][2] == "10"


def test_program_reads_what_sum_and_merge_write(tmp_path):
    from conftest import get_db
    db = get_db(120, 700, "GTR", dg_k=4)                            # the database the committed assignment files were made against
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    for f, o in (("cli_sampleA.tsv", "a.txt"), ("cli_sampleB.tsv", "b.txt")):
        assert _run([_bin("hmmufotu-amd-sum"), pre, os.path.join(GOLD, f), "-o", tmp_path / o]).returncode == 0
    assert _run([_bin("hmmufotu-amd-merge"), tmp_path / "a.txt", tmp_path / "b.txt", "-o", tmp_path / "m.txt"]).returncode == 0
    for name in ("a.txt", "m.txt"):
        t = E.otu_table_read(tmp_path / name)
        r = _run([_bin(), tmp_path / name, "--host", "--db", pre])
        assert r.returncode == 0, r.stderr
        tr = Tree(db.parent, db.blen, [int(x) for x in t["otus"]])
        head, rows, _ = _rows(r.stdout)
        assert [x[0] for x in rows] == t["samples"]
        for j, x in enumerate(rows):
            y = yard(t["counts"][:, j], tr)
            assert [int(v) for v in x[1:5]] == [y[f] for f in ("reads", "S", "F1", "F2")]
            rec = dict(shannon=[float(x[6])], A=[float(y["A"])], PD=[float(x[9])], faith_pd=[float(x[9])])
            hold(rec, 0, y, tr, "host", exact_ints=False)


REFUSED = [
    (["--depths", "1,2", "--steps", 3, "--curve-out", "c"], "--depths does not go with --steps or --max-depth"),
    (["--depths", "1,2", "--max-depth", 3, "--curve-out", "c"], "--depths does not go with --steps or --max-depth"),
    (["--curve-out", "c", "--reps", 0], "need draws: --reps must be at least 1"),
    (["--draws-out", "c", "--reps", 0, "--depths", "2"], "need draws: --reps must be at least 1"),
    (["--depths", "1,x", "--curve-out", "c"], "option --depths: 'x' is not a whole number"),
    (["--depths", "1,,2", "--curve-out", "c"], "option --depths: '' is not a whole number"),
    (["--reps", "-3"], "option --reps: '-3' is not a whole number"),
    (["--steps", "1e3", "--curve-out", "c"], "option --steps: '1e3' is not a whole number"),
    (["--steps", 0, "--curve-out", "c"], "--steps must lie between 1 and 1000000"),
    (["--max-depth", 0, "--curve-out", "c"], "--max-depth must lie between"),
    (["-S", "seven"], "option -S: 'seven' is not a whole number"),
    (["--chunk", 0], "--chunk must lie between 1 and 16777216"),
    (["--mem", "much"], "option --mem: 'much' is not a number"),
    (["--mem", 0], "--mem must be a positive number of GB"),
    (["--device", "-1"], "option --device: '-1' is not a whole number"),
    (["--depths", "3"], "go with --curve-out or --draws-out"),
    (["--depths", "0,3", "--curve-out", "c"], "depth 0 is 0"),
    (["--depths", "3,3", "--curve-out", "c"], "the depths must ascend strictly: 3 follows 3"),
    (["--depths", "5,2", "--draws-out", "c"], "the depths must ascend strictly: 2 follows 5"),
    (["--db", "nowhere/db"], "Unable to load Phylogenetic tree data 'nowhere/db.ptu'"),
    (["--bogus"], "unknown option --bogus"),
]


@pytest.mark.parametrize("args, why", REFUSED)
def test_what_the_program_refuses(tmp_path, prog, args, why):
    """without --host: every refusal comes before a device is asked for, so it reads the same on a machine without one"""
    args = [tmp_path / a if a == "c" else a for a in args]
    r = _run([_bin(), prog["table"], "-o", tmp_path / "o.txt"] + args)
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert not (tmp_path / "o.txt").exists() and not (tmp_path / "c").exists()


def test_program_refuses_tables_and_memory(tmp_path, prog):
    _write_table(tmp_path / "named.txt", ["Bacteria", "7"], ["s"], np.array([[1.0], [2.0]]))
    r = _run([_bin(), tmp_path / "named.txt", "--db", prog["db"]])
    assert r.returncode != 0 and "OTU id 'Bacteria' is not a node number: a tree needs tables made without --use-dbname" in r.stderr
    _write_table(tmp_path / "far.txt", ["5", "4000"], ["s"], np.array([[1.0], [2.0]]))
    r = _run([_bin(), tmp_path / "far.txt", "--db", prog["db"]])
    assert r.returncode != 0 and "OTU id '4000' is not a node of " in r.stderr
    _write_table(tmp_path / "empty.txt", ["5", "6"], ["s", "no reads"], np.array([[1.0, 0.0], [2.0, 0.0]]))
    r = _run([_bin(), tmp_path / "empty.txt"])
    assert r.returncode != 0 and "Sample 'no reads' has no reads" in r.stderr
    _write_table(tmp_path / "frac.txt", ["5", "6"], ["s"], np.array([[1.5], [2.0]]))
    r = _run([_bin(), tmp_path / "frac.txt", "--host"])
    assert r.returncode != 0 and "OTU '5' has a cell that is not a non-negative integer in sample 's'" in r.stderr
    z = E.alpha_sizes(prog["counts"], depths=(2,), reps=1, **prog["tree"].args())
    need = E.alpha_need(4, z["n_cell"], z["n_entry"], z["max_nnz"], z["max_chunk"], 1)
    r = _run([_bin(), prog["table"], "--db", prog["db"], "--mem", repr((need - 1) / 2.0 ** 30), "-o", tmp_path / "o.txt"])
    assert r.returncode != 0 and "need %d bytes of device memory, the budget is %d bytes" % (need, need - 1) in r.stderr, r.stderr
    assert not (tmp_path / "o.txt").exists()


def test_program_usage_and_missing_files(tmp_path, prog):
    r = _run([_bin(), prog["table"], prog["table"]])
    assert r.returncode != 0 and "Usage:" in r.stderr
    u = _run([_bin()])
    assert u.returncode == 0 and "--curve-out" in u.stderr and "--draws-out" in u.stderr and "--max-depth" in u.stderr and _run([_bin(), "--help"]).returncode == 0
    v = _run([_bin(), "--version"])
    assert v.returncode == 0 and "v1.5.1" in v.stderr
    r = _run([_bin(), tmp_path / "none.txt", "--host"])
    assert r.returncode != 0 and "Unable to open OTUTable" in r.stderr
    r = _run([_bin(), prog["table"], "--host", "-o", tmp_path / "no" / "where.txt"])
    assert r.returncode != 0 and "Unable to write to" in r.stderr
    r = _run([_bin(), prog["table"], "--host", "--curve-out", tmp_path / "no" / "where.txt"])
    assert r.returncode != 0 and "Unable to write to" in r.stderr
    r = _run([_bin(), prog["table"], "--depths"])
    assert r.returncode != 0 and "option --depths needs a value" in r.stderr


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_alpha_host.cpp (the checks, the plan, the host path, the metrics, the curve; no HIP headers) with hu_unifrac_host.cpp (the tree
    walk) and hu_otu_table.cpp (the cell checks) and tests/san/alpha_driver.cpp under AddressSanitizer + UBSan, run as a stand-alone
    program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "alpha_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "alpha_driver.cpp"), os.path.join(CSRC, "hu_alpha_host.cpp"), os.path.join(CSRC, "hu_unifrac_host.cpp"),
                        os.path.join(CSRC, "hu_otu_table.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "49 cases" in r.stdout


# ---- the device ----

def _tree_of(kind):
    if kind.startswith("chain"):
        return chain(int(kind[5:]))
    if kind == "star":
        return star(300)
    if kind == "unbalanced":
        return tree_shapes.tree(150, 2, 0, 1)[:2]
    return tree_shapes.tree(150, 3, 3, 1)[:2]                       # a trifurcating top node and polytomies below it


# samples, tree, chunk, reps, key_bits
DEVICE_CASES = [(1, "chain1", 64, 3, 64), (2, "star", 256, 3, 64), (10, "chain63", 64, 3, 4), (10, "chain64", 256, 3, 64), (10, "chain65", 64, 1, 64),
                (64, "unbalanced", 64, 1, 64), (65, "polytomy", 256, 1, 4)]
_DEV = {}


def device_case(S, kind, key_bits):
    """a table, its tree, its depths and the host path's result, made once"""
    key = (S, kind, key_bits)
    if key not in _DEV:
        parent, blen = _tree_of(kind)
        M = 258
        tr = Tree(parent, blen, rows_on(parent, M, S))
        counts = spec_table(M, S, 100 + S)
        depths = spec_depths(counts)
        _DEV[key] = (tr, counts, depths)
    return _DEV[key]


@pytest.mark.gpu
@pytest.mark.parametrize("S, kind, chunk, reps, key_bits", DEVICE_CASES)
def test_device_against_the_host_path(S, kind, chunk, reps, key_bits):
    """samples 1, 2, 64, 65; 1, 63, 64, 65 and 257 nonzero cells; a sample's reads within one chunk, one chunk exactly, one read more, several
    chunks, at chunks of 64 and 256 reads; depths 1, N_j - 1 and N_j of every sample and one beyond the smallest (from ten samples on more
    than 8 depths, so a (sample, repeat) spans two groups of depths); keys that tie; a chain, a star, an unbalanced tree and one with
    polytomies, each with the OTU that is the root; 1, 63, 64 and 65 kept branches"""
    _need_gpu()
    tr, counts, depths = device_case(S, kind, key_bits)
    if kind.startswith("chain"):
        assert tr.B == int(kind[5:])
    assert S < 10 or len(depths) > 8
    kw = dict(depths=depths, reps=reps, seed=21, key_bits=key_bits, **tr.args())
    host = E.alpha_diversity(counts, host=True, **kw)
    dev = E.alpha_diversity(counts, chunk=chunk, **kw)
    same(dev, host, skip=("A", "shannon"))                          # the integers and their metrics equal, PD bit for bit
    key = ("dev", S, kind)
    hold_all(dev, key, counts, tr, depths, reps, 21, key_bits, "device", pd_yard=False)
    hold_all(host, key, counts, tr, depths, reps, 21, key_bits, "host", pd_yard=S <= 2)
    t = E.alpha_timing()
    assert all(t[k] > 0 for k in ("to_device", "select", "take", "metrics", "pd", "to_host"))
    print("S %d %s: worst shannon deviation so far, host %.3g, device %.3g" % (S, kind, WORST["host"], WORST["device"]))


@pytest.mark.gpu
@pytest.mark.parametrize("key_bits", [4, 64])
@pytest.mark.parametrize("n_depth", [1, 8, 17])
def test_device_depths_against_the_width_of_a_group(n_depth, key_bits):
    """the draw kernels serve 8 depths of a (sample, repeat) per workgroup: 1 depth (seven idle), 8 (one full group) and 17 (two full groups
    and one depth, blockIdx.y 0 .. 2) of every (sample, repeat), with keys that tie and without.  Counts of 9, 11, 12, 14 and 16 are in
    DEVICE_CASES from ten samples on: the table of (10, "chain63", 64, 3, 4) has a sample with 9 depths and one with 16.  The host path
    is exact in the integers and in PD; A is a sum of at most 40 terms in another order, 40 roundings apart at the most"""
    _need_gpu()
    rng = np.random.default_rng(7)
    M = 40
    parent, blen = chain(9)
    tr = Tree(parent, blen, rows_on(parent, M, 3))
    counts = np.zeros((M, 3))
    for j, N in enumerate((300, 129, 65)):
        counts[:, j] = rng.multinomial(N, rng.dirichlet(np.full(M, 0.3)))
    depths = [33] if n_depth == 1 else sorted({int(x) for x in np.linspace(1, 65, n_depth)})   # 65: the whole of the smallest sample
    assert len(depths) == n_depth
    kw = dict(depths=depths, reps=2, seed=5, key_bits=key_bits, **tr.args())
    host = E.alpha_diversity(counts, host=True, **kw)
    dev = E.alpha_diversity(counts, chunk=64, **kw)
    same(dev, host, skip=("A", "shannon"))
    assert (host["draws"]["reads"] == np.array(depths)[None, :, None]).all()
    assert np.allclose(dev["draws"]["A"], host["draws"]["A"], rtol=40 * 2.0 ** -52, atol=0)


@pytest.mark.gpu
def test_device_results_do_not_depend_on_the_chunking():
    _need_gpu()
    tr, counts, depths = device_case(10, "chain63", 4)
    kw = dict(depths=depths, reps=3, seed=21, key_bits=4, **tr.args())
    base = E.alpha_diversity(counts, chunk=64, **kw)
    for more in (dict(chunk=64, draw_chunk=1), dict(chunk=64, draw_chunk=7), dict(chunk=256), dict(chunk=16384), dict(chunk=1000, draw_chunk=100)):
        same(base, E.alpha_diversity(counts, **more, **kw))
    same(base, E.alpha_diversity(counts, chunk=64, **kw))           # and not on the run
    no_tree = E.alpha_diversity(counts, chunk=64, depths=depths, reps=1, seed=21)
    assert np.isnan(no_tree["draws"]["PD"]).all() and E.alpha_timing()["pd"] == 0


@pytest.mark.gpu
def test_program_on_the_device(tmp_path, prog):
    _need_gpu()
    out = {}
    for tag, extra in (("dev", ["-v"]), ("host", ["--host"])):
        r = _run([_bin(), prog["table"], "--db", prog["db"], "-o", tmp_path / (tag + "_o.txt"), "--curve-out", tmp_path / (tag + "_c.txt"), "--draws-out", tmp_path / (tag + "_d.txt"),
                  "--depths", "1,2,6,7,40", "--reps", 3, "-S", 9, "--chunk", 5] + extra)
        assert r.returncode == 0, r.stderr
        out[tag] = r
    assert "select " in out["dev"].stderr and "PD " in out["dev"].stderr and "copy back" in out["dev"].stderr
    for f, tail in (("_o.txt", 0), ("_c.txt", 0), ("_d.txt", 1)):
        hd, d, td = _rows((tmp_path / ("dev" + f)).read_text(), tail); hh, h, th = _rows((tmp_path / ("host" + f)).read_text(), tail)
        assert hd == hh and td == th and len(d) == len(h)
        loose = [k for k, name in enumerate(hd) if name.startswith("shannon")]
        for a, b in zip(d, h):
            for k in range(len(hd)):
                if k in loose and a[k] != "NA":
                    assert abs(float(a[k]) - float(b[k])) <= 2 * SHANNON_BAR * math.log(40)
                else:
                    assert a[k] == b[k], (f, hd[k], a, b)


@pytest.mark.gpu
def test_device_memory_refusal_and_a_budget_that_is_respected():
    _need_gpu()
    tr, counts, depths = device_case(10, "chain64", 64)
    kw = dict(depths=depths, reps=1, seed=21, chunk=256, **tr.args())
    z = E.alpha_sizes(counts, depths=depths, reps=1, chunk=256, **tr.args())
    one = E.alpha_need(10, z["n_cell"], z["n_entry"], z["max_nnz"], z["max_chunk"], 1)
    same(E.alpha_diversity(counts, mem_budget=one, **kw), E.alpha_diversity(counts, **kw))      # one draw at a time fits
    with pytest.raises(E.EngineError, match=r"need %d bytes of device memory, the budget is %d bytes" % (one, one - 1)):
        E.alpha_diversity(counts, mem_budget=one - 1, **kw)
    five = E.alpha_need(10, z["n_cell"], z["n_entry"], z["max_nnz"], z["max_chunk"], 5)
    with pytest.raises(E.EngineError, match=r"5 resident draw\(s\) of 10 samples need %d bytes of device memory, the budget is %d bytes" % (five, five - 1)):
        E.alpha_diversity(counts, mem_budget=five - 1, draw_chunk=5, **kw)
    same(E.alpha_diversity(counts, mem_budget=five, draw_chunk=5, **kw), E.alpha_diversity(counts, **kw))


def test_zz_the_shannon_bar_covers_what_was_measured():
    """last in the file: the largest |H - H_exact| / max(1, ln N) the cases above met; the bar is four times the figure of the module's
    docstring, rounded up to a power of two"""
    print("worst shannon deviation: host %.3g, device %.3g; the bar %.3g" % (WORST["host"], WORST["device"], SHANNON_BAR))
    assert max(WORST.values()) <= SHANNON_BAR
