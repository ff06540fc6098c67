"""hmmufotu-amd-unifrac --rarefy: the distances between the samples of an OTU table averaged over rarefied draws,
hu_unifrac_rarefied on the host and on the device, and the program.

The yardstick is written here and shares no code with the entry.  Draw r is taken by name: the columns of
engine.otu_subset(counts, M, seed=seed + r, device=-1), which tests/test_otu_tools.py pins.  Its distances are restated from the
definition in include/hmmufotu_amd.h: a walk from every OTU to the root, the reads below every branch as Python integers, the lengths as
the exact integers of their doubles over 2^1074, and every distance a fractions.Fraction.  Only `generalized` is not exact: its terms are
float64, added with math.fsum.

Bars, all DESIGN.md §20's, none made for this file: a draw is held to (B + 8) x 2^-52 x scale against the rational value (scale 1 for
the normalised methods, sum b_v (p_vi + p_vj) for weighted-raw), `generalized` to 2^-48 against the fsum restatement, and bit for bit to
engine.unifrac of the same draw table with the same slab, host against host and device against device.  mean and sd are held bit for bit
to a restatement of Welford's recurrence over the returned draws in plain float64 operations, one per step."""
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_shapes  # noqa: E402
from hmmufotu_amd import engine as E, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
U = Fraction(1, 2 ** 52)
GEN_BAR = 2.0 ** -48
SCALE = 2 ** 1074
IDENT = ("bray-curtis", "jaccard")
ALL = [("unweighted", None), ("weighted", None), ("weighted-raw", None), ("generalized", 0.5), ("generalized", 0.3), ("generalized", 0.0), ("generalized", 1.0),
       ("bray-curtis", None), ("jaccard", None)]
EXACT = [(m, a) for m, a in ALL if not (m == "generalized" and a not in (1.0,))]
M64 = 2 ** 64 - 1


def _bin(name="hmmufotu-amd-unifrac"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ---- the yardstick ----

class Yard:
    """the branches of a table's ids: parent [nodes] (-1: the root), blen [nodes], otu_node [rows]; parent None: the identity tree"""

    def __init__(self, parent, blen, otu_node, n_rows):
        if parent is None:
            parent = [-1] + [0] * n_rows; blen = [0.0] + [1.0] * n_rows; otu_node = list(range(1, n_rows + 1))
        self.parent = [int(p) for p in parent]
        self.paths = []                                              # per row: the nodes below the branches above it
        seen = {}
        for u in otu_node:
            v = int(u); path = []
            while self.parent[v] >= 0:
                path.append(seen.setdefault(v, len(seen))); v = self.parent[v]
            self.paths.append(path)
        self.B = len(seen)
        self.b = [0] * self.B; self.bf = [0.0] * self.B
        for v, k in seen.items():
            self.b[k] = int(Fraction(float(blen[v])) * SCALE); self.bf[k] = float(blen[v])

    def below(self, X):
        """N [B][S]: the reads of every sample below every branch"""
        S = X.shape[1]
        N = [[0] * S for _ in range(self.B)]
        for path, row in zip(self.paths, X):
            cells = [int(x) for x in row]
            for k in path:
                Nk = N[k]
                for j, c in enumerate(cells):
                    if c:
                        Nk[j] += c
        return N

    def matrix(self, X, method, alpha):
        """(d, scale) of the table X [rows][S] of whole numbers: d [S][S] Fractions (floats for generalized)"""
        X = np.asarray(X)
        S = X.shape[1]
        assert (X == np.round(X)).all()
        T = [int(t) for t in X.sum(0)]
        N = self.below(X)
        gen = method == "generalized" and alpha != 1.0
        if method == "generalized" and not gen:
            method = "weighted"
        d = [[0.0 if gen else Fraction(0)] * S for _ in range(S)]; scale = [[Fraction(1)] * S for _ in range(S)]
        pf = [[float(Fraction(Nk[j], T[j])) for j in range(S)] for Nk in N] if gen else None
        for i in range(S):
            for j in range(i + 1, S):
                if gen:
                    num = []; den = []
                    for k in range(self.B):
                        x = pf[k][i]; y = pf[k][j]; s = x + y
                        if s > 0:
                            w = self.bf[k] * s ** alpha
                            num.append(w * (abs(x - y) / s)); den.append(w)
                    dn = math.fsum(den)
                    d[i][j] = d[j][i] = math.fsum(num) / dn if dn > 0 else 0.0
                    continue
                num = den = 0
                if method == "unweighted":
                    for k in range(self.B):
                        x = N[k][i] > 0; y = N[k][j] > 0
                        if x != y:
                            num += self.b[k]
                        if x or y:
                            den += self.b[k]
                else:
                    ti = T[i]; tj = T[j]
                    for k in range(self.B):
                        x = N[k][i] * tj; y = N[k][j] * ti
                        if x or y:
                            num += self.b[k] * abs(x - y); den += self.b[k] * (x + y)
                if method == "weighted-raw":
                    tt = T[i] * T[j] * SCALE
                    d[i][j] = d[j][i] = Fraction(num, tt); scale[i][j] = scale[j][i] = Fraction(den, tt)
                else:
                    d[i][j] = d[j][i] = Fraction(num, den) if den else Fraction(0)
        return d, scale


def hold(got, yard, X, method, alpha, what=""):
    """one draw's distances against the yardstick of its table; prints the worst figure before it asserts"""
    tm = {"bray-curtis": "weighted", "jaccard": "unweighted"}.get(method, method)
    a = 0.5 if alpha is None else alpha
    exact, scale = yard.matrix(X, tm, a)
    S = got.shape[0]
    worst = 0.0; bad = None
    for i in range(S):
        assert got[i, i] == 0.0
        for j in range(i + 1, S):
            assert got[i, j].tobytes() == got[j, i].tobytes()
            if tm == "generalized" and a != 1.0:
                err = abs(got[i, j] - exact[i][j]); ok = err <= GEN_BAR
            else:
                err = abs(Fraction(float(got[i, j])) - exact[i][j]); ok = err <= (yard.B + 8) * U * scale[i][j]
            worst = max(worst, float(err))
            if not ok and bad is None:
                bad = (what, method, alpha, i, j, float(got[i, j]), float(exact[i][j]), float(err))
    print("%s %s alpha %s: B %d, S %d, worst deviation %.3g" % (what, method, alpha, yard.B, S, worst))
    assert bad is None, bad


def welford(draws):
    """mean and sd of draws [R][S][S] by the recurrence of include/hmmufotu_amd.h: numpy's elementwise float64 operations, one per step"""
    R = draws.shape[0]
    mean = np.zeros(draws.shape[1:]); m2 = np.zeros(draws.shape[1:])
    for r in range(1, R + 1):
        x = draws[r - 1]
        d = x - mean
        q = d / np.float64(r)
        mean = mean + q
        e = x - mean
        p = d * e
        m2 = m2 + p
    if R == 1:
        return mean, np.full(mean.shape, np.nan)
    return mean, np.sqrt(m2 / np.float64(R - 1))


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and ((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all()


# ---- trees and tables ----

def chain(B, seed=0):
    """a chain of B + 3 nodes: a row on node B keeps exactly B branches"""
    rng = np.random.default_rng(100 + seed)
    n = B + 3
    return np.arange(-1, n - 1, dtype=np.int32), np.r_[0.0, rng.exponential(0.05, n - 1) + 1e-5]


def shape_tree(seed=1):
    """a tree_shapes tree: a trifurcating top node and two polytomies below it"""
    par, bl, _ = tree_shapes.tree(40, 3, 2, seed)
    return np.asarray(par, np.int32), np.asarray(bl, np.float64)


def table(n_nodes, M, totals, seed, special=True):
    """M rows and a sample per total.  With `special`: row 0 on the root, rows 1 and 2 on one node, the last row all zero"""
    rng = np.random.default_rng(seed)
    nodes = rng.integers(1, n_nodes, M).astype(np.int32)
    live = M
    if special and M >= 5:
        nodes[0] = 0; nodes[2] = nodes[1]; live = M - 1
    counts = np.zeros((M, len(totals)))
    for j, t in enumerate(totals):
        p = rng.random(live) * (rng.random(live) < 0.6); p[rng.integers(live)] += 0.5
        counts[:live, j] = rng.multinomial(int(t), p / p.sum())
    return nodes, counts


def call(par, bl, nodes, counts, method, alpha, **kw):
    if method in IDENT:
        return E.unifrac_rarefied(counts, method=method, alpha=alpha, **kw)
    return E.unifrac_rarefied(counts, nodes, par, bl, method=method, alpha=alpha, **kw)


def unifrac_of(par, bl, nodes, X, method, alpha, **kw):
    if method in IDENT:
        return E.unifrac(X, method=method, alpha=alpha, **kw)
    return E.unifrac(X, nodes, par, bl, method=method, alpha=alpha, **kw)


_SUB = {}


def draw_table(counts, depth, seed, r, key_bits=64):
    """the draw's table by name: every column of otu_subset on the original table, then the kept ones"""
    key = (counts.tobytes(), counts.shape, depth, (seed + r) & M64, key_bits)
    if key not in _SUB:
        sub = E.otu_subset(counts, depth, seed=(seed + r) & M64, device=-1, key_bits=key_bits)
        _SUB[key] = np.ascontiguousarray(sub[:, counts.sum(0) >= depth])
    return _SUB[key]


def check(par, bl, nodes, counts, depth, reps, seed, method, alpha, host, yard=None, slab=0, key_bits=64, **kw):
    """one call held to everything the issue names; returns its dict"""
    got = call(par, bl, nodes, counts, method, alpha, depth=depth, reps=reps, seed=seed, slab=slab, host=host, key_bits=key_bits, draws=True, **kw)
    keep = counts.sum(0) >= depth
    K = int(keep.sum())
    assert got["kept"].tolist() == keep.tolist()
    assert got["draws"].shape == (reps, K, K) and got["mean"].shape == (K, K) and got["sd"].shape == (K, K)
    for r in range(reps):
        X = draw_table(counts, depth, seed, r, key_bits)
        assert (X.sum(0) == depth).all()
        D = got["draws"][r]
        assert (np.diag(D) == 0).all() and D.tobytes() == D.T.copy().tobytes()
        ref = unifrac_of(par, bl, nodes, X, method, alpha, slab=slab, host=host)
        assert D.tobytes() == ref.tobytes(), ("draw %d is not unifrac of its table" % r, method, alpha, np.abs(D - ref).max())
        if yard is not None:
            hold(D, yard, X, method, alpha, "draw %d" % r)
    mean, sd = welford(got["draws"])
    assert same(got["mean"], mean) and same(got["sd"], sd), (method, alpha)
    assert (np.diag(got["mean"]) == 0).all() and got["mean"].tobytes() == got["mean"].T.copy().tobytes()
    assert (np.isnan(got["sd"]).all() if reps == 1 else (np.diag(got["sd"]) == 0).all()) and same(got["sd"], got["sd"].T.copy())
    return got


def yard_of(par, bl, nodes, counts, method):
    return Yard(None, None, None, counts.shape[0]) if method in IDENT else Yard(par, bl, nodes, counts.shape[0])


_CASE = {}


def small():
    """a tree_shapes tree, 12 rows, 6 samples; totals 30 (the smallest, twice), 31, 64, 65 and 90"""
    if "small" not in _CASE:
        par, bl = shape_tree()
        nodes, counts = table(len(par), 12, [64, 30, 90, 31, 65, 30], 7)
        _CASE["small"] = (par, bl, nodes, counts)
    return _CASE["small"]


def named():
    """the program's table: as small(), but every row on a node of its own, since a table file names an OTU once"""
    if "named" not in _CASE:
        par, bl = shape_tree()
        _, counts = table(len(par), 12, [64, 30, 90, 31, 65, 30], 7, special=False)
        nodes = np.random.default_rng(5).choice(np.arange(len(par)), 12, replace=False).astype(np.int32)
        _CASE["named"] = (par, bl, nodes, counts)
    return _CASE["named"]


# ---- the host path ----

def test_the_restatement_on_a_five_node_tree():
    """sample A: half below 3 (and 1), half below 2; sample B: half below 4 (and 1), half below 2"""
    y = Yard([-1, 0, 0, 1, 1], [0, 1, 2, 0.5, 0.25], [3, 4, 2], 3)
    X = np.array([[2, 0], [0, 1], [2, 1]])
    assert y.B == 4
    assert y.matrix(X, "weighted", 0.5)[0][0][1] == Fraction(1, 9)
    assert y.matrix(X, "weighted-raw", 0.5)[0][0][1] == Fraction(3, 8) and y.matrix(X, "weighted-raw", 0.5)[1][0][1] == Fraction(27, 8)
    assert y.matrix(X, "unweighted", 0.5)[0][0][1] == Fraction(1, 5)
    r = 0.75 * math.sqrt(0.5)
    assert abs(y.matrix(X, "generalized", 0.5)[0][0][1] - r / (r + 3)) < 1e-15
    i = Yard(None, None, None, 3)
    assert i.matrix(X, "weighted", 0.5)[0][0][1] == Fraction(1, 2) and i.matrix(X, "unweighted", 0.5)[0][0][1] == Fraction(2, 3)
    m, s = welford(np.array([[[1.0]], [[2.0]], [[4.0]]]))
    assert m[0, 0] == pytest.approx(7 / 3, abs=1e-15) and s[0, 0] == pytest.approx(math.sqrt(7 / 3), abs=1e-15)


@pytest.mark.parametrize("method, alpha", ALL)
def test_host_every_method(method, alpha):
    """every method at M = 1, the smallest N_j (two samples are whole in every draw) and one above it (they are dropped); R = 1, 2, 5"""
    par, bl, nodes, counts = small()
    y = yard_of(par, bl, nodes, counts, method)
    for depth, reps in ((1, 5), (30, 2), (31, 1), (31, 5)):
        got = check(par, bl, nodes, counts, depth, reps, 11, method, alpha, True, yard=y if reps < 5 else None)
        assert got["kept"].tolist() == ([True] * 6 if depth <= 30 else [True, False, True, True, True, False])


def test_host_root_only_and_shared_nodes():
    """every read on the root: no branch, every distance 0; two rows on one node are one OTU to the tree"""
    par, bl = shape_tree()
    c = np.array([[3.0, 5.0, 4.0]])
    got = E.unifrac_rarefied(c, [0], par, bl, depth=3, reps=2, host=True, draws=True)
    assert not got["mean"].any() and not got["sd"].any() and not got["draws"].any() and got["kept"].all()
    c2 = np.array([[4.0, 0.0, 2.0], [0.0, 4.0, 2.0]])
    got = E.unifrac_rarefied(c2, [5, 5], par, bl, depth=4, reps=3, host=True)
    assert not got["mean"].any() and not got["sd"].any()


def test_host_equal_totals_at_full_depth_is_unifrac():
    """all samples with N reads and M = N: every draw is the table, mean is engine.unifrac bit for bit and sd exactly 0"""
    par, bl = shape_tree()
    nodes, counts = table(len(par), 12, [40] * 5, 3)
    for method, alpha in ALL:
        got = call(par, bl, nodes, counts, method, alpha, depth=40, reps=5, seed=2, host=True, draws=True)
        ref = unifrac_of(par, bl, nodes, counts, method, alpha, host=True)
        assert got["mean"].tobytes() == ref.tobytes() and not got["sd"].any() and all(d.tobytes() == ref.tobytes() for d in got["draws"])


def test_host_seed_wraps_at_2_64():
    par, bl, nodes, counts = small()
    got = check(par, bl, nodes, counts, 20, 3, M64 - 1, "weighted", None, True)       # seeds 2^64 - 2, 2^64 - 1, 0
    assert got["draws"][2].tobytes() == E.unifrac_rarefied(counts, nodes, par, bl, depth=20, reps=1, seed=0, host=True, draws=True)["draws"][0].tobytes()
    assert got["draws"][1].tobytes() == E.unifrac_rarefied(counts, nodes, par, bl, depth=20, reps=1, seed=M64, host=True, draws=True)["draws"][0].tobytes()


def test_host_keys_that_tie():
    par, bl, nodes, counts = small()
    for method, alpha in (("weighted", None), ("unweighted", None), ("bray-curtis", None)):
        check(par, bl, nodes, counts, 20, 2, 5, method, alpha, True, key_bits=4, yard=yard_of(par, bl, nodes, counts, method))
    a = E.unifrac_rarefied(counts, nodes, par, bl, depth=20, reps=2, seed=5, host=True, key_bits=4)["mean"]
    assert a.tobytes() != E.unifrac_rarefied(counts, nodes, par, bl, depth=20, reps=2, seed=5, host=True)["mean"].tobytes()


def test_host_slabs_and_dropped_columns_do_not_renumber():
    par, bl, nodes, counts = small()
    for slab in (1, 7, 32, 10 ** 6):
        check(par, bl, nodes, counts, 31, 2, 3, "weighted", None, True, slab=slab)
    # the draw of a kept sample is keyed by its original column: the kept columns alone, as a table of their own, draw otherwise
    keep = counts.sum(0) >= 31
    a = E.unifrac_rarefied(counts, nodes, par, bl, depth=31, reps=1, seed=3, host=True)["mean"]
    b = E.unifrac_rarefied(np.ascontiguousarray(counts[:, keep]), nodes, par, bl, depth=31, reps=1, seed=3, host=True)["mean"]
    assert a.shape == b.shape and a.tobytes() != b.tobytes()


def test_need_is_the_documented_function():
    def want(n_sample, n_kept, n_cell, n_entry, max_nnz, max_chunk, n_branch, slab, dc, wd):
        Sp = (n_kept + 63) // 64 * 64; nt = Sp // 64; tiles = nt * (nt + 1) // 2; slabs = (n_branch + slab - 1) // slab
        return (32 * n_sample + 4 * (2 * n_cell + n_sample) + 20 * n_entry + 8 * n_branch
                + dc * (n_kept * (1096 + 4 * max_nnz + 24 * max_chunk) + 8 * n_branch * Sp + 65536 * slabs * tiles)
                + (dc if wd else 0) * 8 * n_kept ** 2 + 16 * n_kept ** 2 + 2 ** 20)
    for args in ((6, 4, 50, 200, 12, 1, 77, 256, 1, False), (131, 129, 900, 4000, 24, 3, 133, 32, 7, True), (2, 2, 2, 2, 1, 1, 1, 1, 0, True),
                 (5000, 4999, 10 ** 6, 10 ** 7, 900, 70, 198642, 198642, 100, False)):
        assert E.unifrac_rarefied_need(*args) == want(*args), args
    assert E.unifrac_rarefied_need(6, 4, 50, 200, 12, 1, 77, 0, 1) == -1 and E.unifrac_rarefied_need(6, -1, 50, 200, 12, 1, 77, 1, 1) == -1
    par, bl, nodes, counts = small()
    sz = E.unifrac_rarefied_sizes(counts, nodes, par, bl, depth=31, reps=2)
    y = Yard(par, bl, nodes, 12)
    assert sz["n_kept"] == 4 and sz["n_cell"] == int((counts > 0).sum()) and sz["n_branch"] == y.B and sz["max_depth2"] == 65
    assert sz["max_nnz"] == int((counts > 0).sum(0).max()) and sz["max_chunk"] == 1 and sz["slab"] == E.unifrac_default_slab(4, y.B)
    assert sz["n_entry"] == sum(1 for row in y.below(counts) for v in row if v > 0)
    assert E.unifrac_rarefied_sizes(counts, nodes, par, bl, depth=31, reps=2, chunk=16)["max_chunk"] == 6
    ident = E.unifrac_rarefied_sizes(counts, depth=31, reps=2, method="jaccard")
    assert ident["n_branch"] == 12 and ident["n_entry"] == ident["n_cell"]


def test_what_the_library_refuses():
    par, bl, nodes, counts = small()
    kw = dict(otu_node=nodes, parent=par, blen=bl, host=True)
    for bad, why in ((dict(depth=0, reps=1), "depth is 0"), (dict(depth=5, reps=0), "0 repeats: 1 .. 100000"), (dict(depth=5, reps=100001), "100001 repeats"),
                     (dict(depth=5, reps=-1), "repeats"), (dict(depth=91, reps=1), r"0 sample\(s\) have 91 reads or more: distances need 2; the largest depth that keeps 2 samples is 65"),
                     (dict(depth=66, reps=1), r"1 sample\(s\) have 66 reads or more.*keeps 2 samples is 65"),
                     (dict(depth=5, reps=1, method="generalized", alpha=1.5), "alpha"), (dict(depth=5, reps=1, alpha=0.3), "alpha goes with the generalized"),
                     (dict(depth=5, reps=1, method="jaccard"), "take no tree"), (dict(depth=5, reps=1, slab=-1), "slab"),
                     (dict(depth=5, reps=1, key_bits=0), "key_bits"), (dict(depth=5, reps=1, chunk=0), "chunk"), (dict(depth=5, reps=1, draw_chunk=-1), "draw_chunk"),
                     (dict(depth=5, reps=1, mem_budget=-1), "mem_budget")):
        with pytest.raises(E.EngineError, match=why):
            E.unifrac_rarefied(counts, **dict(kw, **bad))
    assert E.unifrac_rarefied(counts, depth=65, reps=1, **kw)["kept"].sum() == 2     # the depth the message names does keep 2
    with pytest.raises(E.EngineError, match="needs a tree"):
        E.unifrac_rarefied(counts, depth=5, reps=1, host=True)
    with pytest.raises(E.EngineError, match="names node 399"):
        E.unifrac_rarefied(counts, np.r_[nodes[:-1], 399], par, bl, depth=5, reps=1, host=True)
    with pytest.raises(E.EngineError, match="cycle|no root"):
        E.unifrac_rarefied(np.array([[5.0, 6.0], [1.0, 4.0]]), [1, 2], [-1, 2, 1], [0, 1, 1], depth=5, reps=1, host=True)
    for cell, why in ((1.5, "not a non-negative integer"), (-1.0, "negative"), (np.nan, "not finite|not a non-negative"), (2.0 ** 32, r"below 2\^32")):
        x = counts.copy(); x[3, 2] = cell
        with pytest.raises(E.EngineError, match=why):
            E.unifrac_rarefied(x, depth=5, reps=1, **kw)
    x = counts.copy(); x[:, 2] = 0
    with pytest.raises(E.EngineError, match="sample 2 has no reads"):
        E.unifrac_rarefied(x, depth=5, reps=1, **kw)
    with pytest.raises(E.EngineError, match="1 sample: distances need 2"):
        E.unifrac_rarefied(counts[:, :1], depth=5, reps=1, **kw)
    with pytest.raises(E.EngineError, match="depth and reps are required"):
        E.unifrac_rarefied(counts, **kw)
    with pytest.raises(E.EngineError, match="budget is 4096 bytes"):               # the budget is checked before a device is asked for
        E.unifrac_rarefied(counts, nodes, par, bl, depth=5, reps=1, mem_budget=4096)
    with pytest.raises(TypeError):                                                # PD cannot be asked for: alpha_diversity has the rarefied PD
        E.unifrac_rarefied(counts, depth=5, reps=1, pd=True, **kw)


# ---- the program ----

def _write_table(path, ids, samples, counts):
    E.otu_table_write(path, dict(otus=[str(i) for i in ids], taxa=[""] * len(ids), samples=samples, counts=counts), " OTU table generated by test")


def _fmt(samples, d):
    """the matrix as the program writes it"""
    out = "".join("\t" + s for s in samples) + "\n"
    for s, row in zip(samples, d):
        out += s + "".join("\t" + ("NA" if np.isnan(v) else "%.17g" % v) for v in row) + "\n"
    return out


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    """a database whose tree is the tree_shapes tree, and the named table on it"""
    d = tmp_path_factory.mktemp("unifrac_rarefied")
    par, bl, nodes, counts = named()
    n = len(par)
    db = synth.SynthDB(n, 1, par, bl, np.zeros((n, 1), np.int8), np.zeros((n, 1, 4)), np.zeros((n, 1, 4)), np.zeros(n), synth.load_model("JC69"),
                       is_leaf=~np.isin(np.arange(n), par), names=["n%d" % i for i in range(n)], annos=["k__Synth"] * n, anno_dist=np.zeros(n))
    synth.write_ptu(db, str(d / "db.ptu"))
    samples = ["s0", "a sample of two words", "s2", "s3", "s4", "s5"]
    _write_table(d / "t.txt", nodes, samples, counts)
    return dict(dir=d, db=str(d / "db"), table=d / "t.txt", samples=samples)


@pytest.mark.parametrize("args, why", [
    (["--reps", "5"], "--reps goes with --rarefy only"),
    (["--seed", "5"], "--seed goes with --rarefy only"),
    (["-S", "5"], "--seed goes with --rarefy only"),
    (["--sd-out", "SD"], "--sd-out goes with --rarefy only"),
    (["--draw-chunk", "2"], "--draw-chunk goes with --rarefy only"),
    (["--rarefy", "10", "--pd", "PD"], "--pd does not go with --rarefy"),
    (["--rarefy", "0"], "--rarefy must be at least 1"),
    (["--rarefy", "10", "--reps", "0"], "--reps must lie between 1 and 100000"),
    (["--rarefy", "10", "--reps", "100001"], "--reps must lie between 1 and 100000"),
    (["--rarefy", "10", "--draw-chunk", "0"], "--draw-chunk must be at least 1"),
    (["--rarefy", "91"], "the largest depth that keeps 2 samples is 65"),
])
def test_what_the_program_refuses(tmp_path, prog, args, why):
    out = tmp_path / "d.txt"; sd = tmp_path / "sd.txt"; pd = tmp_path / "pd.txt"
    r = _run([_bin(), prog["table"], "--db", prog["db"], "-o", out] + [{"SD": str(sd), "PD": str(pd)}.get(a, a) for a in args])
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert len(r.stderr.strip().split("\n")) == 1
    assert "device" not in r.stderr                                              # refused before a device is asked for: this test runs without one
    assert not out.exists() and not sd.exists() and not pd.exists()


def test_program_on_the_host(tmp_path, prog):
    par, bl, nodes, counts = named()
    keep = counts.sum(0) >= 31
    names = [s for s, k in zip(prog["samples"], keep) if k]
    for method, alpha in (("weighted", None), ("unweighted", None), ("generalized", 0.3), ("jaccard", None)):
        extra = ([] if method in IDENT else ["--db", prog["db"]]) + (["--alpha", alpha] if alpha is not None else [])
        r = _run([_bin(), prog["table"], "--host", "--method", method, "--rarefy", 31, "--reps", 5, "--seed", 9, "-o", tmp_path / "m.txt", "--sd-out", tmp_path / "sd.txt", "-v"] + extra)
        assert r.returncode == 0, r.stderr
        lib = call(par, bl, nodes, counts, method, alpha, depth=31, reps=5, seed=9, host=True)
        assert (tmp_path / "m.txt").read_text() == _fmt(names, lib["mean"]) and (tmp_path / "sd.txt").read_text() == _fmt(names, lib["sd"])
        assert "Sample 'a sample of two words' has fewer than 31 reads: dropped" in r.stderr and "Sample 's5' has fewer than 31 reads: dropped" in r.stderr
        assert "4 samples kept, 2 dropped" in r.stderr and "5 draws of 31 reads" in r.stderr
        back = E.dist_matrix_read(tmp_path / "m.txt")
        assert back["samples"] == names and back["dist"].tobytes() == lib["mean"].tobytes()
    r = _run([_bin(), prog["table"], "--host", "--db", prog["db"], "--rarefy", 31, "--reps", 1, "--sd-out", tmp_path / "sd1.txt"])      # defaults: seed 1; the mean on stdout
    lib = E.unifrac_rarefied(counts, nodes, par, bl, depth=31, reps=1, seed=1, host=True)
    assert r.returncode == 0 and r.stdout == _fmt(names, lib["mean"]) and (tmp_path / "sd1.txt").read_text() == _fmt(names, lib["sd"])
    assert (tmp_path / "sd1.txt").read_text().count("NA") == 16
    r = _run([_bin(), prog["table"], "--host", "--db", prog["db"], "--rarefy", 30, "-o", tmp_path / "d100.txt"])                        # 100 draws by default
    assert r.returncode == 0 and (tmp_path / "d100.txt").read_text() == _fmt(prog["samples"], E.unifrac_rarefied(counts, nodes, par, bl, depth=30, reps=100, host=True)["mean"])


def test_program_mean_feeds_permanova(tmp_path, prog):
    r = _run([_bin(), prog["table"], "--host", "--db", prog["db"], "--rarefy", 30, "--reps", 3, "-o", tmp_path / "m.txt"])
    assert r.returncode == 0, r.stderr
    assert not any(ln.startswith("#") for ln in (tmp_path / "m.txt").read_text().split("\n"))
    (tmp_path / "g.txt").write_text("".join("%s\t%s\n" % (s, "ab"[j % 2]) for j, s in enumerate(prog["samples"])))
    r = _run([_bin("hmmufotu-amd-permanova"), tmp_path / "m.txt", tmp_path / "g.txt", "--host", "--perms", 99])
    assert r.returncode == 0, r.stderr


def test_program_without_rarefy_is_unchanged(tmp_path, prog):
    par, bl, nodes, counts = named()
    for method in ("weighted", "unweighted", "bray-curtis"):
        extra = [] if method in IDENT else ["--db", prog["db"]]
        r = _run([_bin(), prog["table"], "--host", "--method", method, "-o", tmp_path / "d.txt"] + extra)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "d.txt").read_bytes() == _fmt(prog["samples"], unifrac_of(par, bl, nodes, counts, method, None, host=True)).encode()


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_unifrac_rarefied_host.cpp (the checks, the plan, the host path, the recurrence; no HIP headers) with hu_alpha_host.cpp,
    hu_unifrac_host.cpp and hu_otu_table.cpp (the subset's host selection) and tests/san/unifrac_rarefied_driver.cpp under
    AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "unifrac_rarefied_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "unifrac_rarefied_driver.cpp"), os.path.join(CSRC, "hu_unifrac_rarefied_host.cpp"),
                        os.path.join(CSRC, "hu_alpha_host.cpp"), os.path.join(CSRC, "hu_unifrac_host.cpp"), os.path.join(CSRC, "hu_otu_table.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "40"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "74 cases" in r.stdout


# ---- the device ----

def both(par, bl, nodes, counts, depth, reps, seed, method, alpha, yard=None, **kw):
    """the device held to everything `check` names, and to the host path: bit for bit, or within 2^-48 where pow or sqrt is taken"""
    dev = check(par, bl, nodes, counts, depth, reps, seed, method, alpha, False, yard=yard, **kw)
    hkw = {k: v for k, v in kw.items() if k in ("slab", "key_bits")}
    host = call(par, bl, nodes, counts, method, alpha, depth=depth, reps=reps, seed=seed, host=True, draws=True, **hkw)
    assert dev["kept"].tolist() == host["kept"].tolist()
    if method == "generalized" and alpha not in (1.0,):
        for f in ("draws", "mean"):
            worst = np.abs(dev[f] - host[f]).max()
            print("generalized alpha %g, %s: device against host %.3g" % (alpha, f, worst))
            assert worst <= GEN_BAR
        if reps > 1:
            assert np.abs(dev["sd"] - host["sd"]).max() <= GEN_BAR
    else:
        for f in ("draws", "mean", "sd"):
            assert same(dev[f], host[f]), (f, method, alpha)
    return dev


def wide(K):
    """K kept samples and two dropped ones (columns 1 and K, of 12 and 59 reads) on the tree_shapes tree, 16 rows; depth 60: sample 0 has
    exactly 60 reads (whole in every draw), sample 2 has 64 (one chunk of 64 reads), sample 3 (from K = 3 on) 65 (a chunk and one read)"""
    if ("wide", K) not in _CASE:
        par, bl = shape_tree()
        rng = np.random.default_rng(K)
        totals = ([60, 64, 65] + rng.integers(60, 300, max(K - 3, 0)).tolist())[:K]
        totals = totals[:1] + [12] + totals[1:]
        totals = totals[:K] + [59] + totals[K:]
        assert len(totals) == K + 2
        nodes, counts = table(len(par), 16, totals, 40 + K)
        _CASE[("wide", K)] = (par, bl, nodes, counts)
    return _CASE[("wide", K)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 63, 64, 65, 129])
def test_device_kept_sample_counts(K):
    """one tile, a tile's edge, three tile rows; two samples dropped; a whole sample, a sample of one chunk and of a chunk and one read"""
    _need_gpu()
    par, bl, nodes, counts = wide(K)
    assert int((counts.sum(0) >= 60).sum()) == K
    y = Yard(par, bl, nodes, 16)
    both(par, bl, nodes, counts, 60, 2, 3, "weighted", None, yard=y, chunk=64)
    for method, alpha in (("unweighted", None), ("weighted-raw", None), ("generalized", 0.5), ("generalized", 0.3), ("jaccard", None)):
        both(par, bl, nodes, counts, 60, 2, 3, method, alpha, yard=yard_of(par, bl, nodes, counts, method) if K <= 65 and method != "weighted-raw" else None, chunk=64)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 31, 32, 33, 65, 133])
def test_device_branch_counts(B):
    """chains that keep exactly B branches: the 32-branch staging chunk and its edges, slabs of 32, 64, all and the default"""
    _need_gpu()
    par, bl = chain(B, B)
    rng = np.random.default_rng(B)
    M = min(B, 6)
    nodes = np.array([B] + rng.integers(0, B + 1, M - 1).tolist(), np.int32)
    counts = np.zeros((M, 6))
    for j, t in enumerate([25, 40, 9, 25, 77, 31]):
        counts[:, j] = rng.multinomial(t, rng.dirichlet(np.ones(M)))
    y = Yard(par, bl, nodes, M)
    assert y.B == B and E.unifrac_rarefied_sizes(counts, nodes, par, bl, depth=25, reps=1)["n_branch"] == B
    for method, alpha in ALL[:7]:
        for slab in (32, 64, 1000000, 0):
            both(par, bl, nodes, counts, 25, 2, 8, method, alpha, yard=y if slab in (32, 0) else None, slab=slab)


@pytest.mark.gpu
def test_device_repeats_chunks_and_a_second_run():
    """R = 1, 2, 5 with 1, 2 and all draws resident (a chunk edge inside the run), 64 and 256 reads per workgroup: the same arrays every
    time, and on a second run; M = 1 and M = the smallest N_j; keys that tie; the root OTU and two rows on one node are in the table"""
    _need_gpu()
    par, bl, nodes, counts = wide(5)
    assert nodes[0] == 0 and nodes[1] == nodes[2] and counts[0].sum() > 0
    y = Yard(par, bl, nodes, 16)
    for depth, key_bits in ((60, 64), (1, 64), (12, 64), (60, 4)):
        for reps in (1, 2, 5):
            first = None
            for draw_chunk in (1, 2, 0):
                for chunk in (64, 256):
                    got = E.unifrac_rarefied(counts, nodes, par, bl, depth=depth, reps=reps, seed=17, draw_chunk=draw_chunk, chunk=chunk, key_bits=key_bits, draws=True)
                    assert E.unifrac_rarefied_timing()["resident_draws"] == (min(draw_chunk, reps) if draw_chunk else reps)
                    if first is None:
                        first = got
                    for f in ("kept", "draws", "mean", "sd"):
                        assert same(first[f].astype(np.float64), got[f].astype(np.float64)), (f, depth, reps, draw_chunk, chunk)
            again = both(par, bl, nodes, counts, depth, reps, 17, "weighted", None, yard=y if reps == 2 else None, key_bits=key_bits)
            for f in ("draws", "mean", "sd"):
                assert same(first[f], again[f])
    t = E.unifrac_rarefied_timing()
    assert all(t[k] > 0 for k in ("to_device", "draws", "embed", "pairs", "accumulate", "to_host")), t


@pytest.mark.gpu
@pytest.mark.parametrize("method, alpha", ALL)
def test_device_every_method(method, alpha):
    """every method on the small table at M = 1, the smallest N_j and one above it; without draws_out the same mean and sd"""
    _need_gpu()
    par, bl, nodes, counts = small()
    y = yard_of(par, bl, nodes, counts, method)
    for depth, reps in ((1, 5), (30, 2), (31, 5)):
        dev = both(par, bl, nodes, counts, depth, reps, 11, method, alpha, yard=y if reps == 2 else None)
        lean = call(par, bl, nodes, counts, method, alpha, depth=depth, reps=reps, seed=11)
        assert "draws" not in lean and same(lean["mean"], dev["mean"]) and same(lean["sd"], dev["sd"])
    nodes2, eq = table(len(par), 12, [40] * 5, 3)
    got = call(par, bl, nodes2, eq, method, alpha, depth=40, reps=3, seed=2)
    assert got["mean"].tobytes() == unifrac_of(par, bl, nodes2, eq, method, alpha).tobytes() and not got["sd"].any()


@pytest.mark.gpu
def test_device_seed_wrap_and_root_only():
    _need_gpu()
    par, bl, nodes, counts = small()
    both(par, bl, nodes, counts, 20, 3, M64 - 1, "weighted", None)
    got = E.unifrac_rarefied(np.array([[3.0, 5.0, 4.0]]), [0], par, bl, depth=3, reps=2, draws=True)
    assert not got["mean"].any() and not got["sd"].any() and not got["draws"].any()


@pytest.mark.gpu
def test_device_memory_refusal_and_one_resident_draw():
    _need_gpu()
    par, bl, nodes, counts = wide(65)
    sz = E.unifrac_rarefied_sizes(counts, nodes, par, bl, depth=60, reps=5, slab=32)
    need = lambda dc, wd: E.unifrac_rarefied_need(67, sz["n_kept"], sz["n_cell"], sz["n_entry"], sz["max_nnz"], sz["max_chunk"], sz["n_branch"], 32, dc, wd)   # noqa: E731
    full = E.unifrac_rarefied(counts, nodes, par, bl, depth=60, reps=5, seed=4, slab=32, draws=True)
    assert E.unifrac_rarefied_timing()["resident_draws"] == 5
    one = E.unifrac_rarefied(counts, nodes, par, bl, depth=60, reps=5, seed=4, slab=32, draws=True, mem_budget=need(2, True) - 1)
    assert E.unifrac_rarefied_timing()["resident_draws"] == 1                   # the budget admits one draw, not two
    for f in ("draws", "mean", "sd"):
        assert same(full[f], one[f])
    with pytest.raises(E.EngineError, match=r"1 resident draw\(s\) .* need %d bytes of device memory, the budget is %d bytes" % (need(1, False), need(1, False) - 1)) as ei:
        E.unifrac_rarefied(counts, nodes, par, bl, depth=60, reps=5, slab=32, mem_budget=need(1, False) - 1)
    assert "error -4" in str(ei.value)
    with pytest.raises(E.EngineError, match=r"3 resident draw\(s\) .* need %d bytes" % need(3, False)):
        E.unifrac_rarefied(counts, nodes, par, bl, depth=60, reps=5, slab=32, draw_chunk=3, mem_budget=need(3, False) - 1)
    assert same(E.unifrac_rarefied(counts, nodes, par, bl, depth=60, reps=5, seed=4, slab=32, mem_budget=need(1, False))["mean"], full["mean"])


@pytest.mark.gpu
def test_program_on_the_device(tmp_path, prog):
    _need_gpu()
    for method in ("weighted", "unweighted", "jaccard"):
        extra = [] if method in IDENT else ["--db", prog["db"]]
        args = [_bin(), prog["table"], "--method", method, "--rarefy", 31, "--reps", 5, "--seed", 9] + extra
        r = _run(args + ["-o", tmp_path / "dev.txt", "--sd-out", tmp_path / "dev_sd.txt", "--draw-chunk", 2, "--chunk", 64, "--mem", 1, "-v"])
        assert r.returncode == 0, r.stderr
        assert "2 draws resident at once" in r.stderr and "pair kernel" in r.stderr and "4 samples kept, 2 dropped" in r.stderr
        h = _run(args + ["-o", tmp_path / "host.txt", "--sd-out", tmp_path / "host_sd.txt", "--host"])
        assert h.returncode == 0, h.stderr
        assert (tmp_path / "dev.txt").read_text() == (tmp_path / "host.txt").read_text() and (tmp_path / "dev_sd.txt").read_text() == (tmp_path / "host_sd.txt").read_text()
