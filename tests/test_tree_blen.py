"""hmmufotu-amd-tree --ml-lengths: maximum-likelihood branch lengths on a fixed topology.

The yardstick is the restatement in this file, which shares no code with the library: Q from the model's parameters as the reference
defines it (JC69 and HKY85 files carry a beta that makes the mean rate 1; GTR is scaled by minus its trace, src/GTR.cpp:124-131,
which the library follows to place reads as the reference does, so a GTR length is in that unit), P(t) and its derivatives from numpy's eigendecomposition of Q, Felsenstein
pruning per column in float64 linear space with a scale per node and column, sums by math.fsum.  f_u, f_u' and f_u'' come from the
two partial likelihoods at the ends of the branch, i.e. pruning with the tree rooted at the branch, and each branch's one-dimensional
optimum from bisection on the restated f'.  A leaf without a symbol carries pi, as the reference's leaves do
(src/PhyloTreeUnrooted.h:1431-1437).

The bar of the scores: the deviation of f relative to |f|, of f' and f'' relative to the sum of the absolute values of their column
terms.  Measured over the cases of this file, the device's shapes included: 6.02e-13 on the host path (33 leaves, 257 columns) and
5.52e-13 on the device (MI355X; 33 leaves, 65 columns); four times the larger, 2.41e-12, rounded up to a power of two is
SCORE_BAR = 2^-38 = 3.64e-12.  The deviation of f alone stays below 3e-15; what f' and f'' lose they lose where a leaf's base differs
from its neighbourhood's on a short branch: L_j(t) is then of the order of t, both here and in the library a difference of spectral
terms of the order of 1.
"""
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
GOLD = os.path.join(ROOT, "tests", "golden", "tree_blen")
FASTA70 = os.path.join(REF, "70_otus.fasta.gz")
TAU = E.BLEN_TAU
EPS = 1e-5
SCORE_BAR = 2.0 ** -38
assert SCORE_BAR <= 1e-10 and TAU <= EPS / 100


def _bin(name="hmmufotu-amd-tree"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=600, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


def sm(name):
    return os.path.join(REF, "gg_97_otus_%s.sm" % name)


# ---- the restatement ----

def ref_Q(m):
    """the rate matrix of a model file as the reference builds it"""
    pi = np.asarray(m.pi, float)
    ti = lambda i, j: (i ^ j) == 2
    Q = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            if i == j:
                continue
            if m.name == "GTR":
                Q[i, j] = m.par.reshape(4, 4)[i, j] * pi[j]
            elif m.name == "HKY85":
                Q[i, j] = m.par[1] * pi[j] * (m.par[0] if ti(i, j) else 1.0)
            elif m.name == "JC69":
                Q[i, j] = 1.0 / 3
            else:
                raise ValueError(m.name)
    Q -= np.diag(Q.sum(1))
    if m.name == "GTR":
        Q /= -np.trace(Q)
    return Q


class RefModel:
    def __init__(self, m):
        self.pi = np.full(4, 0.25) if m.name == "JC69" else np.asarray(m.pi, float)
        self.Q = ref_Q(m)
        lam, V = np.linalg.eig(self.Q)
        self.lam, self.V, self.Vi = lam.real, V.real, np.linalg.inv(V.real)
        self.mean_rate = -float((self.pi * np.diag(self.Q)).sum())

    def P(self, t, order=0):
        if t == 0 and order == 0:
            return np.eye(4)
        return (self.V * (self.lam ** order * np.exp(self.lam * t))[None, :]) @ self.Vi


class RefTree:
    """pruning in linear space: msg [L][4] with its largest entry 1 and the logarithm of what was divided out"""

    def __init__(self, parent, seq, model):
        self.parent = np.asarray(parent); self.n = len(parent); self.m = model
        self.root = int(np.nonzero(self.parent < 0)[0][0])
        self.kids = [[] for _ in range(self.n)]
        for u in range(self.n):
            if self.parent[u] >= 0:
                self.kids[self.parent[u]].append(u)
        self.order = [self.root]
        for u in self.order:
            self.order += self.kids[u]
        self.L = seq.shape[1]
        self.leaf = {}
        for u in range(self.n):
            if not self.kids[u]:
                row = np.asarray(seq[u]).astype(int)
                x = np.where(row[:, None] >= 0, np.arange(4)[None, :] == row[:, None], self.m.pi[None, :]).astype(float)
                self.leaf[u] = x

    @staticmethod
    def _norm(x, s):
        mx = x.max(1)
        return x / mx[:, None], s + np.log(mx)

    def messages(self, blen):
        up = [None] * self.n; us = [None] * self.n; down = [None] * self.n; ds = [None] * self.n
        P = [self.m.P(blen[u]) if u != self.root else None for u in range(self.n)]
        for u in reversed(self.order):
            if not self.kids[u]:
                up[u], us[u] = self.leaf[u], np.zeros(self.L)
                continue
            x = np.ones((self.L, 4)); s = np.zeros(self.L)
            for c in self.kids[u]:
                x = x * (up[c] @ P[c].T); s = s + us[c]
            up[u], us[u] = self._norm(x, s)
        for u in self.order[1:]:
            p = self.parent[u]
            x = np.ones((self.L, 4)); s = np.zeros(self.L)
            if p != self.root:
                x = x * (down[p] @ P[p].T); s = s + ds[p]
            for c in self.kids[p]:
                if c != u:
                    x = x * (up[c] @ P[c].T); s = s + us[c]
            down[u], ds[u] = self._norm(x, s)
        self.up, self.us, self.down, self.ds = up, us, down, ds
        return self

    def loglik(self):
        r = self.root
        return math.fsum(np.log(self.up[r] @ self.m.pi) + self.us[r])

    def branch(self, u, t):
        """f, f', f'' of branch u at t and the sums of the absolute column terms of f' and f''"""
        x = self.up[u] * self.m.pi[None, :]; y = self.down[u]
        L0 = np.einsum("ja,ab,jb->j", x, self.m.P(t), y)
        L1 = np.einsum("ja,ab,jb->j", x, self.m.P(t, 1), y)
        L2 = np.einsum("ja,ab,jb->j", x, self.m.P(t, 2), y)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = L1 / L0; h = L2 / L0 - g * g
            f = math.fsum(np.log(L0) + self.us[u] + self.ds[u])
        return f, math.fsum(g), math.fsum(h), math.fsum(np.abs(g)), math.fsum(np.abs(h))

    def slope(self, u, t):
        return self.branch(u, t)[1]

    def optimum(self, u, lo, hi):
        """the maximiser of f_u on [lo, hi] by bisection on the restated f'"""
        if not self.slope(u, lo) > 0:
            return lo
        if not self.slope(u, hi) < 0:
            return hi
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if self.slope(u, mid) > 0:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)


# ---- the inputs ----

def random_tree(n_leaves, rng, four=True):
    """parent [n] in preorder from a bifurcating root 0; one node with four children when there are leaves enough"""
    kids = {}
    active = list(range(n_leaves)); nxt = n_leaves
    want4 = four and n_leaves >= 5
    while len(active) > 2:
        k = 4 if want4 and len(active) >= 5 and rng.random() < 0.5 else 2
        if want4 and len(active) == 5:
            k = 4
        if k == 4:
            want4 = False
        pick = [active.pop(int(rng.integers(len(active)))) for _ in range(k)]
        kids[nxt] = pick; active.append(nxt); nxt += 1
    kids[nxt] = active
    parent = []; ident = {}
    stack = [(nxt, -1)]
    while stack:
        v, p = stack.pop()
        ident[v] = len(parent); parent.append(p)
        for c in reversed(kids.get(v, [])):
            stack.append((c, ident[v]))
    return np.array(parent, np.int32)


class Case:
    pass


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def make_case(n_leaves, L, model, seed, random_leaf=False, max_len=10.0, min_len=0.0, star=False):
    rng = np.random.default_rng(seed)
    c = Case()
    c.name = "%s %d x %d seed %d" % (model, n_leaves, L, seed)
    c.min_len, c.max_len = min_len, max_len
    c.parent = np.array([-1] + [0] * n_leaves, np.int32) if star else random_tree(n_leaves, rng)
    n = len(c.parent)
    c.sm = synth.load_model(model)
    c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par)
    c.true = (np.full(n, 0.02) if star else rng.exponential(0.08, n) + 0.01)
    c.true[0] = 0.0
    seq = synth.evolve_sequences(c.parent, c.true, L, c.sm, np.ones(L), rng)
    kids = [[] for _ in range(n)]
    for u in range(1, n):
        kids[c.parent[u]].append(u)
    c.leaves = [u for u in range(n) if not kids[u]]
    seq[rng.random(seq.shape) < 0.05] = -2
    if L > 2:
        seq[:, 2] = -2                                         # one column without a symbol
    c.sisters = None
    if not star:
        for u in range(n):
            lv = [v for v in kids[u] if not kids[v]]
            if len(kids[u]) == 2 and len(lv) == 2 and u != 0:
                seq[lv[1]] = seq[lv[0]]; c.sisters = tuple(lv)
                break
    c.random = None
    if random_leaf:
        c.random = [u for u in c.leaves if not c.sisters or u not in c.sisters][-1]
        seq[c.random] = rng.integers(0, 4, L)
    for u in range(n):
        if kids[u]:
            seq[u] = -2
    c.seq = np.ascontiguousarray(seq, np.int8)
    c.start = np.where(c.parent >= 0, np.clip(c.true * rng.uniform(0.5, 1.5, n), 0.005, max_len * 0.9), 0.0)
    c.kids = kids
    c.ref = RefTree(c.parent, c.seq, RefModel(c.sm))
    return c


def cases():
    """a node with four children, a bifurcating root, identical sisters, 5 % gaps and a column of gaps in each; a leaf of random
    bases under max_len 2 in the second"""
    return cached("cases", lambda: [make_case(9, 200, "JC69", 1), make_case(12, 257, "HKY85", 2, random_leaf=True, max_len=2.0),
                                    make_case(7, 150, "GTR", 3)])


def score_points(c):
    """the current lengths and three other t per branch"""
    return [c.start, 0.5 * c.start + 0.003, 2.0 * c.start + 0.01, np.full(len(c.start), 0.37)]


def score_deviation(c, host, device=0):
    """the largest deviation of the library's scores from the restatement, f relative to |f|, f' and f'' relative to the sums of their
    absolute column terms"""
    ref = c.ref.messages(c.start)
    worst = 0.0
    for t in score_points(c):
        got = E.tree_branch_scores(c.parent, c.start, c.seq, c.md, t=np.where(c.parent >= 0, t, 0.0), host=host, device=device)
        for u in range(1, len(c.parent)):
            f, g, h, ag, ah = ref.branch(u, t[u])
            worst = max(worst, abs(got["f"][u] - f) / abs(f), abs(got["d1"][u] - g) / ag, abs(got["d2"][u] - h) / ah)
    return worst


# ---- the model and the pulley principle ----

@pytest.mark.parametrize("name", ["JC69", "HKY85", "GTR"])
def test_restated_model_is_the_librarys(name):
    m = synth.load_model(name)
    rm = RefModel(m)
    U, lam, U1 = E.model_spectral(E.model_desc(m.type_id, m.pi, m.par))
    for t in (0.0, 0.01, 0.3, 2.0):
        assert np.abs((U * np.exp(lam * t)[None, :]) @ U1 - rm.P(t)).max() <= 1e-14
    assert np.allclose(rm.pi @ rm.Q, 0, atol=1e-15)
    if name != "GTR":
        assert abs(rm.mean_rate - 1) <= 1e-12              # GTR: scaled by its trace, mean rate 0.2418


def test_pulley_every_branch_gives_the_tree_loglik():
    for c in cases():
        want = c.ref.messages(c.start).loglik()
        got = E.tree_branch_scores(c.parent, c.start, c.seq, c.md, host=True)
        f = got["f"][1:]
        assert np.abs(f - want).max() <= SCORE_BAR * abs(want), c.name
        assert np.abs(f - f[0]).max() <= SCORE_BAR * abs(want)
        for u in range(1, len(c.parent)):
            assert abs(c.ref.branch(u, c.start[u])[0] - want) <= 1e-12 * abs(want)
        r = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, max_rounds=1, host=True)
        assert abs(r["ll_start"] - want) <= SCORE_BAR * abs(want)
        assert got["f"][0] == 0 and got["d1"][0] == 0


def test_scores_against_the_restatement_host():
    worst = max(score_deviation(c, host=True) for c in cases())
    print("largest deviation of the host path's scores: %.3g" % worst)
    assert worst <= SCORE_BAR


# ---- the step ----

def check_step(c, got, blen):
    """property 3 for every branch; returns the kinds met"""
    ref = c.ref.messages(blen)
    kinds = set()
    assert got["n_capped"] == 0 and not got["capped"].any()
    for u in range(1, len(c.parent)):
        t = got["t_star"][u]
        assert c.min_len <= t <= c.max_len
        if t == c.min_len:
            kinds.add("min"); assert ref.slope(u, c.min_len) <= 0, (c.name, u)
        elif t == c.max_len:
            kinds.add("max"); assert ref.slope(u, c.max_len) >= 0, (c.name, u)
        else:
            kinds.add("inner")
            assert ref.slope(u, max(t - 2 * TAU, c.min_len)) >= 0 and ref.slope(u, min(t + 2 * TAU, c.max_len)) <= 0, (c.name, u, t)
    return kinds


def test_step_finds_each_branchs_optimum_host():
    kinds = set()
    for c in cases():
        got = E.tree_branch_step(c.parent, c.start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, host=True)
        kinds |= check_step(c, got, c.start)
        if c.sisters:
            assert got["t_star"][c.sisters[0]] == c.min_len or got["t_star"][c.sisters[1]] == c.min_len
        if c.random is not None:
            ref = c.ref.messages(c.start)
            f, g, h, ag, ah = ref.branch(c.random, c.max_len)
            assert g / ag > 100 * SCORE_BAR                       # the optimum of the random leaf lies beyond max_len for certain
            assert got["t_star"][c.random] == c.max_len
        sc = E.tree_branch_scores(c.parent, c.start, c.seq, c.md, host=True)
        assert np.array_equal(sc["f"], got["f"]) and np.array_equal(sc["d1"], got["d1"]) and np.array_equal(sc["d2"], got["d2"])
    assert kinds == {"min", "max", "inner"}


# ---- the rounds ----

def check_run(c, r, start, need_converged=False):
    lls = [r["ll_start"]] + [x["ll"] for x in r["rounds"]]
    assert all(b > a for a, b in zip(lls, lls[1:])), lls
    assert r["ll_final"] == lls[-1] and r["n_capped"] == 0
    blen = r["blen"]
    assert ((blen[1:] >= c.min_len) & (blen[1:] <= c.max_len)).all()
    ref = c.ref.messages(blen)
    want = ref.loglik()
    assert abs(r["ll_final"] - want) <= SCORE_BAR * abs(want)
    if need_converged:
        assert r["stop"] == "converged", (r["stop"], len(r["rounds"]), r["rounds"][-1])
    if r["stop"] == "converged":
        for u in range(1, len(c.parent)):
            assert abs(blen[u] - ref.optimum(u, c.min_len, c.max_len)) <= 2 * EPS, (c.name, u)


def test_rounds_from_lengths_of_a_tenth_host():
    for c in cases():
        start = np.where(c.parent >= 0, 0.1, 0.0)
        r = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, max_rounds=1000, host=True)
        print(c.name, r["stop"], len(r["rounds"]), r["ll_start"], r["ll_final"])
        check_run(c, r, start, need_converged=True)
        r50 = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, host=True)
        assert r50["rounds"] == r["rounds"][:50]               # the default of 50 rounds is a prefix of the longer run
        big = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, max_rounds=1000, host=True, mem_budget=1 << 40)
        assert np.array_equal(big["blen"], r["blen"]) and big["rounds"] == r["rounds"]     # no dependence on the memory budget


def nj_case():
    """rows evolved down a random tree, their neighbour-joining tree (host path) as the start"""
    def make():
        c0 = make_case(10, 300, "HKY85", 7)
        rows = c0.seq[c0.leaves]
        names = ["s%d" % i for i in range(len(rows))]
        D, _ = E.msa_distances(rows, "HKY85", c0.sm.pi, host=True)
        text = E.nj_newick(names, E.nj(D, host=True))
        t = E.newick_parse(text)
        c = Case()
        c.name = "NJ start"; c.min_len, c.max_len = 0.0, 10.0
        c.parent = np.asarray(t["parent"], np.int32); c.sm, c.md = c0.sm, c0.md
        n = len(c.parent)
        c.seq = np.full((n, rows.shape[1]), -2, np.int8)
        for u in range(n):
            if t["names"][u]:
                c.seq[u] = rows[names.index(t["names"][u])]
        c.start = np.clip(np.asarray(t["blen"], float), 0.0, 10.0)
        c.text = text
        c.ref = RefTree(c.parent, c.seq, RefModel(c.sm))
        return c
    return cached("nj", make)


def test_rounds_from_the_nj_lengths_host():
    c = nj_case()
    r = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, max_rounds=1000, host=True)
    print(c.name, r["stop"], len(r["rounds"]), r["ll_start"], r["ll_final"])
    assert r["rounds"], "the joins' lengths are least-squares fits: the likelihood must rise"
    check_run(c, r, c.start)


def star_case():
    return cached("star", lambda: make_case(6, 120, "JC69", 11, star=True))


def test_a_full_step_is_rejected_on_a_star_started_far_off():
    """short true branches, all lengths started at 2: every branch's own optimum is at 0 while the others are long, and all of
    them at 0 at once has likelihood 0"""
    c = star_case()
    start = np.where(c.parent >= 0, 2.0, 0.0)
    r = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, max_rounds=1000, host=True)
    print([(x["s"], x["delta"]) for x in r["rounds"][:5]], r["stop"], len(r["rounds"]))
    assert any(x["s"] < 1 for x in r["rounds"])
    check_run(c, r, start)


# ---- refusals of the entries ----

def test_entries_refuse_what_the_header_says():
    c = cases()[0]
    dg = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.4, 1.0, 2.5])
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_branch_scores(c.parent, c.start, c.seq, dg, host=True)
    for kw in (dict(eps=0.0), dict(eps=1e-7), dict(max_len=0.0), dict(min_len=-1.0), dict(min_len=2.0, max_len=1.0), dict(max_rounds=0)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True, **kw)
    bad = c.start.copy(); bad[3] = -0.1
    with pytest.raises(E.EngineError, match="error -1: .*node 3"):
        E.tree_branch_step(c.parent, bad, c.seq, c.md, host=True)
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need (\d+) bytes .*budget is 1048576 bytes") as ei:
        E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True, mem_budget=1 << 20)
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) == E.blen_need(n, L) >= 65 * n * L + (1 << 20)
    assert E.blen_need(10, E.BLEN_LDS_COLS + 1) - E.blen_need(10, E.BLEN_LDS_COLS) == 10 * (65 + 24 * (E.BLEN_LDS_COLS + 1)) + 8


# ---- the program ----

def write_fasta(path, names, rows):
    with open(path, "w") as f:
        for nm, r in zip(names, rows):
            f.write(">%s\n%s\n" % (nm, "".join("ACGT"[x] if x >= 0 else "-" for x in r)))


def to_newick(parent, kids, names, blen, u=0):
    lab = names[u]
    if re.search(r"[\s()\[\]':;,]", lab):
        lab = "'%s'" % lab
    s = ("(" + ",".join(to_newick(parent, kids, names, blen, v) for v in kids[u]) + ")" if kids[u] else "") + lab
    return s + (":%.6g" % blen[u] if parent[u] >= 0 else "")


def program_case(tmp_path):
    """a FASTA file and a start tree with names that need quotes, an inner name and children in a fixed order"""
    c = cases()[2]
    names = [""] * len(c.parent)
    for i, u in enumerate(c.leaves):
        names[u] = ["a(1)", "b:2", "c,3", "d;4", "e[5]", "plain6", "g_7"][i]
    names[c.parent[c.leaves[0]]] = "clade:x"
    rows = c.seq[c.leaves]
    keep = (rows >= 0).any(axis=0)
    fa = tmp_path / "in.fasta"
    write_fasta(fa, [names[u] for u in c.leaves][::-1], rows[::-1][:, keep])
    tree = tmp_path / "start.tree"
    tree.write_text(to_newick(c.parent, c.kids, names, c.start) + ";\n")
    return c, names, fa, tree, keep


def same_topology(a, b):
    return (np.array_equal(a["parent"], b["parent"]) and list(a["names"]) == list(b["names"])
            and np.array_equal(a["child_off"], b["child_off"]) and np.array_equal(a["child_idx"], b["child_idx"]))


def test_program_start_tree_round_trip_and_log(tmp_path):
    c, names, fa, tree, keep = program_case(tmp_path)
    out, log = tmp_path / "out.tree", tmp_path / "ml.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("GTR"), "--ml-lengths", "--start-tree", tree, "-o", out, "--ml-log", log, "--ml-rounds", 200, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"log-likelihood -\d+\.\d+ -> -\d+\.\d+ in \d+ round\(s\), stop: converged", r.stderr), r.stderr
    text = out.read_text()
    a, b = E.newick_parse(tree.read_text()), E.newick_parse(text)
    assert same_topology(a, b)
    for q in ("'a(1)'", "'b:2'", "'c,3'", "'d;4'", "'e[5]'", "'clade:x'", "plain6:", "g_7:"):
        assert q in text
    assert text.endswith(";\n")
    # the lengths are, bit for bit, those of the library on the same tree, which is what 17 significant digits are for: the node ids of
    # the parser differ from the case's, so go through the names
    nb = np.asarray(b["blen"])
    want = E.tree_optimize_lengths(c.parent, np.array([float("%.6g" % x) for x in c.start]), c.seq[:, keep], c.md, max_rounds=1000, host=True)
    by_name = {names[u]: want["blen"][u] for u in range(len(c.parent)) if names[u]}
    for i, nm in enumerate(b["names"]):
        if nm:
            assert nb[i] == by_name[nm]
    # the log: a header, the start, one line per accepted round with a rising ll, the reason
    lines = log.read_text().splitlines()
    assert lines[0] == "round\tll\ts\tdelta\tcapped" and lines[-1] == "# stop: converged"
    rows = [x.split("\t") for x in lines[1:-1]]
    assert [int(x[0]) for x in rows] == list(range(len(rows))) and rows[0][2:] == ["0", "0", "0"]
    assert len(rows) - 1 == len(want["rounds"])
    ll = [float(x[1]) for x in rows]
    assert all(q > p for p, q in zip(ll, ll[1:])) and ll[-1] == want["ll_final"]
    assert all(float(x[2]) in (1.0, 0.5, 0.25, 0.125) or float(x[2]) < 0.125 for x in rows[1:]) and all(int(x[4]) == 0 for x in rows)


def test_program_keeps_the_topology_of_the_joins(tmp_path):
    """with and without --ml-lengths on the same alignment: the same distances, the same topology and names, other lengths"""
    c, names, fa, tree, keep = program_case(tmp_path)
    outs = []
    for flags in ([], ["--ml-lengths"]):
        o, d = tmp_path / ("t%d.tree" % len(flags)), tmp_path / ("d%d.txt" % len(flags))
        r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "-o", o, "--dist-out", d] + flags)
        assert r.returncode == 0, r.stderr
        outs.append((o.read_text(), d.read_text()))
    assert outs[0][1] == outs[1][1]
    a, b = E.newick_parse(outs[0][0]), E.newick_parse(outs[1][0])
    assert same_topology(a, b) and not np.array_equal(a["blen"], b["blen"])


@pytest.mark.parametrize("model", ["JC69", "GTR"])
def test_program_without_the_flag_writes_what_it_wrote_before(tmp_path, model):
    """70_otus on the host path, against the file the parent commit wrote"""
    out = tmp_path / "nj.tree"
    r = _run([_bin(), FASTA70, "--host", "-o", out] + ([] if model == "JC69" else ["-sm", sm(model)]))
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLD, "70_otus_nj_host_%s.tree" % model), "rb") as f:
        assert out.read_bytes() == f.read()


def test_program_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, names, fa, tree, keep = program_case(tmp_path)
    leafs = [names[u] for u in c.leaves]
    t = tree.read_text()
    missing = tmp_path / "missing.tree"; missing.write_text(t.replace("plain6", "other6"))
    dup = tmp_path / "dup.tree"; dup.write_text(t.replace("plain6", "g_7"))
    more = tmp_path / "more.fasta"                              # every leaf of the tree is a sequence, and one sequence is no leaf
    write_fasta(more, leafs + ["extra"], np.vstack([c.seq[c.leaves], c.seq[c.leaves[:1]]]))
    ml = ["-sm", sm("GTR"), "--ml-lengths"]
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa, "--ml-lengths"], "-sm is required"),
                      ([fa, "-sm", sm("GTR"), "--start-tree", tree], "goes with --ml-lengths"),
                      ([fa] + ml + ["--start-tree", missing], "Unmatched MSA and Tree: leaf 'other6' .* is no sequence of the MSA"),
                      ([more] + ml + ["--start-tree", tree], "Unmatched MSA and Tree: sequence 'extra' is no leaf of"),
                      ([fa] + ml + ["--start-tree", dup], "Non-unique leaf name"),
                      ([fa] + ml + ["--ml-eps", "0"], "--ml-eps"), ([fa] + ml + ["--ml-eps", "-1"], "--ml-eps"),
                      ([fa] + ml + ["--max-len", "0"], "--max-len"), ([fa] + ml + ["--min-len", "-0.5"], "--min-len"),
                      ([fa] + ml + ["--min-len", "3", "--max-len", "2"], "below --max-len"),
                      ([fa] + ml + ["--ml-rounds", "0"], "--ml-rounds"),
                      ([fa] + ml + ["--mem", "0.0001"], r"need \d+ bytes .* --mem allows 100000 bytes"),
                      ([fa] + ml + ["--mem", "0.0001", "--start-tree", tree], r"need \d+ bytes .* --mem allows 100000 bytes")):
        r = _run([_bin()] + args + ["-o", tmp_path / "o.tree", "--ml-log", tmp_path / "o.log"] if "--ml-lengths" in args else [_bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


# ---- the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_blen_host.cpp (the checks, the host sweep, the step and the round loop; no HIP headers) with tests/san/blen_driver.cpp under
    AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "blen_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "blen_driver.cpp"), os.path.join(CSRC, "hu_blen_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "12 cases" in r.stdout


# ---- the device ----

def device_case(n_leaves, L):
    return cached(("dev", n_leaves, L), lambda: make_case(n_leaves, L, ("JC69", "HKY85", "GTR")[(n_leaves + L) % 3], 100 * n_leaves + L,
                                                          random_leaf=n_leaves >= 5, max_len=2.0 if n_leaves >= 5 else 10.0))


DEVICE_SHAPES = [(3, 1), (4, 63), (5, 64), (33, 65), (130, 255), (5, 256), (33, 257), (130, 1000), (4, 1000), (5, E.BLEN_LDS_COLS), (5, E.BLEN_LDS_COLS + 1)]


def step_score_deviation(c, got):
    """f against the restatement relative to |f|, f' and f'' relative to the sums of their absolute column terms; a sum that is exactly 0
    (a single column whose term vanishes) has no scale, and that one quantity of that branch is left out"""
    ref = c.ref.messages(c.start)
    worst = 0.0
    for u in range(1, len(c.parent)):
        f, g, h, ag, ah = ref.branch(u, c.start[u])
        for have, want, scale in ((got["f"][u], f, abs(f)), (got["d1"][u], g, ag), (got["d2"][u], h, ah)):
            if scale != 0:
                worst = max(worst, abs(have - want) / scale)
    return worst


def test_host_scores_on_the_devices_shapes():
    """the host path is the device tests' measure of t*, so it is held to the restatement on their inputs too"""
    worst = 0.0
    for n_leaves, L in DEVICE_SHAPES:
        if n_leaves * L <= 40000:
            c = device_case(n_leaves, L)
            worst = max(worst, step_score_deviation(c, E.tree_branch_step(c.parent, c.start, c.seq, c.md, host=True, min_len=c.min_len, max_len=c.max_len)))
    print("largest deviation of the host path's scores on the device's shapes: %.3g" % worst)
    assert worst <= SCORE_BAR


@pytest.mark.gpu
def test_scores_against_the_restatement_device():
    _need_gpu()
    worst = max(score_deviation(c, host=False) for c in cases())
    print("largest deviation of the device's scores: %.3g" % worst)
    assert worst <= SCORE_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L):
    """the edges of a thread's stride (256 columns) and of a wave, one column, and the column counts on either side of the switch
    from ratios in LDS to ratios in global memory: t* within 2 tau of the host path's, the scores under the bar, the same bits twice"""
    _need_gpu()
    c = device_case(n_leaves, L)
    kw = dict(min_len=c.min_len, max_len=c.max_len)
    host = E.tree_branch_step(c.parent, c.start, c.seq, c.md, host=True, **kw)
    dev = E.tree_branch_step(c.parent, c.start, c.seq, c.md, **kw)
    again = E.tree_branch_step(c.parent, c.start, c.seq, c.md, **kw)
    for k in ("t_star", "f", "d1", "d2", "capped"):
        assert np.array_equal(dev[k], again[k]), k
    assert dev["n_capped"] == 0 and host["n_capped"] == 0
    gap = np.abs(dev["t_star"] - host["t_star"]).max()
    worst = step_score_deviation(c, dev)
    print("n %d L %d: largest |t* device - t* host| %.3g, largest score deviation %.3g" % (n_leaves, L, gap, worst))
    assert gap <= 2 * TAU and worst <= SCORE_BAR
    if L >= 63 and n_leaves <= 33:
        check_step(c, dev, c.start)


@pytest.mark.gpu
def test_rounds_on_the_device():
    _need_gpu()
    for c in cases() + [star_case()]:
        start = np.where(c.parent >= 0, 2.0 if c is star_case() else 0.1, 0.0)
        kw = dict(min_len=c.min_len, max_len=c.max_len, max_rounds=1000)
        r = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, **kw)
        check_run(c, r, start, need_converged=c is not star_case())
        h = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, host=True, **kw)
        assert np.abs(r["blen"] - h["blen"]).max() <= 2 * EPS and abs(r["ll_final"] - h["ll_final"]) <= SCORE_BAR * abs(h["ll_final"])
        if c is star_case():
            assert any(x["s"] < 1 for x in r["rounds"])
        big = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, mem_budget=1 << 40, **kw)
        assert np.array_equal(big["blen"], r["blen"])


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    _need_gpu()
    c = cases()[0]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.blen_need(n, L)):
        E.tree_branch_step(c.parent, c.start, c.seq, c.md, mem_budget=1 << 20)


@pytest.mark.gpu
def test_tree_ml_lengths_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree --ml-lengths -> hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm on 70_otus: a database of 125 leaves whose
    tree has the topology and the names of the run without the flag"""
    _need_gpu()
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "-o", "nj.tree", "--dist-out", "nj.dist"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "--ml-lengths", "-o", "ml.tree", "--dist-out", "ml.dist", "--ml-log", "ml.log", "-v"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Branch lengths fitted" in r.stderr
    assert (tmp_path / "nj.dist").read_text() == (tmp_path / "ml.dist").read_text()
    a, b = E.newick_parse((tmp_path / "nj.tree").read_text()), E.newick_parse((tmp_path / "ml.tree").read_text())
    assert same_topology(a, b) and not np.array_equal(a["blen"], b["blen"])
    ll = [float(x.split("\t")[1]) for x in (tmp_path / "ml.log").read_text().splitlines()[1:-1]]
    assert len(ll) > 1 and all(q > p for p, q in zip(ll, ll[1:]))
    r = _run([_bin("hmmufotu-amd-train-sm"), FASTA70, "ml.tree", "-o", "ml.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), FASTA70, "ml.tree", "--no-hmm", "-sm", "ml.sm", "-n", "mldb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "mldb.ptu"))
    par = db["parent"]
    assert db["n_nodes"] - len(set(int(p) for p in par if p >= 0)) == 125
