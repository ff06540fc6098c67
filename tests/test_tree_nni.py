"""hmmufotu-amd-tree --ml-lengths --nni: a hill climb over nearest-neighbour interchanges.

The yardstick is a restatement in this file that shares no code with the library.  It takes the model (RefModel) and the pruning in
float64 linear space with a scale per node and math.fsum (RefTree) from tests/test_tree_blen.py, names the eligible edges and their
subtrees A, B, C, D by the rules of the issue, REARRANGES the tree's parent array for an arrangement, prunes the rearranged tree, roots
it at the central edge and takes that edge's f, f' and, by bisection on f', its optimum.  An arrangement's score is therefore held
against a tree that was really rearranged, not against the nine-ratio formula under test.

The bar of f^q(t*), relative to |f|: measured over the cases of this file, the device's shapes included, the largest deviation is
8.41e-15 on the host path (HOST_WORST) and 1.58e-15 on the device (DEVICE_WORST; MI355X, 33 leaves x 65 columns); four times the larger,
3.4e-14, rounded up to a power of two is F_BAR = 2^-44 = 5.7e-14, far below the 1e-10 above which a formula would be wrong.  t* is
held as the branch-length fit's step is: the restated slope changes sign within 2 HU_BLEN_TAU of it, or the end of the interval is
justified.
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
from test_tree_blen import RefModel, RefTree, ref_Q, random_tree, sm, to_newick, write_fasta, SCORE_BAR  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70 = os.path.join(REF, "70_otus.fasta.gz")
TAU = E.BLEN_TAU
MIN_GAIN = 1e-3
HOST_WORST = 8.41e-15       # measured: the host path, cases() and the device's shapes (its serial sums over up to 1,451 columns)
DEVICE_WORST = 1.58e-15     # measured: MI355X, 33 leaves x 65 columns; 1.30e-15 over cases()
F_BAR = 2.0 ** -44          # 4 x 8.41e-15 = 3.4e-14, rounded up to a power of two: 5.7e-14
assert F_BAR <= 1e-10


def _bin(name="hmmufotu-amd-tree"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=600, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the restatement: edges, rearranged trees, scores ----

def kids_of(parent):
    kids = [[] for _ in parent]
    for u, p in enumerate(parent):
        if p >= 0:
            kids[p].append(u)
    return kids


def edge_parts(parent, u):
    """kind, A, B, C, D, s of the edge above u by the three rooted cases, or a reason why it is not scored"""
    parent = np.asarray(parent); kids = kids_of(parent)
    root = int(np.nonzero(parent < 0)[0][0])
    p = int(parent[u])
    if u == root or not kids[u]:
        return None
    if p != root:
        if len(kids[u]) != 2 or len(kids[p]) != 2:
            return "polytomy"
        A, B = sorted(kids[u])
        return dict(kind="inner", u=u, A=A, B=B, C=[v for v in kids[p] if v != u][0], D=None, s=None, p=p)
    if len(kids[p]) >= 3:
        if len(kids[u]) != 2 or len(kids[p]) != 3:
            return "polytomy"
        A, B = sorted(kids[u]); C, D = sorted(v for v in kids[p] if v != u)
        return dict(kind="root3", u=u, A=A, B=B, C=C, D=D, s=None, p=p)
    if len(kids[p]) == 2:
        s = [v for v in kids[p] if v != u][0]
        if not kids[s] or u > s:
            return None                                        # a leaf edge, or scored from s
        if len(kids[u]) != 2 or len(kids[s]) != 2:
            return "polytomy"
        A, B = sorted(kids[u]); C, D = sorted(kids[s])
        return dict(kind="root2", u=u, A=A, B=B, C=C, D=D, s=s, p=p)
    return None


def eligible(parent):
    out, skipped = [], 0
    for u in range(len(parent)):
        e = edge_parts(parent, u)
        if e == "polytomy":
            skipped += 1
        elif e is not None:
            out.append(e)
    return out, skipped


def rearranged(parent, blen, e, q, t=None):
    """the arrays after arrangement q of edge e: B <-> C (1) or A <-> C (2); the central edge at t when given"""
    par = np.array(parent, np.int32); bl = np.array(blen, float)
    if q:
        X = e["B"] if q == 1 else e["A"]
        par[X] = parent[e["C"]]; par[e["C"]] = e["u"]
    if t is not None:
        if e["kind"] == "root2":
            tot = bl[e["u"]] + bl[e["s"]]
            bu = t * (bl[e["u"]] / tot) if tot > 0 else 0.5 * t
            bl[e["u"]] = bu; bl[e["s"]] = t - bu
        else:
            bl[e["u"]] = t
    return par, bl


class Arrangement:
    """the rearranged tree pruned and rooted at the central edge: f(t), its slope and its optimum"""

    def __init__(self, c, blen, e, q):
        par, bl = rearranged(c.parent, blen, e, q)
        if e["kind"] == "root2":
            bl[e["s"]] = 0.0                                    # the whole edge lies above u: branch(u, t) is rooted at it
        self.ref = RefTree(par, c.seq, c.rm).messages(bl)
        self.u = e["u"]

    def f(self, t):
        return self.ref.branch(self.u, t)[0]

    def slope(self, t):
        return self.ref.slope(self.u, t)

    def optimum(self, lo, hi):
        return self.ref.optimum(self.u, lo, hi)


def check_t_star(a, t, lo, hi, what):
    assert lo <= t <= hi, what
    if t == lo:
        assert a.slope(lo) <= 0, what
        return "min"
    if t == hi:
        assert a.slope(hi) >= 0, what
        return "max"
    assert a.slope(max(t - 2 * TAU, lo)) >= 0 and a.slope(min(t + 2 * TAU, hi)) <= 0, what
    return "inner"


def central(blen, e):
    return blen[e["u"]] + (blen[e["s"]] if e["kind"] == "root2" else 0.0)


def check_scores(c, got, blen=None):
    """every eligible edge and arrangement against the restatement; returns the largest deviation of f, the kinds of edges and of optima"""
    blen = c.start if blen is None else blen
    want, skipped = eligible(c.parent)
    assert [e["u"] for e in want] == list(got["edge_node"]) and got["skipped"] == skipped, c.name
    worst, kinds, ends = 0.0, set(), set()
    for i, e in enumerate(want):
        kinds.add(e["kind"])
        for q in range(3):
            a = Arrangement(c, blen, e, q)
            t = got["t_star"][i][q]
            ends.add(check_t_star(a, t, c.min_len, c.max_len, (c.name, e["u"], q, t)))
            f = a.f(t)
            worst = max(worst, abs(got["f"][i][q] - f) / abs(f))
            if q == 0:
                f0 = a.f(central(blen, e))
                worst = max(worst, abs(got["f0_at_blen"][i] - f0) / abs(f0))
    return worst, kinds, ends


# ---- the inputs ----

def build_tree(n_leaves, rng, top=2, leaf_child=False):
    """parent [n] in preorder from root 0 with `top` children; leaf_child: one of them is a leaf.  A bifurcating root without
    leaf_child has two inner children"""
    while True:
        kids = {}
        active = list(range(n_leaves)); nxt = n_leaves
        hold = [active.pop()] if leaf_child else []
        while len(active) > top - len(hold):
            pick = [active.pop(int(rng.integers(len(active)))) for _ in range(2)]
            kids[nxt] = pick; active.append(nxt); nxt += 1
        kids[nxt] = active + hold
        if top == 3 or leaf_child or all(v in kids for v in active):
            break
    parent = []; ident = {}
    stack = [(nxt, -1)]
    while stack:
        v, p = stack.pop()
        ident[v] = len(parent); parent.append(p)
        for ch in reversed(kids.get(v, [])):
            stack.append((ch, ident[v]))
    return np.array(parent, np.int32)


class Case:
    pass


def make_case(parent, L, model, seed, random_leaf=False, max_len=10.0, gap_row=False):
    rng = np.random.default_rng(seed)
    c = Case()
    c.parent = np.asarray(parent, np.int32)
    n = len(c.parent)
    c.kids = kids_of(c.parent)
    c.leaves = [u for u in range(n) if not c.kids[u]]
    c.name = "%s %d leaves x %d seed %d" % (model, len(c.leaves), L, seed)
    c.min_len, c.max_len = 0.0, max_len
    c.sm = synth.load_model(model)
    c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par)
    c.rm = RefModel(c.sm)
    c.true = rng.exponential(0.08, n) + 0.01
    c.true[0] = 0.0
    seq = synth.evolve_sequences(c.parent, c.true, L, c.sm, np.ones(L), rng)
    seq[rng.random(seq.shape) < 0.05] = -2                     # rows with gaps
    if L > 2:
        seq[:, 2] = -2                                         # one column without a symbol
    c.random = None
    if random_leaf:
        c.random = c.leaves[-1]
        seq[c.random] = rng.integers(0, 4, L)
    if gap_row:
        seq[c.leaves[0]] = -2                                  # a leaf row of gaps only
    for u in range(n):
        if c.kids[u]:
            seq[u] = -2
    c.seq = np.ascontiguousarray(seq, np.int8)
    c.start = np.where(c.parent >= 0, np.clip(c.true * rng.uniform(0.5, 1.5, n), 0.005, max_len * 0.9), 0.0)
    if c.random is not None:
        c.start[c.random] = max_len                            # the leaf of random bases sits on a branch at max_len
    return c


POLY5 = np.array([-1, 0, 1, 2, 2, 1, 1, 0], np.int32)         # root {1, leaf 7}, 1 = {2, leaf 5, leaf 6}, 2 = {leaf 3, leaf 4}
STAR3 = np.array([-1, 0, 0, 0], np.int32)


def cases():
    """4, 6, 12 and 33 leaves under the three models: a trifurcating top node, a bifurcating root with two inner children and with a
    leaf child, a node with four children (random_tree), 5 % gaps and a column of gaps in each, a leaf row of gaps only, a leaf of
    random bases on a branch at max_len"""
    def make():
        r = np.random.default_rng
        return [make_case(build_tree(4, r(1), top=2), 60, "JC69", 1),
                make_case(build_tree(4, r(2), top=3), 61, "HKY85", 2, gap_row=True),
                make_case(build_tree(6, r(3), top=2, leaf_child=True), 70, "GTR", 3),
                make_case(build_tree(6, r(4), top=2), 64, "JC69", 4),
                make_case(build_tree(12, r(5), top=3), 130, "HKY85", 5, random_leaf=True, max_len=2.0),
                make_case(random_tree(12, r(6)), 90, "JC69", 6, gap_row=True),
                make_case(random_tree(33, r(7)), 101, "GTR", 7, random_leaf=True, max_len=2.0)]
    return cached("cases", make)


def poly_case():
    return cached("poly", lambda: make_case(POLY5, 40, "HKY85", 8))


def star_case():
    return cached("star3", lambda: make_case(STAR3, 40, "GTR", 9))


def scores(c, host, **kw):
    return E.tree_nni_scores(c.parent, c.start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, host=host, **kw)


def tree_loglik_host(parent, blen, c):
    """hu_tree_loglik's value on the host path: the start of a fit"""
    return E.tree_optimize_lengths(parent, blen, c.seq, c.md, max_rounds=1, host=True)["ll_start"]


# ---- 1. the pulley principle ----

def test_pulley_every_eligible_edge_gives_the_tree_loglik():
    met = 0
    for c in cases():
        got = scores(c, host=True)
        want = tree_loglik_host(c.parent, c.start, c)
        assert abs(RefTree(c.parent, c.seq, c.rm).messages(c.start).loglik() - want) <= SCORE_BAR * abs(want)
        assert len(got["f0_at_blen"]) > 0 or len(c.leaves) == 6
        assert np.all(np.abs(got["f0_at_blen"] - want) <= SCORE_BAR * abs(want)), c.name
        met += len(got["f0_at_blen"])
    assert met >= 20


# ---- 2. scores and optima against the restatement ----

def run_restatement(host):
    worst, kinds, ends = 0.0, set(), set()
    for c in cases():
        w, k, e = check_scores(c, scores(c, host=host))
        print("%s: largest deviation of f %.3g" % (c.name, w))
        worst = max(worst, w); kinds |= k; ends |= e
    assert kinds == {"inner", "root3", "root2"}
    assert ends == {"min", "max", "inner"} or ends == {"max", "inner"} or ends == {"min", "inner"}, ends
    # the bifurcating root with a leaf child: its edge is no eligible one
    c = cases()[2]
    assert all(e["kind"] == "inner" for e in eligible(c.parent)[0])
    # a polytomy: its edge is skipped and counted; three leaves: nothing to score, a success
    got = scores(poly_case(), host=host)
    assert len(got["edge_node"]) == 0 and got["skipped"] == 1 and got["t_star"].shape == (0, 3)
    got = scores(star_case(), host=host)
    assert len(got["edge_node"]) == 0 and got["skipped"] == 0 and got["f"].shape == (0, 3)
    assert any(c.random is not None for c in cases()) and eligible(cases()[6].parent)[1] > 0
    return worst


def test_scores_and_optima_against_the_restatement_host():
    """measured: HOST_WORST"""
    worst = run_restatement(host=True)
    print("largest deviation of the host path's f: %.3g" % worst)
    assert worst <= F_BAR


# ---- 3. apply ----

def bipartitions(parent, blen, names):
    """{the side of an edge without the first leaf: its length}; the two branches at a bifurcating root are one edge"""
    kids = kids_of(parent); n = len(parent)
    leaves = sorted(names[u] for u in range(n) if not kids[u])
    under = [None] * n
    order = [int(np.nonzero(np.asarray(parent) < 0)[0][0])]
    for u in order:
        order += kids[u]
    out = {}
    for u in reversed(order):
        under[u] = frozenset([names[u]]) if not kids[u] else frozenset().union(*[under[v] for v in kids[u]])
        if parent[u] >= 0:
            side = under[u] if leaves[0] not in under[u] else frozenset(leaves) - under[u]
            if side:
                out[side] = out.get(side, 0.0) + blen[u]
    return out


def is_tree(parent, like):
    parent = np.asarray(parent)
    if (parent < 0).sum() != 1:
        return False
    kids = kids_of(parent)
    order = [int(np.nonzero(parent < 0)[0][0])]
    for u in order:
        order += kids[u]
    return sorted(order) == list(range(len(parent))) and [len(k) for k in kids] == [len(k) for k in kids_of(like)]


def test_apply_gives_the_predicted_loglik_and_its_inverse_restores():
    exact = 0
    for c in cases()[:6]:
        got = scores(c, host=True)
        names = ["n%d" % u for u in range(len(c.parent))]
        before = bipartitions(c.parent, c.start, names)
        for i, e in enumerate(eligible(c.parent)[0]):
            for q in (1, 2):
                t = got["t_star"][i][q]
                r = E.tree_nni_apply(c.parent, c.start, e["u"], q, t)
                par, bl = rearranged(c.parent, c.start, e, q, t)
                assert np.array_equal(r["parent"], par) and np.allclose(r["blen"], bl, rtol=1e-15, atol=0)
                assert is_tree(r["parent"], c.parent)
                ll = tree_loglik_host(r["parent"], r["blen"], c)
                assert abs(ll - got["f"][i][q]) <= F_BAR * abs(ll), (c.name, e["u"], q)
                # the Newick writer: the same bipartitions and lengths after a round trip through the parser
                text = E.newick_from_arrays(r["parent"], r["child_off"], r["child_idx"], names, r["blen"])
                back = E.newick_parse(text)
                assert back["names"][0] == names[int(np.nonzero(c.parent < 0)[0][0])]            # the same top node
                a, b = bipartitions(r["parent"], r["blen"], names), bipartitions(back["parent"], back["blen"], back["names"])
                assert a.keys() == b.keys() and all(abs(a[k] - b[k]) <= 1e-15 * max(a[k], 1e-300) * 4 for k in a)
                assert a.keys() != before.keys()
                # the inverse: the moved subtree and what took its place change back
                e2 = edge_parts(r["parent"], e["u"]); moved = e["B"] if q == 1 else e["A"]
                if e2["C"] == moved:
                    q2 = 1 if e2["B"] == e["C"] else 2
                else:                                          # the other side's smaller subtree is another one: the same unrooted tree by the opposite pair
                    q2 = 1 if e2["A"] == e["C"] else 2
                inv = E.tree_nni_apply(r["parent"], r["blen"], e["u"], q2, central(c.start, e), r["child_off"], r["child_idx"])
                z = bipartitions(inv["parent"], inv["blen"], names)
                assert z.keys() == before.keys() and all(abs(z[k] - before[k]) <= 4e-16 * before[k] for k in z)
                if e2["C"] == moved:
                    exact += 1
                    off, idx = E._child_arrays(c.parent, None, None)
                    assert np.array_equal(inv["parent"], c.parent) and np.array_equal(inv["child_idx"], idx)
                    if e["kind"] != "root2":                    # a root-spanning edge that went through t* = 0 comes back in halves: its sum is held above
                        assert np.array_equal(inv["blen"], c.start)
    assert exact >= 20
    c = cases()[0]
    with pytest.raises(E.EngineError, match="error -1: .*not eligible"):
        E.tree_nni_apply(c.parent, c.start, c.leaves[0], 1, 0.1)
    with pytest.raises(E.EngineError, match="error -1: .*arrangement 3"):
        E.tree_nni_apply(c.parent, c.start, eligible(c.parent)[0][0]["u"], 3, 0.1)


def test_newick_from_arrays_quotes_as_the_writer_of_lengths_does():
    parent = np.array([-1, 0, 1, 1, 0, 0], np.int32)
    names = ["top", "clade:x", "a(1)", "plain", "c,3", ""]
    blen = np.array([0, 0.1, 1.0 / 3, 2e-7, 5.0, 0.25])
    text = E.newick_from_arrays(parent, None, None, names, blen)
    assert text == "(('a(1)':0.33333333333333331,plain:1.9999999999999999e-07)'clade:x':0.10000000000000001,'c,3':5,:0.25)top;\n"
    assert E.newick_write(text, E.newick_parse(text)["blen"]) == text
    off = np.array([0, 3, 5, 5, 5, 5, 5], np.int32); idx = np.array([5, 4, 1, 3, 2], np.int32)
    assert E.newick_from_arrays(parent, off, idx, names, blen).startswith("(:0.25,'c,3':5,(plain:")
    with pytest.raises(E.EngineError, match="error -1"):
        E.newick_from_arrays(parent, off, np.array([5, 4, 1, 3, 3], np.int32), names, blen)


# ---- 4. the search ----

def simulate(parent, blen, L, rm, rng):
    """an alignment down the tree: the root's bases from pi, a child's from the row of P(t) of its parent's base"""
    n = len(parent)
    seq = np.zeros((n, L), np.int8)
    seq[0] = rng.choice(4, size=L, p=rm.pi / rm.pi.sum())
    for u in range(1, n):                                      # preorder: a parent comes before its children
        P = rm.P(blen[u]); P = np.clip(P, 0, None); P /= P.sum(1)[:, None]
        cum = np.cumsum(P, axis=1)[seq[parent[u]]]
        seq[u] = np.minimum((rng.random(L)[:, None] > cum).sum(1), 3)
    return seq


def search_case():
    """a known 12-leaf tree, lengths 0.05 to 0.2, HKY85, 600 columns; the start: that tree after two non-adjacent NNIs, lengths 0.1"""
    def make():
        rng = np.random.default_rng(2024)
        c = Case()
        c.name = "search"
        c.true_parent = build_tree(12, rng, top=3)
        n = len(c.true_parent)
        c.sm = synth.load_model("HKY85"); c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par); c.rm = RefModel(c.sm)
        c.min_len, c.max_len = 0.0, 10.0
        c.true_blen = np.where(c.true_parent >= 0, rng.uniform(0.05, 0.2, n), 0.0)
        seq = simulate(c.true_parent, c.true_blen, 600, c.rm, rng)
        kids = kids_of(c.true_parent)
        for u in range(n):
            if kids[u]:
                seq[u] = -2
        c.seq = np.ascontiguousarray(seq, np.int8)
        c.names = ["" if kids[u] else "s%d" % u for u in range(n)]
        # two edges that share no end node and are no neighbours
        edges = [e for e in eligible(c.true_parent)[0] if e["kind"] == "inner"]
        first = edges[0]
        far = [e for e in edges if not {e["u"], e["p"]} & {first["u"], first["p"], first["A"], first["B"], first["C"], int(c.true_parent[first["p"]])}]
        second = far[-1]
        par = c.true_parent
        c.perturbed = []
        for e, q in ((first, 1), (second, 2)):
            par, _ = rearranged(par, c.true_blen, edge_parts(par, e["u"]), q)
            c.perturbed.append(e["u"])
        c.parent = par
        c.start = np.where(c.parent >= 0, 0.1, 0.0)
        return c
    return cached("search", make)


def restated_gains(c, parent, blen):
    """per eligible edge of the tree: u, the gain of its better rearrangement, each arrangement at its own restated optimum"""
    cc = Case(); cc.parent = np.asarray(parent, np.int32); cc.seq = c.seq; cc.rm = c.rm
    out = []
    for e in eligible(cc.parent)[0]:
        f = []
        for q in range(3):
            a = Arrangement(cc, blen, e, q)
            f.append(a.f(a.optimum(c.min_len, c.max_len)))
        out.append((e["u"], max(f[1], f[2]) - f[0]))
    return out


def check_search(c, r, need_truth):
    lls = [r["ll_start"]] + [x["ll"] for x in r["rounds"]]
    assert all(b > a for a, b in zip(lls, lls[1:])), lls
    assert r["ll_final"] >= lls[-1]
    assert r["stop"] == "local optimum", r["stop"]
    assert is_tree(r["parent"], c.parent)
    assert sum(x["applied"] for x in r["rounds"]) == len(r["swaps"])
    if need_truth:
        assert bipartitions(r["parent"], r["blen"], c.names).keys() == bipartitions(c.true_parent, c.true_blen, c.names).keys()
    # the certificate: on the final tree the restatement finds no edge whose rearrangement gains more than min_gain
    gains = restated_gains(c, r["parent"], r["blen"])
    assert gains and max(g for u, g in gains) <= MIN_GAIN, gains
    want = RefTree(r["parent"], c.seq, c.rm).messages(r["blen"]).loglik()
    assert abs(r["ll_final"] - want) <= SCORE_BAR * abs(want)


def test_search_recovers_the_tree_the_alignment_came_from_host():
    c = search_case()
    # the seed makes both perturbing swaps strictly improving: by the restatement, on the start tree with fitted lengths
    fit = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)
    gains = dict(restated_gains(c, c.parent, fit["blen"]))
    assert all(gains[u] > 1.0 for u in c.perturbed), gains
    r = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True)
    print(r["stop"], r["rounds"], r["swaps"], r["ll_start"], r["ll_final"])
    assert r["ll_start"] == fit["ll_final"] and len(r["swaps"]) >= 2
    check_search(c, r, need_truth=True)
    again = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True, mem_budget=1 << 40)
    assert np.array_equal(again["parent"], r["parent"]) and np.array_equal(again["blen"], r["blen"]) and again["swaps"] == r["swaps"]
    one = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True, nni_rounds=1)
    assert one["stop"] == "max rounds" and one["rounds"] == r["rounds"][:1] and one["ll_final"] > one["rounds"][0]["ll"]


def nj_search_case():
    def make():
        c0 = search_case()
        kids = kids_of(c0.true_parent)
        leaves = [u for u in range(len(kids)) if not kids[u]]
        rows = c0.seq[leaves]; names = [c0.names[u] for u in leaves]
        D, _ = E.msa_distances(rows, "HKY85", c0.sm.pi, host=True)
        t = E.newick_parse(E.nj_newick(names, E.nj(D, host=True)))
        c = Case()
        c.name = "NJ start"; c.min_len, c.max_len = 0.0, 10.0
        c.parent = np.asarray(t["parent"], np.int32); c.sm, c.md, c.rm = c0.sm, c0.md, c0.rm
        c.names = list(t["names"]); c.child_off, c.child_idx = t["child_off"], t["child_idx"]
        c.seq = np.full((len(c.parent), rows.shape[1]), -2, np.int8)
        for u, nm in enumerate(c.names):
            if nm:
                c.seq[u] = rows[names.index(nm)]
        c.start = np.clip(np.asarray(t["blen"], float), 0.0, 10.0)
        return c
    return cached("njsearch", make)


def test_search_from_the_programs_own_nj_tree_host():
    c = nj_search_case()
    r = E.tree_nni_search(c.parent, c.start, c.seq, c.md, child_off=c.child_off, child_idx=c.child_idx, host=True)
    print(r["stop"], r["rounds"], r["swaps"])
    check_search(c, r, need_truth=False)
    assert r["ll_final"] >= E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)["ll_final"]


HALVING_PARENT = [-1, 0, 0, 0, 3, 3, 5, 6, 6, 5, 9, 10, 10, 9]
HALVING_ROWS = {1: "CC-CCAGGGCTAGTGT-CTTCGTAGA", 2: "CC-CTAGCGCT-GAGTGATTAGT-GG", 4: "-C-GCGGCGCGAGTGTCCTACGTAGG", 7: "CC-GC-ACGCGAGT-CCATTCA-A-A",
                8: "CC-GTAGGGCGGG-GTGCTTAGTGGA", 11: "CC-CCAA-GCTAGTG-TCTTCGTAGA", 12: "GC-GTAGCGCTGGTGTGCTTCGTGGA", 13: "CC-GCAGCGCGGGTGTTCTTCGTAGA"}


def test_a_rejected_set_of_swaps_is_halved_host():
    """eight leaves, 26 columns (found by a search over random short alignments): the edges above 6 and above 10 are one node apart
    (5 - 9), both are candidates and share no end node, so both are taken; applied together they lower the log-likelihood, and the
    better one alone is applied"""
    c = Case()
    c.parent = np.array(HALVING_PARENT, np.int32); c.min_len, c.max_len = 0.0, 10.0
    c.sm = synth.load_model("HKY85"); c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par); c.rm = RefModel(c.sm)
    c.seq = np.full((len(c.parent), 26), -2, np.int8)
    for u, row in HALVING_ROWS.items():
        c.seq[u] = ["ACGT".index(x) if x != "-" else -2 for x in row]
    c.names = ["s%d" % u if u in HALVING_ROWS else "" for u in range(len(c.parent))]
    start = np.where(c.parent >= 0, 0.1, 0.0)
    r = E.tree_nni_search(c.parent, start, c.seq, c.md, host=True)
    first = r["rounds"][0]
    assert (first["candidates"], first["taken"], first["applied"]) == (2, 2, 1) and r["swaps"][0][:2] == (1, 6)
    # the two swaps at once are worse than the fitted start, by the restatement on the really rearranged tree
    fit = E.tree_optimize_lengths(c.parent, start, c.seq, c.md, host=True)
    sc = E.tree_nni_scores(c.parent, fit["blen"], c.seq, c.md, host=True)
    par, bl = c.parent, fit["blen"]
    for u in (6, 10):
        i = list(sc["edge_node"]).index(u); q = 1 if sc["f"][i][1] >= sc["f"][i][2] else 2
        assert max(sc["f"][i][1], sc["f"][i][2]) - sc["f"][i][0] > MIN_GAIN
        par, bl = rearranged(par, bl, edge_parts(par, u), q, sc["t_star"][i][q])
    assert RefTree(par, c.seq, c.rm).messages(bl).loglik() < RefTree(c.parent, c.seq, c.rm).messages(fit["blen"]).loglik()
    check_search(c, r, need_truth=False)


def test_search_entries_refuse_what_the_header_says():
    c = cases()[3]
    dg = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.4, 1.0, 2.5])
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_nni_scores(c.parent, c.start, c.seq, dg, host=True)
    for kw in (dict(nni_rounds=0), dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=float("nan")), dict(eps=1e-7), dict(max_rounds=0)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True, **kw)
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need (\d+) bytes .*budget is 1048576 bytes") as ei:
        E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True, mem_budget=1 << 20)
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) == E.nni_need(n, L)
    inner = (n - 1) // 2
    assert E.nni_need(n, L) == E.blen_need(n, L) + 160 * inner
    assert E.nni_need(n, E.NNI_LDS_COLS + 1) == E.blen_need(n, E.NNI_LDS_COLS + 1) + 160 * inner + 72 * inner * (E.NNI_LDS_COLS + 1)
    assert 4 * (6144 + 72 * E.NNI_LDS_COLS) <= 160 * 1024 < 4 * (6144 + 72 * (E.NNI_LDS_COLS + 1))


# ---- 5. the program ----

def program_case(tmp_path):
    c = search_case()
    kids = kids_of(c.parent)
    leaves = [u for u in range(len(kids)) if not kids[u]]
    fa = tmp_path / "in.fasta"
    write_fasta(fa, [c.names[u] for u in leaves], c.seq[leaves])
    tree = tmp_path / "start.tree"
    names = list(c.names); names[0] = "top"
    tree.write_text(to_newick(c.parent, kids, names, c.start) + ";\n")
    return c, fa, tree


def read_log(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "round\tll\tscored\tcandidates\ttaken\tapplied"
    assert re.fullmatch(r"# stop: (local optimum|no improving swap|max rounds)", lines[-2]) and re.fullmatch(r"# skipped: \d+ edges at polytomies", lines[-1])
    rows = [x.split("\t") for x in lines[1:-2]]
    assert [int(x[0]) for x in rows] == list(range(len(rows))) and rows[0][2:] == ["0", "0", "0", "0"] and all(len(x) == 6 for x in rows)
    ll = [float(x[1]) for x in rows]
    assert all(b > a for a, b in zip(ll, ll[1:]))
    return rows, lines[-2][8:]


def test_program_nni_with_a_start_tree_and_without(tmp_path):
    c, fa, tree = program_case(tmp_path)
    out, log = tmp_path / "out.tree", tmp_path / "nni.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--nni", "--start-tree", tree, "-o", out, "--nni-log", log, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"NNI search: log-likelihood -\d+\.\d+ -> -\d+\.\d+, \d+ swap\(s\) applied in \d+ round\(s\), stop: local optimum", r.stderr), r.stderr
    assert re.search(r"fits \S+ s, scoring \S+ s, trials \S+ s", r.stderr)
    want = E.tree_nni_search(c.parent, np.array([float("%.6g" % x) for x in c.start]), c.seq, c.md, host=True)
    rows, stop = read_log(log)
    assert stop == "local optimum" and len(rows) - 1 == len(want["rounds"])
    assert [float(x[1]) for x in rows[1:]] == [x["ll"] for x in want["rounds"]] and float(rows[0][1]) == want["ll_start"]
    assert [[int(v) for v in x[2:]] for x in rows[1:]] == [[x["scored"], x["candidates"], x["taken"], x["applied"]] for x in want["rounds"]]
    back = E.newick_parse(out.read_text())
    assert back["names"][0] == "top"                            # the top node stays
    a, b = bipartitions(back["parent"], back["blen"], back["names"]), bipartitions(want["parent"], want["blen"], c.names)
    assert a.keys() == b.keys() == bipartitions(c.true_parent, c.true_blen, c.names).keys()
    assert all(abs(a[k] - b[k]) <= 4e-16 * b[k] for k in a)
    # from the joins
    out2, log2 = tmp_path / "nj.tree", tmp_path / "nj.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--nni", "-o", out2, "--nni-log", log2, "--nni-rounds", 5, "--nni-min-gain", "0.01"])
    assert r.returncode == 0, r.stderr
    read_log(log2)
    plain = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "-o", tmp_path / "ml.tree"])
    assert plain.returncode == 0
    t2, t1 = E.newick_parse(out2.read_text()), E.newick_parse((tmp_path / "ml.tree").read_text())
    assert sorted(x for x in t2["names"] if x) == sorted(x for x in t1["names"] if x)


def test_program_without_nni_writes_what_the_parent_commit_wrote(tmp_path):
    """70_otus on the host path against the files of tests/golden/tree_blen"""
    for model in ("JC69", "GTR"):
        out = tmp_path / ("nj_%s.tree" % model)
        r = _run([_bin(), FASTA70, "--host", "-o", out] + ([] if model == "JC69" else ["-sm", sm(model)]))
        assert r.returncode == 0, r.stderr
        with open(os.path.join(ROOT, "tests", "golden", "tree_blen", "70_otus_nj_host_%s.tree" % model), "rb") as f:
            assert out.read_bytes() == f.read()


def test_program_nni_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, fa, tree = program_case(tmp_path)
    ml = ["-sm", sm("HKY85"), "--ml-lengths"]
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa, "-sm", sm("HKY85"), "--nni"], "--nni goes with --ml-lengths"),
                      ([fa] + ml + ["--nni-rounds", "3"], "go with --nni"),
                      ([fa] + ml + ["--nni-min-gain", "0.1"], "go with --nni"),
                      ([fa] + ml + ["--nni-log", tmp_path / "x.log"], "go with --nni"),
                      ([fa] + ml + ["--nni", "--nni-rounds", "0"], "--nni-rounds"),
                      ([fa] + ml + ["--nni", "--nni-min-gain", "0"], "--nni-min-gain"),
                      ([fa] + ml + ["--nni", "--nni-min-gain", "-1"], "--nni-min-gain"),
                      ([fa] + ml + ["--nni", "--mem", "0.0001"], r"--nni: .*need \d+ bytes .* --mem allows 100000 bytes"),
                      ([fa] + ml + ["--nni", "--mem", "0.0001", "--start-tree", tree], r"need \d+ bytes .* --mem allows 100000 bytes")):
        r = _run([_bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


# ---- 6. the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_nni_host.cpp and hu_blen_host.cpp (no HIP headers) with tests/san/nni_driver.cpp under AddressSanitizer + UBSan, run as a
    stand-alone program: the scores, apply, the selection with its halving and a short search on two small trees"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nni_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "nni_driver.cpp"), os.path.join(CSRC, "hu_nni_host.cpp"), os.path.join(CSRC, "hu_blen_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "halving: 5 -> 3 -> 2 -> 1" in r.stdout and "searches: 2" in r.stdout


# ---- the device ----

def device_case(n_leaves, L):
    def make():
        rng = np.random.default_rng(1000 * n_leaves + L)
        kind = (n_leaves + L) % 3
        # random_tree has a node with four children, which leaves a small tree without an eligible edge
        parent = (build_tree(n_leaves, rng, top=2) if kind == 1 or n_leaves < 5 else random_tree(n_leaves, rng) if kind == 2 and n_leaves >= 12
                  else build_tree(n_leaves, rng, top=3))
        return make_case(parent, L, ("JC69", "HKY85", "GTR")[(n_leaves + L) % 3], 100 * n_leaves + L, random_leaf=n_leaves >= 5,
                         max_len=2.0 if n_leaves >= 5 else 10.0)
    return cached(("dev", n_leaves, L), make)


DEVICE_SHAPES = [(4, 1), (5, 63), (5, 64), (33, 65), (130, 255), (6, 256), (33, 257), (5, E.NNI_LDS_COLS), (5, E.NNI_LDS_COLS + 1),
                 (5, E.BLEN_LDS_COLS + 1), (130, 1000)]


def test_the_devices_shapes_hold_the_three_root_cases_and_the_host_path_meets_the_bar_on_them():
    kinds, worst = set(), 0.0
    for n_leaves, L in DEVICE_SHAPES:
        c = device_case(n_leaves, L)
        assert eligible(c.parent)[0], (n_leaves, L)
        kinds |= {e["kind"] for e in eligible(c.parent)[0]}
        if n_leaves * L <= 10000 and L > 1:
            worst = max(worst, check_scores(c, scores(c, host=True))[0])
    print("largest deviation of the host path's f on the device's shapes: %.3g" % worst)
    assert kinds == {"inner", "root3", "root2"} and worst <= F_BAR


@pytest.mark.gpu
def test_scores_and_optima_against_the_restatement_device():
    """measured: DEVICE_WORST"""
    _need_gpu()
    worst = run_restatement(host=False)
    print("largest deviation of the device's f: %.3g" % worst)
    assert worst <= F_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L):
    """the edges of a thread's stride (256 columns) and of a wave, one column, and the column counts on either side of the switch from
    ratios in LDS to ratios in global memory, of this kernel and of the fit's: t* within 2 tau of the host path's, f under the bar, the
    same bits twice"""
    _need_gpu()
    c = device_case(n_leaves, L)
    host, dev, again = scores(c, host=True), scores(c, host=False), scores(c, host=False)
    assert len(host["edge_node"]) > 0
    for k in ("edge_node", "t_star", "f", "f0_at_blen"):
        assert np.array_equal(dev[k], again[k]), k
    assert np.array_equal(dev["edge_node"], host["edge_node"]) and dev["skipped"] == host["skipped"]
    gap = np.abs(dev["t_star"] - host["t_star"]).max()
    with np.errstate(invalid="ignore"):
        dev_f = np.abs(dev["f"] - host["f"]) / np.abs(host["f"])
        dev_f0 = np.abs(dev["f0_at_blen"] - host["f0_at_blen"]) / np.abs(host["f0_at_blen"])
    worst = max(dev_f.max(), dev_f0.max())
    print("n %d L %d: largest |t* device - t* host| %.3g, largest deviation of f %.3g" % (n_leaves, L, gap, worst))
    assert gap <= 2 * TAU and worst <= F_BAR
    if n_leaves * L <= 10000 and L > 1:
        w = check_scores(c, dev)[0]
        print("n %d L %d: largest deviation of the device's f from the restatement %.3g" % (n_leaves, L, w))
        assert w <= F_BAR


@pytest.mark.gpu
def test_search_on_the_device():
    _need_gpu()
    c = search_case()
    host = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True)
    # no two candidate gains of a round within 1e-6 of each other, by the host scores: a differing last bit cannot reorder them
    par, bl = c.parent, c.start
    for rnd in range(len(host["rounds"])):
        fit = E.tree_optimize_lengths(par, bl, c.seq, c.md, host=True)
        sc = E.tree_nni_scores(par, fit["blen"], c.seq, c.md, host=True)
        gain = np.sort((np.maximum(sc["f"][:, 1], sc["f"][:, 2]) - sc["f"][:, 0]))
        gain = gain[gain > MIN_GAIN / 2]
        assert len(gain) > 0 and (len(gain) < 2 or np.diff(gain).min() > 1e-6), gain
        bl = fit["blen"]
        for r_, u, q in [s for s in host["swaps"] if s[0] == rnd + 1]:
            i = list(sc["edge_node"]).index(u)
            a = E.tree_nni_apply(par, bl, u, q, sc["t_star"][i][q])
            par, bl = a["parent"], a["blen"]
    dev = E.tree_nni_search(c.parent, c.start, c.seq, c.md)
    assert dev["swaps"] == host["swaps"] and dev["stop"] == host["stop"] and np.array_equal(dev["parent"], host["parent"])
    assert abs(dev["ll_final"] - host["ll_final"]) <= F_BAR * abs(host["ll_final"])
    check_search(c, dev, need_truth=True)


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    _need_gpu()
    c = cases()[4]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.nni_need(n, L)):
        E.tree_nni_scores(c.parent, c.start, c.seq, c.md, mem_budget=1 << 20)


@pytest.mark.gpu
def test_tree_nni_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree --ml-lengths --nni -> hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm on 70_otus: a database that
    hmmufotu-amd loads"""
    _need_gpu()
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "--ml-lengths", "--nni", "--nni-rounds", 2, "--ml-rounds", 5, "-o", "nni.tree", "--nni-log", "nni.log", "-v"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "NNI search" in r.stderr
    rows, stop = read_log(tmp_path / "nni.log")
    print(rows, stop)
    r = _run([_bin("hmmufotu-amd-train-sm"), FASTA70, "nni.tree", "-o", "nni.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), FASTA70, "nni.tree", "--no-hmm", "-sm", "nni.sm", "-n", "nnidb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "nnidb.ptu"))
    assert (np.asarray(db["parent"]) < 0).sum() == 1
    r = _run([_bin("hmmufotu-amd-train-hmm"), FASTA70, "-dm", os.path.join(REF, "gg_97_otus.dm"), "-o", "nnidb.hmm"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    D = E.Database.load(str(tmp_path / "nnidb.hmm"), str(tmp_path / "nnidb.ptu"))
    assert D.n_nodes == db["n_nodes"]
    D.close()
