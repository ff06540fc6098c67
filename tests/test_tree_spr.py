"""hmmufotu-amd-tree --ml-lengths --spr: subtree pruning and regrafting.

The yardstick is a restatement in this file that shares no code with the library.  It names the prunable nodes and, by a
breadth-first search over the edges of the pruned tree, their targets with their distances; it REALLY MOVES the subtree on the parent
array (the target edge split in halves, the pendant the free length), prunes that tree with the RefTree of tests/test_tree_blen.py
(float64 linear space, a scale per node, math.fsum) and takes the pendant's f, f' and, by bisection on f', its optimum.  A target's
score is therefore held against a tree that was really rearranged, not against the recomputed messages under test.

The bar of f, relative to |f|: measured against the restatement over every case of this file, the device's shapes included, the
largest deviation is HOST_WORST on the host path and DEVICE_WORST on the device; four times the larger, rounded up to a power of two,
is F_BAR, far below the 1e-10 above which a formula would be wrong.  t* is held as the branch-length fit's step is: the restated slope
changes sign within 2 HU_BLEN_TAU of it, or the end of the interval is justified; device and host t* lie within 2 HU_BLEN_TAU.
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
from test_tree_blen import RefModel, RefTree, random_tree, sm, to_newick, write_fasta, SCORE_BAR  # noqa: E402
from test_tree_nni import (Case, bipartitions, build_tree, cases, edge_parts, is_tree, kids_of, make_case, nj_search_case,  # noqa: E402
                           simulate, tree_loglik_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70 = os.path.join(REF, "70_otus.fasta.gz")
TAU = E.BLEN_TAU
MIN_GAIN = 1e-3
HOST_WORST = 5.81e-15       # measured: the host path, 12 leaves x 1,451 columns (its serial sums); 2.15e-15 over spr_cases() at the far radius
DEVICE_WORST = 2.25e-15     # measured: MI355X, 9 leaves x 65 columns; 1.36e-15 over spr_cases() at the far radius
F_BAR = 2.0 ** -45          # 4 x 5.81e-15 = 2.3e-14, rounded up to a power of two: 2.84e-14
assert F_BAR <= 1e-10
FAR = 32                    # a radius beyond the diameter of every tree of this file


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


# ---- the restatement: prunable nodes, targets, moved trees, scores ----

def prune_parts(parent, v):
    """v, p, s, g of a prunable v; None for the root; "skipped" where the parent is the root or no node of two children"""
    parent = np.asarray(parent); kids = kids_of(parent)
    if parent[v] < 0:
        return None
    p = int(parent[v])
    if parent[p] < 0 or len(kids[p]) != 2:
        return "skipped"
    return dict(v=v, p=p, s=[x for x in kids[p] if x != v][0], g=int(parent[p]))


def prunable(parent):
    out, skipped = [], 0
    for v in range(len(parent)):
        e = prune_parts(parent, v)
        if e == "skipped":
            skipped += 1
        elif e is not None:
            out.append(e)
    return out, skipped


def pruned_tree(parent, blen, e):
    """T': parent with -2 for the nodes lifted out (the subtree of v, and p), s on g over the merged length"""
    par = np.array(parent, np.int64); bl = np.array(blen, float); kids = kids_of(parent)
    gone = [e["v"]]
    for x in gone:
        gone += kids[x]
    par[gone] = -2; par[e["p"]] = -2
    par[e["s"]] = e["g"]; bl[e["s"]] = blen[e["s"]] + blen[e["p"]]
    return par, bl


def targets_of(parent, blen, e, radius):
    """{w: distance} by a breadth-first search over the edges of T' from the edge of s: two edges are neighbours when they share a node"""
    par, _ = pruned_tree(parent, blen, e)
    at = {}                                                    # node -> the edges (lower ends) that touch it
    for w in range(len(par)):
        if par[w] >= 0:
            at.setdefault(w, []).append(w); at.setdefault(int(par[w]), []).append(w)
    dist = {e["s"]: 0}
    front = [e["s"]]
    for d in range(1, radius + 1):
        nxt = []
        for w in front:
            for node in (w, int(par[w])):
                for w2 in at[node]:
                    if w2 not in dist:
                        dist[w2] = d; nxt.append(w2)
        front = nxt
    del dist[e["s"]]
    return dist


def moved(parent, blen, e, w, t=None):
    """the arrays after the subtree of v went into the edge of w: that edge in halves, the pendant at t when given"""
    par, bl = pruned_tree(parent, blen, e)
    assert par[w] >= 0 and w != e["s"]
    pw = par[w]; half = 0.5 * bl[w]
    out = np.array(parent, np.int32); ob = np.array(blen, float)
    out[e["s"]] = e["g"]; ob[e["s"]] = bl[e["s"]]
    out[e["p"]] = pw; out[w] = e["p"]; ob[w] = half; ob[e["p"]] = half
    if t is not None:
        ob[e["v"]] = t
    return out, ob


class Regraft:
    """the moved tree (w = s: the tree as it stands) pruned and rooted at the pendant of v: f(t), its slope and its optimum"""

    def __init__(self, c, blen, e, w):
        par, bl = (np.asarray(c.parent), np.asarray(blen, float)) if w == e["s"] else moved(c.parent, blen, e, w)
        ref = RefTree(par, c.seq, c.rm).messages(bl)
        v = e["v"]
        # what RefTree.branch reads of the pendant: the two sides in linear space and the logarithms divided out
        self.m, self.x, self.y, self.s = c.rm, ref.up[v] * c.rm.pi[None, :], ref.down[v], ref.us[v] + ref.ds[v]

    def _L(self, t, order):
        return np.einsum("ja,ab,jb->j", self.x, self.m.P(t, order), self.y)

    def f(self, t):
        with np.errstate(divide="ignore"):
            return math.fsum(np.log(self._L(t, 0)) + self.s)

    def slope(self, t):
        with np.errstate(divide="ignore", invalid="ignore"):
            return math.fsum(self._L(t, 1) / self._L(t, 0))

    def optimum(self, lo, hi):
        if not self.slope(lo) > 0:
            return lo
        if not self.slope(hi) < 0:
            return hi
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if self.slope(mid) > 0:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)


def regraft(c, blen, e, w):
    """a Regraft of a case's own start, kept: the host's and the device's scores are held against the same one"""
    if blen is not c.start:
        return Regraft(c, blen, e, w)
    return cached(("regraft", c.name, e["v"], w), lambda: Regraft(c, blen, e, w))


def check_t_star(a, t, lo, hi, what):
    """the branch-length fit's rule, with the slope held to its own rounding: a column's term of f' is a quotient of sums of four products
    of size up to max |lambda|, each rounded to 2^-53, so a slope that is 0 in exact arithmetic (a leaf row of gaps only under JC69, whose
    pendant has a flat f) comes out anywhere within 4 x 2^-52 x max |lambda| x columns of 0"""
    noise = 4 * 2.0 ** -52 * np.abs(a.m.lam).max() * len(a.s)
    assert lo <= t <= hi, what
    if t == lo:
        assert a.slope(lo) <= noise, what
        return "min"
    if t == hi:
        assert a.slope(hi) >= -noise, what
        return "max"
    assert a.slope(max(t - 2 * TAU, lo)) >= -noise and a.slope(min(t + 2 * TAU, hi)) <= noise, what
    return "inner"


def rel(a, b):
    return abs(a - b) / abs(b)


def check_scores(c, got, radius, blen=None):
    """every prunable node, its baseline and every target against the restatement; the largest deviation of f and what was met"""
    blen = c.start if blen is None else blen
    want, skipped = prunable(c.parent)
    assert [e["v"] for e in want] == list(got["prune_node"]) and got["skipped"] == skipped, c.name
    assert len(got["v_off"]) == len(want) + 1 and got["v_off"][0] == 0 and got["v_off"][-1] == len(got["target_node"])
    worst, met = 0.0, set()
    root = int(np.nonzero(np.asarray(c.parent) < 0)[0][0]); kids = kids_of(c.parent)
    for i, e in enumerate(want):
        a, b = got["v_off"][i], got["v_off"][i + 1]
        tg = targets_of(c.parent, blen, e, radius)
        assert dict(zip(got["target_node"][a:b].tolist(), got["dist"][a:b].tolist())) == tg and b - a == len(tg), (c.name, e)
        base = regraft(c, blen, e, e["s"])
        met.add(check_t_star(base, got["base_t"][i], c.min_len, c.max_len, (c.name, e["v"], "baseline")))
        worst = max(worst, rel(got["base_f"][i], base.f(got["base_t"][i])), rel(got["f_at_blen"][i], base.f(blen[e["v"]])))
        if e["g"] == root:
            met.add("g is the root")
        for k in range(a, b):
            w, t = int(got["target_node"][k]), got["t_star"][k]
            r = regraft(c, blen, e, w)
            met.add(check_t_star(r, t, c.min_len, c.max_len, (c.name, e["v"], w, t)))
            worst = max(worst, rel(got["f"][k], r.f(t)))
            if c.parent[w] == root and len(kids[root]) == 2 and e["g"] != root and got["dist"][k] < radius:
                met.add("a bifurcating root on a walk")
            if len(kids[int(c.parent[w])]) >= 4 and got["dist"][k] < radius:
                met.add("four children in a neighbourhood")
            if len(kids[root]) == 3 and c.parent[w] == root:
                met.add("a trifurcating top node")
    return worst, met


# ---- the inputs ----

def spr_cases():
    """the trees of tests/test_tree_nni.py: 4, 6, 12 and 33 leaves under the three models, a trifurcating top node, a bifurcating root
    with two inner children and with a leaf child, a node with four children, gaps, a leaf row of gaps only, a leaf of random bases"""
    return cases()


def scores(c, host, radius, **kw):
    return E.tree_spr_scores(c.parent, c.start, c.seq, c.md, radius=radius, min_len=c.min_len, max_len=c.max_len, host=host, **kw)


def far_scores(c, host):
    return cached(("far", c.name, host), lambda: scores(c, host, FAR))


def impossible_case():
    """six leaves; two sister leaves on branches of length 0 that differ in column 0: the column has likelihood 0"""
    def make():
        c = make_case(build_tree(6, np.random.default_rng(3), top=2, leaf_child=True), 20, "HKY85", 11)
        sis = [k for k in c.kids if len(k) == 2 and not c.kids[k[0]] and not c.kids[k[1]]][0]
        c.seq[sis[0], 0] = 0; c.seq[sis[1], 0] = 1
        c.start = c.start.copy(); c.start[sis] = 0.0
        c.sisters = sis
        return c
    return cached("impossible", make)


# ---- 1. the pulley principle ----

def test_pulley_every_prunable_node_gives_the_tree_loglik():
    met = 0
    for c in spr_cases():
        got = scores(c, True, 1)
        want = tree_loglik_host(c.parent, c.start, c)
        assert abs(RefTree(c.parent, c.seq, c.rm).messages(c.start).loglik() - want) <= SCORE_BAR * abs(want)
        assert len(got["f_at_blen"]) == len(prunable(c.parent)[0]) > 0
        assert np.all(np.abs(got["f_at_blen"] - want) <= SCORE_BAR * abs(want)), c.name
        assert np.all(got["base_f"] >= got["f_at_blen"] - SCORE_BAR * abs(want))
        met += len(got["f_at_blen"])
    assert met >= 100


# ---- 2. the target sets ----

def test_target_sets_against_the_restated_enumeration():
    # 33 leaves joined at random, and a balanced tree of 256 leaves in heap order, where a node in the middle sees no leaf up to distance 3
    trees = [cached("binary", lambda: make_case(build_tree(33, np.random.default_rng(12), top=3), 8, "JC69", 12)),
             cached("balanced", lambda: make_case(np.array([-1] + [(i - 1) // 2 for i in range(1, 511)], np.int32), 4, "JC69", 13))]
    for c, radius in [(c, r) for c in trees for r in (1, 2, 3, 5)]:
        got = scores(c, True, radius)
        full = 0
        for i, e in enumerate(prunable(c.parent)[0]):
            a, b = got["v_off"][i], got["v_off"][i + 1]
            tg = targets_of(c.parent, c.start, e, radius)
            assert dict(zip(got["target_node"][a:b].tolist(), got["dist"][a:b].tolist())) == tg
            # nothing inside the subtree of v, not p, v or the top node
            inside = [e["v"]]
            for x in inside:
                inside += c.kids[x]
            assert not set(got["target_node"][a:b].tolist()) & (set(inside) | {e["p"], 0})
            count = np.bincount(got["dist"][a:b], minlength=radius + 1)
            assert count[0] == 0 and all(count[d] <= 2 ** (d + 1) for d in range(1, radius + 1))
            full += all(count[d] == 2 ** (d + 1) for d in range(1, min(radius, 3) + 1))
        assert full > 0 or c is trees[0]                        # a neighbourhood without a leaf up to distance 3: 4, 8, 16 targets
    c = trees[0]
    # a polytomy as parent and a parent that is the top node are counted, three leaves have nothing to prune
    got = E.tree_spr_scores(np.array([-1, 0, 0, 0], np.int32), [0, .1, .1, .1], np.array([[-2], [0], [1], [2]], np.int8), c.md, host=True)
    assert len(got["prune_node"]) == 0 and got["skipped"] == 3 and len(got["target_node"]) == 0 and list(got["v_off"]) == [0]


# ---- 3. scores and optima against the restatement ----

def run_restatement(host):
    worst, met = 0.0, set()
    for c in spr_cases():
        w, m = check_scores(c, far_scores(c, host), FAR)
        print("%s: largest deviation of f %.3g" % (c.name, w))
        worst = max(worst, w); met |= m
        # radius 1, 2, 3: the restated sets, and the bits of the same targets at the radius beyond the diameter
        far = far_scores(c, host)
        for radius in (1, 2, 3):
            got = scores(c, host, radius)
            assert np.array_equal(got["prune_node"], far["prune_node"]) and np.array_equal(got["base_f"], far["base_f"])
            for i, e in enumerate(prunable(c.parent)[0]):
                a, b = got["v_off"][i], got["v_off"][i + 1]
                assert dict(zip(got["target_node"][a:b].tolist(), got["dist"][a:b].tolist())) == targets_of(c.parent, c.start, e, radius)
                fa = far["v_off"][i]
                at = {int(far["target_node"][k]): k for k in range(fa, far["v_off"][i + 1])}
                for k in range(a, b):
                    k2 = at[int(got["target_node"][k])]
                    assert got["f"][k] == far["f"][k2] and got["t_star"][k] == far["t_star"][k2] and got["dist"][k] == far["dist"][k2]
    assert {"g is the root", "a bifurcating root on a walk", "four children in a neighbourhood", "a trifurcating top node", "inner"} <= met, met
    assert met & {"min", "max"}, met
    assert any(c.random is not None for c in spr_cases())
    return worst


def test_scores_and_optima_against_the_restatement_host():
    """measured: HOST_WORST"""
    worst = run_restatement(host=True)
    print("largest deviation of the host path's f: %.3g" % worst)
    assert worst <= F_BAR


def check_impossible(host):
    c = impossible_case()
    got = scores(c, host, FAR)
    assert not np.isnan(got["f"]).any() and not np.isnan(got["t_star"]).any() and not np.isnan(got["base_f"]).any()
    want, _ = prunable(c.parent)
    n_inf = 0
    for i, e in enumerate(want):
        for k in range(got["v_off"][i], got["v_off"][i + 1]):
            r = Regraft(c, c.start, e, int(got["target_node"][k]))
            f = r.f(got["t_star"][k])
            if not np.isfinite(f):                             # the restatement divides by the column's largest entry, 0: nan or -inf
                assert got["f"][k] == -np.inf
                n_inf += 1
            else:                                              # a sister moved away: the column is possible again
                assert rel(got["f"][k], f) <= F_BAR
    # as the tree stands every pendant sees the impossible column, but for the sisters' own: there the pendant is the branch of length 0
    # itself, whose column section 22's clamp keeps off log 0
    assert n_inf > 0 and all(got["f_at_blen"][i] == -np.inf for i, e in enumerate(want) if e["v"] not in c.sisters)
    assert not np.isnan(got["f_at_blen"]).any() and not np.isnan(got["base_t"]).any()


def test_a_column_of_likelihood_zero_gives_minus_infinity_host():
    check_impossible(True)


# ---- 4. apply ----

def test_apply_gives_the_predicted_loglik_and_its_inverse_restores():
    n_moves = 0
    for c in spr_cases()[:6]:
        got = far_scores(c, True)
        names = ["n%d" % u for u in range(len(c.parent))]
        before = bipartitions(c.parent, c.start, names)
        for i, e in enumerate(prunable(c.parent)[0]):
            for k in range(got["v_off"][i], got["v_off"][i + 1]):
                w, t = int(got["target_node"][k]), got["t_star"][k]
                r = E.tree_spr_apply(c.parent, c.start, e["v"], w, t)
                par, bl = moved(c.parent, c.start, e, w, t)
                assert np.array_equal(r["parent"], par) and np.allclose(r["blen"], bl, rtol=1e-15, atol=0)
                kids = kids_of(r["parent"])
                order = [0]
                for u in order:
                    order += kids[u]
                assert sorted(order) == list(range(len(c.parent))) and sorted(u for u in order if not kids[u]) == sorted(c.leaves)
                assert sorted(kids[e["p"]]) == sorted([w, e["v"]])
                ll = tree_loglik_host(r["parent"], r["blen"], c)
                assert abs(ll - got["f"][k]) <= SCORE_BAR * abs(ll), (c.name, e["v"], w)
                text = E.newick_from_arrays(r["parent"], r["child_off"], r["child_idx"], names, r["blen"])
                back = E.newick_parse(text)
                assert back["names"][0] == names[0]
                x, y = bipartitions(r["parent"], r["blen"], names), bipartitions(back["parent"], back["blen"], back["names"])
                assert x.keys() == y.keys() and all(abs(x[q] - y[q]) <= 4e-15 * max(x[q], 1e-300) for q in x)
                # the inverse: v back into the edge of s, which now hangs on g
                inv = E.tree_spr_apply(r["parent"], r["blen"], e["v"], e["s"], c.start[e["v"]], r["child_off"], r["child_idx"])
                assert np.array_equal(inv["parent"], c.parent)
                off, idx = E._child_arrays(c.parent, None, None)
                assert np.array_equal(inv["child_idx"], idx)
                z = bipartitions(inv["parent"], inv["blen"], names)
                # the topology is back; the lengths too, but for the edges of s and p, which now share their sum in halves
                assert z.keys() == before.keys() and sum(abs(z[q] - before[q]) > 4e-16 * before[q] for q in z) <= 2
                assert abs(math.fsum(z.values()) - math.fsum(before.values())) <= 1e-14 * math.fsum(before.values())
                n_moves += 1
    assert n_moves >= 300


def test_a_move_to_a_child_edge_of_s_is_the_matching_nni():
    met = 0
    for c in spr_cases()[2:6]:
        names = ["n%d" % u for u in range(len(c.parent))]
        for e in prunable(c.parent)[0]:
            ed = edge_parts(c.parent, e["s"])
            if not isinstance(ed, dict) or ed["kind"] != "inner":
                continue
            # the edge above s with A < B below s and C = v: arrangement 1 exchanges B and v, so v becomes the sister of A
            for q, w in ((1, ed["A"]), (2, ed["B"])):
                a = E.tree_spr_apply(c.parent, c.start, e["v"], w, 0.1)
                b = E.tree_nni_apply(c.parent, c.start, e["s"], q, 0.1)
                assert bipartitions(a["parent"], a["blen"], names).keys() == bipartitions(b["parent"], b["blen"], names).keys()
                met += 1
    assert met >= 10


def test_apply_refuses_what_is_no_target_position():
    c = spr_cases()[4]
    e = [x for x in prunable(c.parent)[0] if c.kids[x["v"]]][0]
    for w, msg in ((e["v"], "no edge"), (e["p"], "no edge"), (0, "no edge"), (e["s"], "no move"), (c.kids[e["v"]][0], "inside the subtree"), (len(c.parent), "no edge")):
        with pytest.raises(E.EngineError, match="error -1: .*" + msg):
            E.tree_spr_apply(c.parent, c.start, e["v"], w, 0.1)
    skipped = [v for v in range(1, len(c.parent)) if prune_parts(c.parent, v) == "skipped"][0]
    for v in (0, skipped, -1):
        with pytest.raises(E.EngineError, match="error -1: .*not prunable"):
            E.tree_spr_apply(c.parent, c.start, v, e["s"], 0.1)
    with pytest.raises(E.EngineError, match="error -1: .*pendant length"):
        E.tree_spr_apply(c.parent, c.start, e["v"], e["g"] if e["g"] else c.kids[e["s"]][0], -0.5)


# ---- 5. the search ----

def restated_candidates(c, parent, blen, radius, lo=0.0, hi=10.0):
    """per prunable node of the tree: (gain, v, w, dist) of its best target, every position with the pendant at its restated optimum"""
    cc = Case(); cc.parent = np.asarray(parent, np.int32); cc.seq = c.seq; cc.rm = c.rm
    out = []
    for e in prunable(cc.parent)[0]:
        b = Regraft(cc, blen, e, e["s"])
        fb = b.f(b.optimum(lo, hi))
        best = None
        for w, d in sorted(targets_of(cc.parent, blen, e, radius).items()):
            r = Regraft(cc, blen, e, w)
            f = r.f(r.optimum(lo, hi))
            if best is None or f > best[0]:
                best = (f, w, d)
        if best is not None:
            out.append((best[0] - fb, e["v"], best[1], best[2]))
    return out


def marked_by(parent, v, w):
    """the nodes a move of v into the edge of w marks: its own six and the path from p to w"""
    e = prune_parts(parent, v)
    up = lambda x: [x] + (up(int(parent[x])) if parent[x] >= 0 else [])
    a, b = up(e["p"]), up(w)
    meet = [x for x in b if x in a][0]
    return {v, e["p"], e["s"], e["g"], w, int(parent[w])} | set(b[:b.index(meet) + 1]) | set(a[:a.index(meet) + 1])


def restated_selection(parent, sc, min_gain=MIN_GAIN):
    """the candidates of library scores in the order of the selection, and those of them taken"""
    cand = []
    for i, v in enumerate(sc["prune_node"]):
        a, b = sc["v_off"][i], sc["v_off"][i + 1]
        if b == a:
            continue
        k = min(range(a, b), key=lambda k: (-sc["f"][k], sc["target_node"][k]))
        if sc["f"][k] - sc["base_f"][i] > min_gain:
            cand.append((sc["f"][k] - sc["base_f"][i], int(v), int(sc["target_node"][k]), int(sc["dist"][k]), sc["t_star"][k]))
    cand.sort(key=lambda x: (-x[0], x[1], x[2]))
    used, taken = set(), []
    for x in cand:
        m = marked_by(parent, x[1], x[2])
        if not m & used:
            used |= m; taken.append(x)
    return cand, taken


def sim_case(n_leaves, seed):
    """an alignment of 600 columns simulated down a known tree, lengths 0.05 to 0.2, HKY85"""
    rng = np.random.default_rng(seed)
    c = Case()
    c.true_parent = build_tree(n_leaves, rng, top=3)
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
    return c


def spr_search_case(two=False):
    """a known tree of 12 leaves (two: of 16) after one SPR at distance >= 3 (two: after two, whose marked nodes are disjoint), lengths 0.1"""
    def make():
        c = sim_case(16 if two else 12, 77 if two else 2025)
        c.name = "spr search %d" % two
        par, bl = np.array(c.true_parent), np.array(c.true_blen)
        c.perturbed, used = [], set()
        for v in range(len(par) - 1, 0, -1):
            e = prune_parts(par, v)
            if not isinstance(e, dict):
                continue
            far = [w for w, d in sorted(targets_of(par, bl, e, 3).items()) if d == 3 and not marked_by(par, v, w) & used]
            if not far:
                continue
            used |= marked_by(par, v, far[-1])
            par, bl = moved(par, bl, e, far[-1])
            c.perturbed.append((v, far[-1]))
            if len(c.perturbed) == (2 if two else 1):
                break
        assert len(c.perturbed) == (2 if two else 1)
        c.parent = par
        c.start = np.where(c.parent >= 0, 0.1, 0.0)
        return c
    return cached(("sprsearch", two), make)


def check_search(c, r, radius, need_truth):
    lls = [r["ll_start"]] + [x["ll"] for x in r["rounds"]]
    assert all(b > a for a, b in zip(lls, lls[1:])), lls
    assert r["ll_final"] >= lls[-1]
    assert r["stop"] == "local optimum", r["stop"]
    assert is_tree(r["parent"], c.parent)
    assert sum(x["applied"] for x in r["rounds"]) == len(r["moves"])
    if need_truth:
        assert bipartitions(r["parent"], r["blen"], c.names).keys() == bipartitions(c.true_parent, c.true_blen, c.names).keys()
    # the certificate: on the final tree the restatement finds no move within the radius that gains more than min_gain
    gains = restated_candidates(c, r["parent"], r["blen"], radius)
    assert gains and max(g[0] for g in gains) <= MIN_GAIN, gains
    want = RefTree(r["parent"], c.seq, c.rm).messages(r["blen"]).loglik()
    assert abs(r["ll_final"] - want) <= SCORE_BAR * abs(want)


def test_search_recovers_the_tree_the_alignment_came_from_host():
    c = spr_search_case()
    # the start is strictly worse than the true topology, both with fitted lengths, by the restatement
    fit = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)
    tru = E.tree_optimize_lengths(c.true_parent, np.where(c.true_parent >= 0, 0.1, 0.0), c.seq, c.md, host=True)
    assert RefTree(c.parent, c.seq, c.rm).messages(fit["blen"]).loglik() < RefTree(c.true_parent, c.seq, c.rm).messages(tru["blen"]).loglik() - 1.0
    assert bipartitions(c.parent, c.start, c.names).keys() != bipartitions(c.true_parent, c.true_blen, c.names).keys()
    # no chain of improving NNIs need lead back: the SPR search does
    r = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True)
    print(r["stop"], r["rounds"], r["moves"], r["ll_start"], r["ll_final"])
    assert r["ll_start"] == fit["ll_final"] and len(r["moves"]) >= 1 and max(m[4] for m in r["moves"]) >= 2
    check_search(c, r, 4, need_truth=True)
    again = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True, mem_budget=1 << 40, slab=1)
    assert np.array_equal(again["parent"], r["parent"]) and np.array_equal(again["blen"], r["blen"]) and again["moves"] == r["moves"]
    one = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True, spr_rounds=1)
    assert one["stop"] == "max rounds" and one["rounds"] == r["rounds"][:1] and one["ll_final"] >= one["rounds"][0]["ll"]


def first_round(c, radius):
    fit = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)
    sc = E.tree_spr_scores(c.parent, fit["blen"], c.seq, c.md, radius=radius, host=True)
    return fit, sc, restated_selection(c.parent, sc)


def test_of_two_candidates_whose_paths_share_a_node_only_the_better_is_taken():
    c = spr_search_case()
    fit, sc, (cand, taken) = first_round(c, 4)
    assert len(cand) >= 2 and len(taken) < len(cand)
    dropped = [x for x in cand if x not in taken][0]
    better = [x for x in taken if cand.index(x) < cand.index(dropped) and marked_by(c.parent, x[1], x[2]) & marked_by(c.parent, dropped[1], dropped[2])]
    assert better and better[0][0] >= dropped[0]
    r = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True, spr_rounds=1)
    first = r["rounds"][0]
    assert (first["candidates"], first["taken"]) == (len(cand), len(taken)) and first["pruned"] == len(sc["prune_node"]) and first["targets"] == len(sc["target_node"])
    assert [m[1:] for m in r["moves"]] == [(x[1], prune_parts(c.parent, x[1])["s"], x[2], x[3]) for x in taken[:first["applied"]]]


def test_two_candidates_with_disjoint_paths_are_both_applied():
    c = spr_search_case(two=True)
    fit, sc, (cand, taken) = first_round(c, 4)
    assert len(taken) >= 2 and not marked_by(c.parent, taken[0][1], taken[0][2]) & marked_by(c.parent, taken[1][1], taken[1][2])
    r = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True)
    first = r["rounds"][0]
    assert first["taken"] == len(taken) and first["applied"] == len(taken) and [m[1] for m in r["moves"][:len(taken)]] == [x[1] for x in taken]
    check_search(c, r, 4, need_truth=True)


HALVING_RADIUS = 2
HALVING_PARENT = [-1, 0, 0, 2, 3, 4, 4, 3, 2, 8, 8, 0, 11, 12, 12, 11, 15, 15]
HALVING_ROWS = {1: 'CAAGGCGCTCGA-AAGGGATGATGAGC',
                5: 'TAACCCGCACGTAGG-G--G-GTTAGC',
                6: 'CAATC-CCACGC-AGG--ATAGATAGC',
                7: 'CAAGCCTCCT--A-GGGGGG-AGT-GG',
                9: 'CAAT-AGCGG--AAGCGGA-AGTTCTC',
                10: 'CCATTCGCAC-CCAGGGAAGACTTGAG',
                13: 'CAAGCCGGCGGTAAGG-GACTG-CAGC',
                14: 'CACGCAGG-GGTAAGGGCAGAATTACT',
                16: 'CTTTTCACACG-CAGAC--GAGTTAGC',
                17: 'G-AGCCGCATGTATGGTGGAAGA-AA-'}


def halving_case():
    c = Case()
    c.parent = np.array(HALVING_PARENT, np.int32); c.min_len, c.max_len = 0.0, 10.0
    c.sm = synth.load_model("HKY85"); c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par); c.rm = RefModel(c.sm)
    L = len(next(iter(HALVING_ROWS.values())))
    c.seq = np.full((len(c.parent), L), -2, np.int8)
    for u, row in HALVING_ROWS.items():
        c.seq[u] = ["ACGT".index(x) if x != "-" else -2 for x in row]
    c.names = ["s%d" % u if u in HALVING_ROWS else "" for u in range(len(c.parent))]
    c.start = np.where(c.parent >= 0, 0.1, 0.0)
    return c


def test_a_rejected_set_of_moves_is_halved_host():
    """ten leaves, 27 columns (found by a search over random short alignments): two moves with disjoint paths are taken; applied together they lower the
    log-likelihood, and the better one alone is applied"""
    c = halving_case()
    r = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=HALVING_RADIUS, host=True)
    first = r["rounds"][0]
    assert first["taken"] >= 2 and first["applied"] < first["taken"], first
    fit, sc, (cand, taken) = first_round(c, HALVING_RADIUS)
    assert len(taken) == first["taken"] and [m[1] for m in r["moves"] if m[0] == 1] == [x[1] for x in taken[:first["applied"]]]
    # the taken moves at once are worse than the fitted start, by the restatement on the really rearranged tree
    par, bl = c.parent, fit["blen"]
    for g, v, w, d, t in taken:
        par, bl = moved(par, bl, prune_parts(par, v), w, t)
    assert RefTree(par, c.seq, c.rm).messages(bl).loglik() < RefTree(c.parent, c.seq, c.rm).messages(fit["blen"]).loglik()
    lls = [r["ll_start"]] + [x["ll"] for x in r["rounds"]]
    assert all(b > a for a, b in zip(lls, lls[1:])) and r["ll_final"] >= lls[-1]


def test_nni_and_spr_from_the_programs_own_nj_tree_host():
    c = nj_search_case()
    nni = E.tree_nni_search(c.parent, c.start, c.seq, c.md, child_off=c.child_off, child_idx=c.child_idx, host=True)
    r = E.tree_spr_search(nni["parent"], nni["blen"], c.seq, c.md, child_off=nni["child_off"], child_idx=nni["child_idx"], radius=3, host=True)
    print(r["stop"], r["rounds"], r["moves"])
    assert r["ll_final"] >= nni["ll_final"] - SCORE_BAR * abs(nni["ll_final"])
    cc = Case(); cc.__dict__.update(c.__dict__); cc.parent = nni["parent"]
    check_search(cc, r, 3, need_truth=False)


def test_no_dependence_on_the_budget_or_the_slab_host():
    c = spr_cases()[6]
    a = far_scores(c, True)
    n, L = c.seq.shape
    for kw in (dict(slab=1), dict(slab=7), dict(mem_budget=E.spr_need(n, L, FAR)), dict(mem_budget=1 << 40, slab=3)):
        b = scores(c, True, FAR, **kw)
        assert all(np.array_equal(a[k], b[k]) for k in a if k != "skipped") and a["skipped"] == b["skipped"], kw


def test_entries_refuse_what_the_header_says():
    c = spr_cases()[3]
    dg = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.4, 1.0, 2.5])
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_spr_scores(c.parent, c.start, c.seq, dg, host=True)
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_spr_search(c.parent, c.start, c.seq, dg, host=True)
    for kw in (dict(radius=0), dict(radius=33), dict(slab=-1)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_spr_scores(c.parent, c.start, c.seq, c.md, host=True, **kw)
    for kw in (dict(spr_rounds=0), dict(min_gain=0.0), dict(min_gain=-1.0), dict(min_gain=float("nan")), dict(eps=1e-7), dict(max_rounds=0), dict(radius=0),
               dict(radius=33)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_spr_search(c.parent, c.start, c.seq, c.md, host=True, **kw)
    n, L = c.seq.shape
    for fn in (E.tree_spr_search, E.tree_spr_scores):
        with pytest.raises(E.EngineError, match=r"error -4: .*need (\d+) bytes .*budget is 1048576 bytes") as ei:
            fn(c.parent, c.start, c.seq, c.md, host=True, mem_budget=1 << 20, radius=2)
        assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) == E.spr_need(n, L, 2)
    # hu_blen_need plus 32 bytes per node, 96 per target and the scratch of the workgroups
    assert E.spr_need(n, L, 2) == E.blen_need(n, L) + (n - 1) * (32 + 96 * min(13, n) + 2 * 32 * L)
    big = E.BLEN_LDS_COLS + 1
    assert E.spr_need(n, big, 1) == E.blen_need(n, big) + (n - 1) * (32 + 96 * 5 + 32 * big + 24 * big)
    assert E.spr_need(1000, 60000, 32) == E.blen_need(1000, 60000) + 999 * 32 + (1 << 26) + (1 << 30)
    assert E.spr_need(n, L, 0) == 0 and E.spr_need(n, L, 33) == 0


# ---- 6. the program ----

def program_case(tmp_path):
    c = spr_search_case()
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
    assert lines[0] == "round\tll\tpruned\ttargets\tcandidates\ttaken\tapplied"
    assert re.fullmatch(r"# stop: (local optimum|no improving move|max rounds)", lines[-2]) and re.fullmatch(r"# skipped: \d+ nodes", lines[-1])
    rows = [x.split("\t") for x in lines[1:-2]]
    assert [int(x[0]) for x in rows] == list(range(len(rows))) and rows[0][2:] == ["0"] * 5 and all(len(x) == 7 for x in rows)
    ll = [float(x[1]) for x in rows]
    assert all(b > a for a, b in zip(ll, ll[1:]))
    return rows, lines[-2][8:]


def test_program_spr_with_a_start_tree_and_without(tmp_path):
    c, fa, tree = program_case(tmp_path)
    out, log = tmp_path / "out.tree", tmp_path / "spr.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--spr", "--spr-radius", 4, "--start-tree", tree, "-o", out, "--spr-log", log, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"SPR search: log-likelihood -\d+\.\d+ -> -\d+\.\d+, \d+ move\(s\) applied in \d+ round\(s\) at radius 4, stop: local optimum", r.stderr), r.stderr
    assert re.search(r"round 1: the subtree of node \d+ from the edge of node \d+ into the edge of node \d+, distance \d+", r.stderr)
    assert re.search(r"SPR fits \S+ s, scoring \S+ s, trials \S+ s", r.stderr)
    want = E.tree_spr_search(c.parent, np.array([float("%.6g" % x) for x in c.start]), c.seq, c.md, radius=4, host=True)
    rows, stop = read_log(log)
    assert stop == "local optimum" and len(rows) - 1 == len(want["rounds"])
    assert [float(x[1]) for x in rows[1:]] == [x["ll"] for x in want["rounds"]] and float(rows[0][1]) == want["ll_start"]
    assert [[int(v) for v in x[2:]] for x in rows[1:]] == [[x["pruned"], x["targets"], x["candidates"], x["taken"], x["applied"]] for x in want["rounds"]]
    back = E.newick_parse(out.read_text())
    assert back["names"][0] == "top"                            # the top node stays
    a, b = bipartitions(back["parent"], back["blen"], back["names"]), bipartitions(want["parent"], want["blen"], c.names)
    assert a.keys() == b.keys() == bipartitions(c.true_parent, c.true_blen, c.names).keys()
    assert all(abs(a[k] - b[k]) <= 4e-16 * b[k] for k in a)
    # from the joins, with the interchanges before and after, and the supports of the result
    out2, log2, nlog = tmp_path / "nj.tree", tmp_path / "nj.log", tmp_path / "nni.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--nni", "--spr", "-o", out2, "--spr-log", log2, "--nni-log", nlog, "--spr-rounds", 5,
              "--spr-min-gain", "0.01", "--support", 50, "-v"])
    assert r.returncode == 0, r.stderr
    assert r.stderr.index("NNI search:") < r.stderr.index("SPR search:") < r.stderr.index("Local supports:")
    read_log(log2)
    t2 = E.newick_parse(out2.read_text())
    only = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--nni", "-o", tmp_path / "nni.tree", "-v"])
    assert only.returncode == 0
    ll = lambda text: float(re.findall(r"search[^:]*: log-likelihood \S+ -> (-\d+\.\d+),", text)[-1])
    assert ll(r.stderr) >= ll(only.stderr)
    t1 = E.newick_parse((tmp_path / "nni.tree").read_text())
    assert sorted(x for x in t1["names"] if x) == sorted(x for x in t2["names"] if x and not re.fullmatch(r"[01]\.\d{3}", x))
    assert any(re.fullmatch(r"[01]\.\d{3}", x) for x in t2["names"])


def test_program_without_spr_writes_what_the_parent_commit_wrote(tmp_path):
    """70_otus on the host path against the files of tests/golden/tree_blen"""
    for model in ("JC69", "GTR"):
        out = tmp_path / ("nj_%s.tree" % model)
        r = _run([_bin(), FASTA70, "--host", "-o", out] + ([] if model == "JC69" else ["-sm", sm(model)]))
        assert r.returncode == 0, r.stderr
        with open(os.path.join(ROOT, "tests", "golden", "tree_blen", "70_otus_nj_host_%s.tree" % model), "rb") as f:
            assert out.read_bytes() == f.read()


def test_program_spr_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, fa, tree = program_case(tmp_path)
    ml = ["-sm", sm("HKY85"), "--ml-lengths"]
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa, "-sm", sm("HKY85"), "--spr"], "--spr goes with --ml-lengths"),
                      ([fa] + ml + ["--spr-radius", "3"], "go with --spr"),
                      ([fa] + ml + ["--spr-rounds", "3"], "go with --spr"),
                      ([fa] + ml + ["--spr-min-gain", "0.1"], "go with --spr"),
                      ([fa] + ml + ["--spr-log", tmp_path / "x.log"], "go with --spr"),
                      ([fa] + ml + ["--spr", "--spr-radius", "0"], "--spr-radius"),
                      ([fa] + ml + ["--spr", "--spr-radius", "33"], "--spr-radius"),
                      ([fa] + ml + ["--spr", "--spr-rounds", "0"], "--spr-rounds"),
                      ([fa] + ml + ["--spr", "--spr-min-gain", "0"], "--spr-min-gain"),
                      ([fa] + ml + ["--spr", "--spr-min-gain", "-1"], "--spr-min-gain"),
                      ([fa] + ml + ["--spr", "--mem", "0.0001"], r"--spr: .*need \d+ bytes .* --mem allows 100000 bytes"),
                      ([fa] + ml + ["--nni", "--spr", "--mem", "0.0001", "--start-tree", tree], r"need \d+ bytes .* --mem allows 100000 bytes")):
        r = _run([_bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


# ---- 7. the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_spr_host.cpp, hu_nni_host.cpp and hu_blen_host.cpp (no HIP headers) with tests/san/spr_driver.cpp under AddressSanitizer +
    UBSan, run as a stand-alone program: the walks, the scores at three radii and slabs, apply with its refusals and a short search"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "spr_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "spr_driver.cpp"), os.path.join(CSRC, "hu_spr_host.cpp"), os.path.join(CSRC, "hu_nni_host.cpp"),
                        os.path.join(CSRC, "hu_blen_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "slabs agree" in r.stdout and "refusals: 5" in r.stdout and "searches: 2" in r.stdout


# ---- the device ----

def device_case(n_leaves, L):
    def make():
        rng = np.random.default_rng(2000 * n_leaves + L)
        kind = (n_leaves + L) % 3
        parent = (build_tree(n_leaves, rng, top=2) if kind == 1 or n_leaves < 5 else random_tree(n_leaves, rng) if kind == 2 and n_leaves >= 9
                  else build_tree(n_leaves, rng, top=3))
        return make_case(parent, L, ("JC69", "HKY85", "GTR")[(n_leaves + L) % 3], 200 * n_leaves + L, random_leaf=n_leaves >= 5,
                         max_len=2.0 if n_leaves >= 5 else 10.0)
    return cached(("dev", n_leaves, L), make)


DEVICE_SHAPES = [(4, 1, 1), (6, 63, 2), (6, 64, 2), (9, 65, 3), (33, 257, 3), (12, E.BLEN_LDS_COLS, 2), (12, E.BLEN_LDS_COLS + 1, 2), (33, 255, 32),
                 (130, 1000, 3)]


def restated_too(c, n_leaves, L):
    """the device shapes that are also held against the restatement: the small ones, and the 12 leaves on either side of the switch of the
    ratios, whose sums are the longest of this file"""
    return L > 1 and (len(c.parent) * L <= 6000 or n_leaves == 12)


def test_the_devices_shapes_hold_the_root_cases_and_the_host_path_meets_the_bar_on_them():
    met, worst = set(), 0.0
    for n_leaves, L, radius in DEVICE_SHAPES:
        c = device_case(n_leaves, L)
        want, skipped = prunable(c.parent)
        assert want, (n_leaves, L)
        root_kids = len(c.kids[0])
        met |= {"g is the root, %d children" % root_kids for e in want if e["g"] == 0} | {"g is not the root" for e in want if e["g"] != 0}
        if any(len(k) >= 4 for k in c.kids):
            met.add("polytomy")
        if restated_too(c, n_leaves, L):
            worst = max(worst, check_scores(c, scores(c, True, radius), radius)[0])
    print("largest deviation of the host path's f on the device's shapes: %.3g" % worst)
    assert met >= {"g is the root, 2 children", "g is the root, 3 children", "g is not the root", "polytomy"} and worst <= F_BAR


@pytest.mark.gpu
def test_scores_and_optima_against_the_restatement_device():
    """measured: DEVICE_WORST"""
    _need_gpu()
    worst = run_restatement(host=False)
    print("largest deviation of the device's f: %.3g" % worst)
    check_impossible(False)
    assert worst <= F_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L,radius", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L, radius):
    """the edges of a thread's stride (256 columns) and of a wave, one column, the column counts on either side of the switch from ratios
    in LDS to ratios in global memory, a radius beyond the tree: the same targets in the same order, t* within 2 tau of the host path's, f
    under the bar, the same bits twice"""
    _need_gpu()
    c = device_case(n_leaves, L)
    host, dev, again = scores(c, True, radius), scores(c, False, radius), scores(c, False, radius)
    assert len(host["prune_node"]) > 0 and len(host["target_node"]) > 0
    for k in dev:
        assert np.array_equal(dev[k], again[k]), k
    for k in ("prune_node", "v_off", "target_node", "dist"):
        assert np.array_equal(dev[k], host[k]), k
    assert dev["skipped"] == host["skipped"]
    gap = max(np.abs(dev["t_star"] - host["t_star"]).max(), np.abs(dev["base_t"] - host["base_t"]).max())
    worst = max(np.abs((dev[k] - host[k]) / host[k]).max() for k in ("f", "base_f", "f_at_blen"))
    print("n %d L %d radius %d: largest |t* device - t* host| %.3g, largest deviation of f %.3g" % (n_leaves, L, radius, gap, worst))
    assert gap <= 2 * TAU and worst <= F_BAR
    if restated_too(c, n_leaves, L):
        w = check_scores(c, dev, radius)[0]
        print("n %d L %d radius %d: largest deviation of the device's f from the restatement %.3g" % (n_leaves, L, radius, w))
        assert w <= F_BAR


@pytest.mark.gpu
def test_a_slab_of_one_prune_node_gives_the_bits_of_the_default_slab():
    _need_gpu()
    for n_leaves, L, radius in ((33, 257, 3), (12, E.BLEN_LDS_COLS + 1, 2)):
        c = device_case(n_leaves, L)
        a, b, d = scores(c, False, radius), scores(c, False, radius, slab=1), scores(c, False, radius, slab=5)
        for k in a:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], d[k]), k


@pytest.mark.gpu
def test_search_on_the_device():
    _need_gpu()
    c = spr_search_case()
    host = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4, host=True)
    # no two gains of one pruned node and no two candidates of a round within 1e-6 of each other, by the host scores: a differing last bit
    # cannot reorder them
    par, bl = c.parent, c.start
    for rnd in range(len(host["rounds"])):
        fit = E.tree_optimize_lengths(par, bl, c.seq, c.md, host=True)
        sc = E.tree_spr_scores(par, fit["blen"], c.seq, c.md, radius=4, host=True)
        for i in range(len(sc["prune_node"])):
            f = np.sort(sc["f"][sc["v_off"][i]:sc["v_off"][i + 1]])
            if len(f) >= 2 and f[-1] - sc["base_f"][i] > MIN_GAIN / 2:
                assert f[-1] - f[-2] > 1e-6, (rnd, sc["prune_node"][i])
        cand, taken = restated_selection(par, sc, MIN_GAIN / 2)
        gain = np.sort([x[0] for x in cand])
        assert len(gain) > 0 and (len(gain) < 2 or np.diff(gain).min() > 1e-6) and np.abs(gain - MIN_GAIN).min() > 1e-6, gain
        bl = fit["blen"]
        for r_, v, w_from, w, d in [m for m in host["moves"] if m[0] == rnd + 1]:
            t = [x[4] for x in cand if x[1] == v and x[2] == w][0]
            a = E.tree_spr_apply(par, bl, v, w, t)
            par, bl = a["parent"], a["blen"]
    dev = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=4)
    assert dev["moves"] == host["moves"] and dev["stop"] == host["stop"] and np.array_equal(dev["parent"], host["parent"])
    assert abs(dev["ll_final"] - host["ll_final"]) <= F_BAR * abs(host["ll_final"])
    check_search(c, dev, 4, need_truth=True)


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    _need_gpu()
    c = spr_cases()[4]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.spr_need(n, L, 3)):
        E.tree_spr_scores(c.parent, c.start, c.seq, c.md, radius=3, mem_budget=1 << 20)


@pytest.mark.gpu
def test_tree_spr_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree --ml-lengths --nni --spr -> hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm on 70_otus: a database that
    loads"""
    _need_gpu()
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "--ml-lengths", "--nni", "--nni-rounds", 2, "--spr", "--spr-rounds", 1, "--spr-radius", 3, "--ml-rounds", 5,
              "-o", "spr.tree", "--spr-log", "spr.log", "-v"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "NNI search" in r.stderr and "SPR search" in r.stderr
    rows, stop = read_log(tmp_path / "spr.log")
    print(rows, stop)
    r = _run([_bin("hmmufotu-amd-train-sm"), FASTA70, "spr.tree", "-o", "spr.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), FASTA70, "spr.tree", "--no-hmm", "-sm", "spr.sm", "-n", "sprdb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "sprdb.ptu"))
    assert (np.asarray(db["parent"]) < 0).sum() == 1
