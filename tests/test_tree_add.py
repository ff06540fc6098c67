"""hmmufotu-amd-tree --ml-lengths --start-tree T --add: new sequences inserted into a start tree.

The yardstick is a restatement that shares no code with the library: the two nodes p and v of an insertion are really appended on the
parent array, the grown tree is pruned by RefTree (tests/test_tree_blen.py: float64 in linear space, math.fsum over the columns), and
the pendant's f, f' and, by bisection on f', its optimum are taken on that tree.  So f_{w,r}(t) is held to what it claims to be: the
log-likelihood of the tree with r inserted at w.

The bar of f is made the project's way: the largest deviation |f - restated f| / |f| measured over all cases of this file is
HOST_WORST on the host path and DEVICE_WORST on the MI355X; four times the larger, rounded up to a power of two, is F_BAR.
"""
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
from test_tree_nni import (Case, bipartitions, build_tree, cases, kids_of, make_case, simulate, star_case, tree_loglik_host,  # noqa: E402
                           FASTA70)
from test_tree_spr import impossible_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")

TAU = E.BLEN_TAU
HOST_WORST = 1.32e-14       # measured: the host path, 5 leaves x 1,450 columns (its serial sums); 1.48e-15 over add_cases()
DEVICE_WORST = 1.17e-15     # measured: MI355X, 3 leaves x 1 column; 1.08e-15 over add_cases()
F_BAR = 2.0 ** -44          # 4 x 1.32e-14 = 5.28e-14, rounded up to a power of two: 5.68e-14; section 25's 2^-45 was the expectation
assert 4 * max(HOST_WORST, DEVICE_WORST) <= F_BAR <= 1e-10
TILE = E.ADD_TILE


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


# ---- the restatement ----

def grown(parent, blen, seq, w, row, t, kids=None):
    """the arrays with the row really inserted at w: p = n and v = n + 1 appended; the child lists by the rule of the header"""
    parent = np.asarray(parent); n = len(parent)
    assert 0 <= w < n and parent[w] >= 0
    par = np.concatenate([parent, [parent[w], n]]).astype(np.int32)
    par[w] = n
    bl = np.concatenate([np.asarray(blen, float), [0.5 * blen[w], t]])
    bl[w] = 0.5 * blen[w]
    sq = np.concatenate([np.asarray(seq, np.int8), np.full((1, seq.shape[1]), -2, np.int8), np.asarray(row, np.int8)[None, :]])
    out = dict(parent=par, blen=bl, seq=sq)
    if kids is not None:
        k2 = [list(k) for k in kids] + [[w, n + 1], []]
        pw = int(parent[w])
        k2[pw][k2[pw].index(w)] = n
        out["kids"] = k2
    return out


class Pendant:
    """the objective of the pendant of row hung into the middle of the edge above w, on the really grown tree"""

    def __init__(self, c, blen, w, row):
        g = grown(c.parent, blen, c.seq, w, row, 0.1)
        self.v = len(c.parent) + 1
        self.L = c.seq.shape[1]
        self.m = c.rm
        self.t = RefTree(g["parent"], g["seq"], c.rm).messages(g["blen"])

    def f(self, t):
        return self.t.branch(self.v, t)[0]

    def slope(self, t):
        return self.t.slope(self.v, t)

    def optimum(self, lo, hi):
        return self.t.optimum(self.v, lo, hi)


def check_t_star(a, t, lo, hi, what):
    """§22's rule: the restated slope changes sign within 2 tau of t, or the end of the interval is justified.  A slope that is 0 in exact
    arithmetic (a row of gaps only has a flat f) comes out within 4 x 2^-52 x max |lambda| x columns of 0"""
    noise = 4 * 2.0 ** -52 * np.abs(a.m.lam).max() * a.L
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


def mean_len(parent, blen, lo, hi):
    x = [float(blen[u]) for u in range(len(parent)) if parent[u] >= 0]
    return min(max(sum(x) / len(x), lo), hi)


# ---- the inputs ----

def with_rm(c):
    if not hasattr(c, "rm"):
        c.rm = RefModel(c.sm)
    return c


def queries_of(c, seed):
    """four queries: the row of an existing leaf, a row of gaps only, a leaf's row with a tenth of its bases changed and 5 % gaps, a row of
    random bases"""
    rng = np.random.default_rng(seed)
    L = c.seq.shape[1]
    c.twin = c.leaves[1]
    near = np.array(c.seq[c.leaves[-2 if c.leaves[-2] != c.twin else 0]])
    hit = rng.random(L) < 0.1
    near[hit] = rng.integers(0, 4, L)[hit]
    near[rng.random(L) < 0.05] = -2
    return np.ascontiguousarray(np.stack([c.seq[c.twin], np.full(L, -2), near, rng.integers(0, 4, L)]), np.int8)


def add_cases():
    """3, 4, 6, 12 and 33 leaves under JC69, HKY85 and GTR: the trees of tests/test_tree_nni.py (a trifurcating top node, a bifurcating root
    with two inner children and with a leaf child, a node with four children, 5 % gaps, a column of gaps; max_len 2 in two of them) and the
    star of three leaves"""
    def make():
        out = []
        for i, c in enumerate([star_case()] + list(cases())):
            c = with_rm(c)
            c.q = queries_of(c, 100 + i)
            out.append(c)
        return out
    return cached("add", make)


def scores(c, host, blen=None, q=None, **kw):
    return E.tree_add_scores(c.parent, c.start if blen is None else blen, c.seq, c.q if q is None else q, c.md, min_len=c.min_len, max_len=c.max_len,
                             host=host, **kw)


def check_scores(c, got, q=None, blen=None):
    """every (query, edge) against the really grown tree; the largest deviation of f and what was met"""
    q = c.q if q is None else q; blen = c.start if blen is None else blen
    n = len(c.parent); root = int(np.nonzero(np.asarray(c.parent) < 0)[0][0])
    assert got["t_star"].shape == got["f"].shape == (len(q), n)
    worst, met = 0.0, set()
    for r in range(len(q)):
        assert got["t_star"][r, root] == 0.0 and got["f"][r, root] == -np.inf
        best = None
        for w in range(n):
            if w == root:
                continue
            a = Pendant(c, blen, w, q[r])
            t, f = got["t_star"][r, w], got["f"][r, w]
            assert np.isfinite(f) and not np.isnan(t), (c.name, r, w)
            met.add(check_t_star(a, t, c.min_len, c.max_len, (c.name, r, w, t)))
            worst = max(worst, rel(f, a.f(t)))
            if best is None or f > got["f"][r, best]:
                best = w
        assert got["best_w"][r] == best and got["best_f"][r] == got["f"][r, best] and got["best_t"][r] == got["t_star"][r, best], (c.name, r)
    return worst, met


# ---- 1. the scores ----

def run_restatement(host):
    worst, met = 0.0, set()
    for c in add_cases():
        got = scores(c, host)
        w, m = check_scores(c, got)
        print("%s: largest deviation of f %.3g, met %s" % (c.name, w, sorted(m)))
        worst = max(worst, w); met |= m
        kids = kids_of(c.parent)
        # the query equal to a leaf: its best edge is that leaf's or touches it, and the pendant is at min_len
        u, p = c.twin, int(c.parent[c.twin])
        touch = {u, p} | set(kids[p]) | ({x for x in kids[int(c.parent[p])]} if c.parent[p] >= 0 else set())
        assert int(got["best_w"][0]) in touch and got["best_t"][0] == c.min_len, (c.name, got["best_w"][0], got["best_t"][0])
        # the query of gaps only: a flat objective, every edge the tree's own log-likelihood, no NaN
        assert not np.isnan(got["f"][1]).any() and not np.isnan(got["t_star"][1]).any()
    assert {"min", "inner", "max"} <= met, met
    return worst


def test_scores_and_optima_against_the_really_grown_tree_host():
    """measured: HOST_WORST"""
    worst = run_restatement(host=True)
    print("largest deviation of the host path's f: %.3g" % worst)
    assert worst <= F_BAR


def check_impossible(host):
    """a column made impossible by two sisters on branches of length 0: -inf on every edge, never NaN"""
    c = with_rm(impossible_case())
    q = queries_of(c, 7)
    got = scores(c, host, q=q)
    root = 0
    assert not np.isnan(got["f"]).any() and not np.isnan(got["t_star"]).any()
    assert (got["f"] == -np.inf).all()
    assert (got["best_w"] == min(w for w in range(len(c.parent)) if w != root)).all() and (got["best_f"] == -np.inf).all()
    assert ((got["t_star"] >= c.min_len) | (np.arange(len(c.parent)) == root)[None, :]).all() and (got["t_star"] <= c.max_len).all()


def test_a_column_of_likelihood_zero_gives_minus_infinity_host():
    check_impossible(True)


def test_the_start_of_every_pendant_is_the_mean_length():
    """a flat objective (the row of gaps only) stays where it starts when f' is exactly 0 there, else at an end: under JC69 both ends'
    slopes are rounding noise, so only the interval is held; the start itself shows in a tree whose every branch has one length"""
    c = add_cases()[1]
    bl = np.where(c.parent >= 0, 0.25, 0.0)
    assert mean_len(c.parent, bl, 0.0, 10.0) == 0.25 and mean_len(c.parent, bl, 0.0, 0.2) == 0.2 and mean_len(c.parent, bl, 0.5, 10.0) == 0.5


# ---- 2. apply ----

def test_apply_gives_the_restated_arrays_and_the_predicted_loglik():
    for c in add_cases()[1:]:
        got = scores(c, True)
        kids = kids_of(c.parent)
        off, idx = E._child_arrays(c.parent, None, None)
        names = ["" if kids[u] else "s%d" % u for u in range(len(kids))]
        n = len(c.parent)
        for r in (0, 2, 3):
            for w in sorted({int(got["best_w"][r]), n - 1, 1}):
                t = float(got["t_star"][r, w])
                a = E.tree_add_apply(c.parent, c.start, w, t, off, idx, min_len=c.min_len, max_len=c.max_len)
                want = grown(c.parent, c.start, c.seq, w, c.q[r], t, kids)
                assert np.array_equal(a["parent"], want["parent"]) and np.array_equal(a["blen"], want["blen"]), (c.name, r, w)
                got_kids = [list(a["child_idx"][a["child_off"][u]:a["child_off"][u + 1]]) for u in range(n + 2)]
                assert got_kids == want["kids"], (c.name, r, w)
                # still a tree, with the old leaves plus one
                assert (a["parent"] < 0).sum() == 1 and int(np.nonzero(a["parent"] < 0)[0][0]) == int(np.nonzero(c.parent < 0)[0][0])
                k2 = kids_of(a["parent"])
                order = [int(np.nonzero(a["parent"] < 0)[0][0])]
                for u in order:
                    order += k2[u]
                assert sorted(order) == list(range(n + 2))
                assert [u for u in range(n + 2) if not k2[u]] == [u for u in range(n) if not kids[u]] + [n + 1]
                # the predicted f is the log-likelihood of the grown tree
                cc = Case(); cc.seq = want["seq"]; cc.md = c.md
                ll = tree_loglik_host(a["parent"], a["blen"], cc)
                assert rel(ll, got["f"][r, w]) <= F_BAR, (c.name, r, w, ll, got["f"][r, w])
                # the Newick round trip, the order of children included
                text = E.newick_from_arrays(a["parent"], a["child_off"], a["child_idx"], names + ["", "new"], a["blen"])
                back = E.newick_parse(text)
                ident = {}
                def walk(x, y):
                    ident[x] = y
                    assert len(want["kids"][x]) == len(back["children"][y])
                    for cx, cy in zip(want["kids"][x], back["children"][y]):
                        walk(cx, int(cy))
                walk(int(np.nonzero(c.parent < 0)[0][0]), int(np.nonzero(back["parent"] < 0)[0][0]))
                assert len(ident) == n + 2
                for x, y in ident.items():
                    assert back["names"][y] == (names + ["", "new"])[x] and (a["parent"][x] < 0 or back["blen"][y] == a["blen"][x])


def test_apply_refuses_what_the_header_says():
    c = add_cases()[3]
    n = len(c.parent)
    for w, t, msg in ((0, 0.1, "names no edge"), (-1, 0.1, "names no edge"), (n, 0.1, "names no edge"), (1, -0.1, "outside"), (1, 10.5, "outside"),
                      (1, float("nan"), "outside")):
        with pytest.raises(E.EngineError, match="error -1: .*" + msg):
            E.tree_add_apply(c.parent, c.start, w, t)
    with pytest.raises(E.EngineError, match="error -1: .*outside"):
        E.tree_add_apply(c.parent, c.start, 1, 1.5, min_len=0.0, max_len=1.0)
    assert len(E.tree_add_apply(c.parent, c.start, 1, 1.0, min_len=0.0, max_len=1.0)["parent"]) == n + 2


# ---- 3. the search ----

SEARCH_SEED = 2026


def restrict(parent, blen, drop):
    """the tree without the leaves `drop`: a node left with one child goes and its child takes both lengths; ids in preorder.
    Returns parent, blen and old id -> new id"""
    kids = kids_of(parent)
    root = int(np.nonzero(np.asarray(parent) < 0)[0][0])

    def build(u):
        if not kids[u]:
            return None if u in drop else (u, blen[u], [])
        sub = [x for x in (build(v) for v in kids[u]) if x is not None]
        if not sub:
            return None
        if len(sub) == 1 and u != root:
            v, t, k = sub[0]
            return (v, t + blen[u], k)
        return (u, blen[u], sub)
    top = build(root)
    par, bl, ident = [], [], {}
    stack = [(top, -1)]
    while stack:
        (u, t, sub), p = stack.pop()
        ident[u] = len(par); par.append(p); bl.append(t if p >= 0 else 0.0)
        for x in reversed(sub):
            stack.append((x, ident[u]))
    return np.array(par, np.int32), np.array(bl), ident


def search_case():
    """an alignment of 600 columns simulated down a known tree of 12 leaves (trifurcating top node, HKY85, lengths 0.05 to 0.2); four leaves
    are removed, two of them sisters; the start tree is the true tree restricted to the other eight"""
    def make():
        rng = np.random.default_rng(SEARCH_SEED)
        c = Case()
        c.name = "add search"
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
        c.true_names = ["" if kids[u] else "s%d" % u for u in range(n)]
        sis = [k for k in kids if len(k) == 2 and not kids[k[0]] and not kids[k[1]] and c.true_parent[c.true_parent[k[0]]] > 0]
        assert sis
        c.sisters = tuple(sis[0])
        near, grand = set(), int(c.true_parent[c.true_parent[c.sisters[0]]])     # the other two are no neighbours of the sisters
        todo = [grand]
        for u in todo:
            near.add(u); todo += kids[u]
        others = [u for u in range(n) if not kids[u] and u not in near]
        drop = sorted(list(c.sisters) + [others[1], others[-1]])
        c.drop = drop
        c.parent, bl, ident = restrict(c.true_parent, c.true_blen, set(drop))
        m = len(c.parent)
        c.seq = np.full((m, 600), -2, np.int8)
        c.names = [""] * m
        for u, i in ident.items():
            if not kids[u]:
                c.seq[i] = seq[u]; c.names[i] = c.true_names[u]
        c.q = np.ascontiguousarray(seq[drop], np.int8)
        c.qnames = [c.true_names[u] for u in drop]
        c.start = np.where(c.parent >= 0, 0.1, 0.0)
        c.truth = bipartitions(c.true_parent, c.true_blen, c.true_names).keys()
        return c
    return cached("search", make)


def restated_search(c):
    """the loop of the header with the restatement's scores; the fits are the library's host path, which tests/test_tree_blen.py holds to
    the restatement.  Returns the grown arrays, the names and the insertions (round, query, w, f)"""
    par, seq, names = np.array(c.parent), np.array(c.seq), list(c.names)
    bl = E.tree_optimize_lengths(par, c.start, seq, c.md, host=True)["blen"]
    left, log, rnd = list(range(len(c.q))), [], 0
    while left:
        rnd += 1
        cc = Case(); cc.parent, cc.seq, cc.rm = par, seq, c.rm
        best = {}
        for r in left:
            cand = []
            for w in range(len(par)):
                if par[w] < 0:
                    continue
                a = Pendant(cc, bl, w, c.q[r])
                t = a.optimum(c.min_len, c.max_len)
                cand.append((a.f(t), -w, t))
            f, mw, t = max(cand)
            best[r] = (f, -mw, t)
        take = []
        for r in left:
            rivals = [x for x in left if best[x][1] == best[r][1]]
            if max(rivals, key=lambda x: (best[x][0], -x)) == r:
                take.append(r)
        for r in take:
            f, w, t = best[r]
            g = grown(par, bl, seq, w, c.q[r], t)
            par, bl, seq = g["parent"], g["blen"], g["seq"]
            names += ["", c.qnames[r]]
            log.append((rnd, r, w, f))
        left = [r for r in left if r not in take]
        bl = E.tree_optimize_lengths(par, bl, seq, c.md, host=True)["blen"]
    return par, bl, seq, names, log


def check_search(c, r):
    want = cached("restated search", lambda: restated_search(c))
    par, bl, seq, names, log = want
    # first: the restatement alone names the true position of every query
    assert bipartitions(par, bl, names).keys() == c.truth
    got_names = list(c.names) + [""] * (2 * len(c.q))
    for k, v in enumerate(r["query_node"]):
        got_names[v] = c.qnames[k]
    assert bipartitions(r["parent"], r["blen"], got_names).keys() == c.truth
    assert len(r["rounds"]) >= 2 and sum(x["inserted"] for x in r["rounds"]) == len(c.q) == len(r["inserts"])
    assert [x["scored"] for x in r["rounds"]][0] == len(c.q)
    assert [(i["round"], i["query"], i["w"]) for i in r["inserts"]] == [(a, b, w) for a, b, w, f in log]
    assert all(rel(i["f"], f) <= F_BAR for i, (a, b, w, f) in zip(r["inserts"], log))
    # exactly one of the sisters goes in in the first round: the one with the larger f
    sq = [c.drop.index(u) for u in c.sisters]
    first = [i for i in r["inserts"] if i["round"] == 1 and i["query"] in sq]
    assert len(first) == 1
    sc = E.tree_add_scores(c.parent, E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)["blen"], c.seq, c.q, c.md, host=True)
    assert sc["best_w"][sq[0]] == sc["best_w"][sq[1]]
    assert first[0]["query"] == max(sq, key=lambda k: sc["best_f"][k])
    # every name is carried, every leaf holds its row
    kids = kids_of(r["parent"])
    assert sorted(got_names[u] for u in range(len(kids)) if not kids[u]) == sorted(c.true_names[u] for u in range(len(c.true_names)) if c.true_names[u])
    assert all(not kids[v] and np.array_equal(r["seq"][v], c.q[k]) for k, v in enumerate(r["query_node"]))
    assert (r["parent"] < 0).sum() == 1 and r["parent"][0] < 0
    ll = RefTree(r["parent"], r["seq"], c.rm).messages(r["blen"]).loglik()
    assert abs(r["ll_final"] - ll) <= SCORE_BAR * abs(ll)
    assert r["rounds"][-1]["ll"] == r["ll_final"]


def host_search(c, **kw):
    return E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, host=True, **kw)


def test_search_puts_every_removed_leaf_back_host():
    c = search_case()
    check_search(c, cached("host search", lambda: host_search(c)))


def test_search_without_a_query_is_the_fit():
    c = search_case()
    r = E.tree_add_search(c.parent, c.start, c.seq, [], c.md, host=True)
    fit = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, host=True)
    assert np.array_equal(r["blen"], fit["blen"]) and r["ll_final"] == fit["ll_final"] and r["rounds"] == [] and np.array_equal(r["parent"], c.parent)


# ---- 4. the slab and the tile ----

def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("t_star", "f", "best_w", "best_t", "best_f"))


def test_no_dependence_on_the_slab_or_the_tile_host():
    c = add_cases()[5]
    a = scores(c, True)
    for kw in (dict(slab=1, tile=1), dict(slab=3, tile=2), dict(tile=64)):
        assert same_bits(a, scores(c, True, **kw)), kw
    s = search_case()
    x, y = cached("host search", lambda: host_search(s)), host_search(s, slab=1, tile=1)
    assert np.array_equal(x["parent"], y["parent"]) and np.array_equal(x["blen"], y["blen"]) and x["inserts"] == y["inserts"]


# ---- 5. the memory and the refusals ----

def test_entries_refuse_what_the_header_says():
    c = add_cases()[3]
    dg = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.4, 1.0, 2.5])
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_add_scores(c.parent, c.start, c.seq, c.q, dg, host=True)
    with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
        E.tree_add_search(c.parent, c.start, c.seq, c.q, dg, host=True)
    for kw in (dict(slab=-1), dict(tile=-1), dict(min_len=-1.0), dict(max_len=0.0)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_add_scores(c.parent, c.start, c.seq, c.q, c.md, host=True, **kw)
    for kw in (dict(eps=1e-7), dict(max_rounds=0), dict(tile=-2)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, host=True, **kw)
    bad = c.q.copy(); bad[2, 5] = 4
    with pytest.raises(E.EngineError, match="error -1: .*query 2 holds the code 4 at column 5"):
        E.tree_add_scores(c.parent, c.start, c.seq, bad, c.md, host=True)
    n, L = c.seq.shape
    q = len(c.q)
    with pytest.raises(E.EngineError, match=r"error -4: .*need (\d+) bytes .*budget is 1048576 bytes") as ei:
        E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, host=True, mem_budget=1 << 20)
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) == E.add_need(n + 2 * q, L, q)
    with pytest.raises(E.EngineError, match=r"error -4: .*need (\d+) bytes .*budget is 1048576 bytes") as ei:
        E.tree_add_scores(c.parent, c.start, c.seq, c.q, c.md, host=True, mem_budget=1 << 20)
    assert int(re.search(r"need (\d+) bytes", str(ei.value)).group(1)) == E.add_need(n, L, q)
    # the fit of the final tree, plus a launch: per tile 16 bytes per node and query, the rows and the records, the ratios beyond LDS
    assert E.add_need(n, L, q) == E.blen_need(n, L) + TILE * (16 * n + L + 24)
    assert E.add_need(n, L, 0) == E.blen_need(n, L) and E.add_need(n, L, 3 * TILE + 1) == E.blen_need(n, L) + 4 * TILE * (16 * n + L + 24)
    big = E.BLEN_LDS_COLS + 1
    assert E.add_need(n, big, TILE + 1) == E.blen_need(n, big) + 2 * (TILE * (16 * n + big + 24) + 24 * big * n)
    assert E.add_need(8191, 7682, 1024) == E.blen_need(8191, 7682) + (1 << 32)
    assert E.add_need(0, L, 1) == 0 and E.add_need(n, 0, 1) == 0 and E.add_need(n, L, -1) == 0


# ---- 6. the program ----

def program_case(tmp_path, full=True):
    c = search_case()
    kids = kids_of(c.parent)
    leaves = [u for u in range(len(kids)) if not kids[u]]
    # the rows of the MSA: the old leaves and the queries interleaved, the queries in the order of c.q
    names = [c.names[u] for u in leaves]; rows = [c.seq[u] for u in leaves]
    if full:
        for k, (nm, row) in enumerate(zip(c.qnames, c.q)):
            names.insert(2 * k + 1, nm); rows.insert(2 * k + 1, row)
    fa = tmp_path / ("in.fasta" if full else "old.fasta")
    write_fasta(fa, names, np.array(rows))
    tree = tmp_path / "start.tree"
    tn = list(c.names); tn[0] = "top"
    tree.write_text(to_newick(c.parent, kids, tn, c.start) + ";\n")
    return c, fa, tree


def read_log(path):
    lines = path.read_text().splitlines()
    assert lines[0] == "round\tll\tscored\tinserted" and lines[-1] == "# stop: all inserted"
    rows = [x.split("\t") for x in lines[1:] if not x.startswith("#")]
    ins = [x[len("# insert: "):].split("\t") for x in lines if x.startswith("# insert: ")]
    assert len(rows) + len(ins) + 2 == len(lines)
    assert [int(x[0]) for x in rows] == list(range(len(rows))) and rows[0][2:] == ["0", "0"] and all(len(x) == 4 for x in rows) and all(len(x) == 6 for x in ins)
    return rows, ins


def test_program_add_inserts_the_new_sequences(tmp_path):
    c, fa, tree = program_case(tmp_path)
    out, log = tmp_path / "out.tree", tmp_path / "add.log"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", tree, "--add", "--add-log", log, "-o", out, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"Sequences inserted: 4 in \d+ round\(s\), log-likelihood -\d+\.\d+ of the start tree, -\d+\.\d+ of the grown tree of %d nodes" % (len(c.parent) + 8), r.stderr)
    assert re.search(r"round 1: 4 scored, \d inserted, log-likelihood -\d+", r.stderr) and re.search(r"insertion sweeps \S+ s, scoring \S+ s, fits \S+ s", r.stderr)
    # the library on the arrays the program parses: the node ids are the parser's
    p = E.newick_parse(tree.read_text())
    row_of = {nm: c.seq[u] for u, nm in enumerate(c.names) if nm}
    seqp = np.full((len(p["parent"]), 600), -2, np.int8)
    for u, nm in enumerate(p["names"]):
        if len(p["children"][u]) == 0:
            seqp[u] = row_of[nm]
    want = E.tree_add_search(p["parent"], p["blen"], seqp, c.q, c.md, child_off=p["child_off"], child_idx=p["child_idx"], host=True)
    rows, ins = read_log(log)
    assert float(rows[0][1]) == want["ll_start"] and [float(x[1]) for x in rows[1:]] == [x["ll"] for x in want["rounds"]]
    assert [[int(x[2]), int(x[3])] for x in rows[1:]] == [[x["scored"], x["inserted"]] for x in want["rounds"]]
    assert [(int(x[0]), x[1], int(x[2]), int(x[3]), float(x[4]), float(x[5])) for x in ins] == \
        [(i["round"], c.qnames[i["query"]], i["v"], i["w"], i["t"], i["f"]) for i in want["inserts"]]
    back = E.newick_parse(out.read_text())
    assert back["names"][0] == "top" and len(back["parent"]) == len(c.parent) + 8
    assert bipartitions(back["parent"], back["blen"], back["names"]).keys() == c.truth
    assert E.newick_from_arrays(want["parent"], want["child_off"], want["child_idx"],
                                [dict(zip(want["query_node"].tolist(), c.qnames)).get(u, p["names"][u] if u < len(p["names"]) else "") for u in range(len(want["parent"]))],
                                want["blen"]) == out.read_text()
    # then the searches and the supports on the grown tree: every leaf is kept
    out2 = tmp_path / "all.tree"
    r = _run([_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", tree, "--add", "--nni", "--spr", "--support", 20, "-o", out2, "-v"])
    assert r.returncode == 0, r.stderr
    assert r.stderr.index("Sequences inserted:") < r.stderr.index("NNI search:") < r.stderr.index("SPR search:") < r.stderr.index("Local supports:")
    t2 = E.newick_parse(out2.read_text())
    k2 = kids_of(t2["parent"])
    assert sorted(t2["names"][u] for u in range(len(k2)) if not k2[u]) == sorted(x for x in c.true_names if x)


def test_program_add_without_a_new_sequence_is_the_run_without_the_flag(tmp_path):
    c, fa, tree = program_case(tmp_path, full=False)
    for extra in ([], ["--nni"], ["--spr", "--spr-radius", "2"]):
        a, b = tmp_path / "a.tree", tmp_path / "b.tree"
        head = [_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", tree] + extra
        r1, r2 = _run(head + ["-o", a]), _run(head + ["--add", "-o", b])
        assert r1.returncode == 0 and r2.returncode == 0, r1.stderr + r2.stderr
        assert a.read_bytes() == b.read_bytes() and r1.stderr == r2.stderr, extra
    log = tmp_path / "none.log"
    r = _run(head + ["--add", "--add-log", log, "-o", b])
    assert r.returncode == 0 and a.read_bytes() == b.read_bytes()
    rows, ins = read_log(log)
    assert len(rows) == 1 and ins == []


def test_program_add_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, fa, tree = program_case(tmp_path)
    ml = ["-sm", sm("HKY85"), "--ml-lengths"]
    extra = tmp_path / "extra.tree"
    kids = kids_of(c.parent)
    tn = list(c.names); tn[[u for u in range(len(kids)) if not kids[u]][0]] = "nobody"
    extra.write_text(to_newick(c.parent, kids, tn, c.start) + ";\n")
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa] + ml + ["--add"], "--add goes with --ml-lengths --start-tree"),
                      ([fa, "-sm", sm("HKY85"), "--add"], "--add goes with --ml-lengths --start-tree"),
                      ([fa, "-sm", sm("HKY85"), "--add", "--start-tree", tree], "--start-tree goes with --ml-lengths"),
                      ([fa] + ml + ["--start-tree", tree, "--add-log", tmp_path / "x.log"], "--add-log goes with --add"),
                      ([fa] + ml + ["--start-tree", tree], "Unmatched MSA and Tree: sequence '%s' is no leaf of" % c.qnames[0]),
                      ([fa] + ml + ["--start-tree", extra, "--add"], "Unmatched MSA and Tree: leaf 'nobody' of .* is no sequence of the MSA"),
                      ([fa] + ml + ["--start-tree", tree, "--add", "--mem", "0.0001"], r"--add: %d nodes of 600 columns after 4 insertions need %d bytes .* --mem allows 100000 bytes"
                       % (len(c.parent) + 8, E.add_need(len(c.parent) + 8, 600, 4)))):
        r = _run([_bin()] + args + ["-o", tmp_path / "o.tree", "--add-log", tmp_path / "a.log"] if "--add" in args and "--add-log" not in args else
                 [_bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


# ---- 7. the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_add_host.cpp and hu_blen_host.cpp (no HIP headers) with tests/san/add_driver.cpp under AddressSanitizer + UBSan, run as a
    stand-alone program: three leaves plus one query, a four-child node, 1 and 257 columns, a query of gaps only, two queries on one edge,
    the refusals"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "add_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "add_driver.cpp"), os.path.join(CSRC, "hu_add_host.cpp"), os.path.join(CSRC, "hu_blen_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "searches: 4" in r.stdout and "refusals: 6" in r.stdout and "two on one edge: 2 rounds" in r.stdout


# ---- the device ----

def device_case(n_leaves, L, nq):
    def make():
        rng = np.random.default_rng(3000 * n_leaves + L)
        kind = (n_leaves + L) % 3
        parent = (np.array([-1, 0, 0, 0], np.int32) if n_leaves == 3 else build_tree(n_leaves, rng, top=2 + kind % 2) if n_leaves < 9 else random_tree(n_leaves, rng))
        c = with_rm(make_case(parent, L, ("JC69", "HKY85", "GTR")[kind], 300 * n_leaves + L, random_leaf=n_leaves >= 5, max_len=2.0 if n_leaves >= 5 else 10.0))
        base = queries_of(c, 5 * n_leaves + L)
        more = []
        for k in range(nq):
            row = np.array(base[(0, 2, 3)[k % 3]])              # no row of gaps only: its f is the same on every edge, and the best one is rounding
            if k >= 3:
                hit = rng.random(L) < 0.2
                row[hit] = rng.integers(-1, 4, L)[hit]
                row[row < 0] = -2
            more.append(row)
        c.q = np.ascontiguousarray(np.stack(more), np.int8)
        return c
    return cached(("dev", n_leaves, L, nq), make)


DEVICE_SHAPES = [(3, 1, 1), (5, 63, 1), (5, 64, TILE), (33, 65, TILE + 1), (5, 255, TILE + 1), (3, 256, TILE), (33, 257, 1), (5, E.BLEN_LDS_COLS, TILE + 1),
                 (5, E.BLEN_LDS_COLS + 1, TILE + 1), (33, E.BLEN_LDS_COLS + 1, 1), (3, E.BLEN_LDS_COLS, 1)]


def restated_too(c, L, nq):
    """the device shapes that are also held against the restatement: the small ones, and one query on either side of the switch of the ratios"""
    return len(c.parent) * L * nq <= 40000 or nq == 1


def test_the_host_path_meets_the_bar_on_the_devices_shapes():
    """and no query of these shapes has two edges within four bars of each other at the top: a last bit cannot change a best edge"""
    worst = 0.0
    for n_leaves, L, nq in DEVICE_SHAPES:
        c = device_case(n_leaves, L, nq)
        f = np.sort(scores(c, True)["f"], axis=1)
        assert ((f[:, -1] - f[:, -2]) > 4 * F_BAR * np.abs(f[:, -1])).all(), (n_leaves, L, nq)
        if restated_too(c, L, nq):
            worst = max(worst, check_scores(c, scores(c, True))[0])
    print("largest deviation of the host path's f on the device's shapes: %.3g" % worst)
    assert worst <= F_BAR


@pytest.mark.gpu
def test_scores_and_optima_against_the_really_grown_tree_device():
    """measured: DEVICE_WORST"""
    _need_gpu()
    worst = run_restatement(host=False)
    print("largest deviation of the device's f: %.3g" % worst)
    check_impossible(False)
    assert worst <= F_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L,nq", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L, nq):
    """the edges of a thread's stride (256 columns) and of a wave, one column, the column counts on either side of the switch from ratios in
    LDS to ratios in global memory, one query, a full tile and one more: the same best edges, t* within 2 tau of the host path's, f under
    the bar, the same bits twice"""
    _need_gpu()
    c = device_case(n_leaves, L, nq)
    host, dev, again = scores(c, True), scores(c, False), scores(c, False)
    assert same_bits(dev, again)
    assert np.array_equal(dev["best_w"], host["best_w"])
    root = np.asarray(c.parent) < 0
    assert np.array_equal(dev["t_star"][:, root], host["t_star"][:, root]) and np.array_equal(dev["f"][:, root], host["f"][:, root])
    gap = np.abs(dev["t_star"] - host["t_star"]).max()
    worst = np.abs((dev["f"][:, ~root] - host["f"][:, ~root]) / host["f"][:, ~root]).max()
    print("n %d L %d q %d: largest |t* device - t* host| %.3g, largest deviation of f %.3g" % (n_leaves, L, nq, gap, worst))
    assert gap <= 2 * TAU and worst <= F_BAR
    if restated_too(c, L, nq):
        w = check_scores(c, dev)[0]
        print("n %d L %d q %d: largest deviation of the device's f from the restatement %.3g" % (n_leaves, L, nq, w))
        assert w <= F_BAR


@pytest.mark.gpu
def test_a_slab_and_a_tile_of_one_give_the_bits_of_the_default_on_the_device():
    _need_gpu()
    for n_leaves, L, nq in ((33, 65, TILE + 1), (5, E.BLEN_LDS_COLS + 1, TILE + 1)):
        c = device_case(n_leaves, L, nq)
        a = scores(c, False)
        for kw in (dict(slab=1, tile=1), dict(slab=5, tile=3), dict(tile=64), dict(slab=TILE)):
            assert same_bits(a, scores(c, False, **kw)), (n_leaves, L, kw)


@pytest.mark.gpu
def test_search_on_the_device():
    _need_gpu()
    c = search_case()
    host = cached("host search", lambda: host_search(c))
    dev = E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md)
    assert np.array_equal(dev["parent"], host["parent"]) and np.array_equal(dev["child_idx"], host["child_idx"]) and np.array_equal(dev["query_node"], host["query_node"])
    assert [(i["round"], i["query"], i["v"], i["w"]) for i in dev["inserts"]] == [(i["round"], i["query"], i["v"], i["w"]) for i in host["inserts"]]
    gap = np.abs(dev["blen"] - host["blen"]).max()
    print("largest |blen device - blen host| %.3g" % gap)
    assert gap <= 2e-5                                          # 2 eps of the fit
    check_search(c, dev)
    small = E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, slab=1, tile=1)
    assert np.array_equal(small["blen"], dev["blen"]) and small["inserts"] == dev["inserts"]


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    _need_gpu()
    c = add_cases()[5]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.add_need(n, L, len(c.q))):
        E.tree_add_scores(c.parent, c.start, c.seq, c.q, c.md, mem_budget=1 << 20)
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.add_need(n + 2 * len(c.q), L, len(c.q))):
        E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, mem_budget=1 << 20)


@pytest.mark.gpu
def test_tree_add_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree --ml-lengths on 70_otus without five of its rows, then --start-tree that tree --add on the full alignment: a tree
    of 125 leaves; then hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm: a database of 125 leaves"""
    _need_gpu()
    import gzip
    with gzip.open(FASTA70, "rt") as f:
        recs = f.read().split(">")[1:]
    assert len(recs) == 125
    left_out = [recs[i].split()[0] for i in (3, 40, 41, 77, 124)]
    (tmp_path / "old.fasta").write_text("".join(">" + x for x in recs if x.split()[0] not in left_out))
    (tmp_path / "full.fasta").write_text("".join(">" + x for x in recs))
    r = _run([_bin(), "old.fasta", "-sm", sm("GTR"), "--ml-lengths", "--ml-rounds", 5, "-o", "old.tree"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin(), "full.fasta", "-sm", sm("GTR"), "--ml-lengths", "--ml-rounds", 5, "--start-tree", "old.tree", "--add", "--add-log", "add.log", "-o", "full.tree", "-v"],
             cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    rows, ins = read_log(tmp_path / "add.log")
    print(rows, ins)
    assert sorted(x[1] for x in ins) == sorted(left_out)
    t = E.newick_parse((tmp_path / "full.tree").read_text())
    k = kids_of(t["parent"])
    assert sorted(t["names"][u] for u in range(len(k)) if not k[u]) == sorted(x.split()[0] for x in recs)
    r = _run([_bin("hmmufotu-amd-train-sm"), "full.fasta", "full.tree", "-o", "add.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), "full.fasta", "full.tree", "--no-hmm", "-sm", "add.sm", "-n", "adddb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "adddb.ptu"))
    par = np.asarray(db["parent"])
    assert (par < 0).sum() == 1 and len(par) - len(set(par[par >= 0].tolist())) == 125
