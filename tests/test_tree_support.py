"""hmmufotu-amd-tree --support: local branch supports of the eligible edges, a RELL bootstrap over the three
arrangements of an edge, and the aLRT statistic.

The yardstick is the restatement of tests/test_tree_nni.py and tests/test_tree_blen.py, which shares no code with the library: the
per-column value of an arrangement is log L0 + us + ds of a tree that was really rearranged, pruned in linear space and rooted at the
central edge (Arrangement), taken at the library's own t*_q, which is held to the restated optimum as the scores' test holds it: a
column's value moves by its slope times the distance, so a t* that is only within HU_BLEN_TAU of the library's would move S by more than
the bar.  The draws are restated from engine.sim_philox and the rule of the issue; the tests of S take the library's table, which that
test holds.  S is taken by math.fsum.

The bar of S, relative to |f^0(t*_0)|: measured over cases(), the other CPU cases and the device's shapes, the largest deviation is
HOST_WORST on the host path and DEVICE_WORST on the device; four times the larger, rounded up to a power of two, is S_BAR.  It has to be
at most 2^-42, a quarter of HU_SUPPORT_TIE, for the tie threshold to cover the rounding; S_BAR is asserted against that.  A replicate is
close when the restatement's own |S^q_b + eta_e| <= S_BAR |f^0| for either q; the library's count must lie between the restated count
of decided supporters and that plus the edge's close replicates, and by the restatement alone close replicates are at most 1 % of a
case's replicates (a case that breaks it gets another seed).  The largest of the device's shapes, 130 leaves x 1,000 columns x 1,000
replicates with 124 edges, takes 22 s to restate; there, and wherever the device is held against the host path, closeness is taken from
the host path's sums.  Restated once with the sums in 80-bit arithmetic, that shape had no close replicate and its host path's S
deviated by 2.2e-16.
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
from test_tree_blen import RefModel, RefTree, random_tree, sm, to_newick, write_fasta  # noqa: E402,F401
from test_tree_nni import (Arrangement, Case, F_BAR, MIN_GAIN, STAR3, build_tree, cached, cases, check_t_star, eligible, kids_of, make_case,  # noqa: E402
                           poly_case, program_case, search_case, simulate, star_case, device_case, _bin, _run, _need_gpu, FASTA70, REF)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
TIE = E.SUPPORT_TIE
HOST_WORST = 4.65e-15       # measured: the host path, GTR 6 leaves x 70 columns; 2.17e-15 over the device's shapes that are restated
DEVICE_WORST = 4.72e-15     # measured: MI355X, the CPU cases; at most 2e-16 from the host path's S over the device's shapes
S_BAR = 2.0 ** -45          # 4 x 4.72e-15 = 1.89e-14, rounded up to a power of two: 2.84e-14
assert S_BAR <= 2.0 ** -42 and TIE == 2.0 ** -40
B_CASES = 300
DBL_MAX = sys.float_info.max


# ---- the restatement ----

def restated_weights(L, B, seed):
    w = np.zeros((B, L), np.int64)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    for b in range(B):
        for g in range((L + 3) // 4):
            words = E.sim_philox([g, b, 0, 0x53555050], key)
            for k in range(4):
                if 4 * g + k < L:
                    w[b, (int(words[k]) * L) >> 32] += 1
    return w


def column_values(c, blen, e, q, t):
    """l^q_j of the rearranged tree at the central length t"""
    a = Arrangement(c, blen, e, q)
    r, u = a.ref, a.u
    L0 = np.einsum("ja,ab,jb->j", r.up[u] * r.m.pi[None, :], r.m.P(t), r.down[u])
    with np.errstate(divide="ignore"):
        return np.log(np.maximum(L0, 0.0)) + r.us[u] + r.ds[u], a


def restate(c, got, blen, B, seed, check_optima=True):
    """per eligible edge: f [3], S [B][2] by fsum (-inf where a drawn column is impossible), eta; t* is the library's, held to the restated optimum"""
    w = E.support_weights(c.seq.shape[1], B, seed).astype(float)
    out = []
    for i, e in enumerate(eligible(c.parent)[0]):
        l = []
        for q in range(3):
            v, a = column_values(c, blen, e, q, got["t_star"][i][q])
            if check_optima:
                check_t_star(a, got["t_star"][i][q], c.min_len, c.max_len, (c.name, e["u"], q))
            l.append(v)
        assert np.all(np.isfinite(l[0])), c.name
        f = [math.fsum(x) if np.all(np.isfinite(x)) else -math.inf for x in l]
        S = np.zeros((B, 2))
        for q in (1, 2):
            d = l[q] - l[0]
            fin = np.isfinite(d)
            for b in range(B):
                S[b, q - 1] = -math.inf if np.any(w[b][~fin] > 0) else math.fsum(w[b][fin] * d[fin])
        out.append(dict(e=e, f=f, S=S, eta=TIE * abs(f[0])))
    return out


def hold(c, got, ref, B):
    """sums under the bar and count by the rule of close replicates; returns the largest deviation of S and the close replicates"""
    assert got["replicates"] == B and len(ref) == len(got["edge_node"]) and [r["e"]["u"] for r in ref] == list(got["edge_node"]), c.name
    worst, close_all = 0.0, 0
    for i, r in enumerate(ref):
        f0 = abs(r["f"][0]); thr = S_BAR * f0
        S, T = r["S"], got["sums"][i]
        assert not np.isnan(T).any() and not np.isnan(got["f"][i]).any()
        inf = np.isinf(S)
        assert np.all(T[inf] <= -DBL_MAX), c.name
        if (~inf).any():
            worst = max(worst, float(np.abs(T[~inf] - S[~inf]).max()) / f0)
        decided = int(np.sum((S[:, 0] < -r["eta"] - thr) & (S[:, 1] < -r["eta"] - thr)))
        close = int(np.sum((np.abs(S[:, 0] + r["eta"]) <= thr) | (np.abs(S[:, 1] + r["eta"]) <= thr)))
        assert decided <= got["count"][i] <= decided + close, (c.name, r["e"]["u"], decided, close, got["count"][i])
        assert got["support"][i] == got["count"][i] / B
        fin = [q for q in range(3) if math.isfinite(r["f"][q])]
        assert all(abs(got["f"][i][q] - r["f"][q]) <= F_BAR * abs(r["f"][q]) for q in fin)
        if len(fin) == 3:
            alrt = 2 * (r["f"][0] - max(r["f"][1], r["f"][2]))
            assert abs(got["alrt"][i] - alrt) <= 4 * F_BAR * max(abs(x) for x in r["f"]), c.name
        close_all = max(close_all, close)
    assert close_all <= 0.01 * B, (c.name, close_all)
    return worst, close_all


def support(c, host, blen=None, B=B_CASES, seed=1, **kw):
    return E.tree_nni_support(c.parent, c.start if blen is None else blen, c.seq, c.md, replicates=B, seed=seed, min_len=c.min_len, max_len=c.max_len,
                              host=host, with_sums=True, **kw)


def strip_inner(seq, parent):
    kids = kids_of(parent)
    for u in range(len(parent)):
        if kids[u]:
            seq[u] = -2
    return np.ascontiguousarray(seq, np.int8)


def simulated_case(name, parent, blen, L, model, seed):
    c = Case()
    c.name = name; c.parent = np.asarray(parent, np.int32)
    c.sm = synth.load_model(model); c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par); c.rm = RefModel(c.sm)
    c.min_len, c.max_len = 0.0, 10.0
    c.start = np.asarray(blen, float)
    c.seq = strip_inner(simulate(c.parent, c.start, L, c.rm, np.random.default_rng(seed)), c.parent)
    return c


def collapsed_case(L=200):
    """six leaves under a trifurcating top node, HKY85; the rows come down the tree with the first eligible edge at length 0"""
    def make():
        rng = np.random.default_rng(2)
        parent = build_tree(6, rng, top=3)
        bl = np.where(parent >= 0, rng.uniform(0.05, 0.2, len(parent)), 0.0)
        u = eligible(parent)[0][0]["u"]
        bl[u] = 0.0
        # a seed of the simulation at which all three optima are 0; at others one arrangement takes a length of about 1e-3 by chance
        c = simulated_case("collapsed %d" % L, parent, bl, L, "HKY85", {200: 2, E.SUPPORT_LDS_COLS + 1: 8}[L])
        c.collapsed = u
        return c
    return cached(("collapsed", L), make)


def impossible_case():
    """a bifurcating root over two cherries; every branch at 0; the cherries hold one base each, equal in the first 20 columns and
    different in the other 30: there A and C (or B and C) under one node at distance 0 share no base"""
    def make():
        c = Case()
        c.name = "impossible"; c.parent = np.array([-1, 0, 1, 1, 0, 4, 4], np.int32)
        c.sm = synth.load_model("JC69"); c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par); c.rm = RefModel(c.sm)
        c.min_len, c.max_len = 0.0, 10.0
        c.start = np.zeros(7)
        seq = np.full((7, 50), -2, np.int8)
        left = np.arange(50) % 4
        right = np.where(np.arange(50) < 20, left, (left + 1 + np.arange(50) % 3) % 4)
        seq[2] = seq[3] = left; seq[5] = seq[6] = right
        c.seq = np.ascontiguousarray(seq)
        return c
    return cached("impossible", make)


def known_case():
    """a known 12-leaf tree, HKY85, 600 columns: one inner branch of 0.3 and one of 0.002, the others 0.05 to 0.2"""
    def make():
        rng = np.random.default_rng(77)
        parent = build_tree(12, rng, top=3)
        bl = np.where(parent >= 0, rng.uniform(0.05, 0.2, len(parent)), 0.0)
        inner = [e["u"] for e in eligible(parent)[0] if e["kind"] == "inner"]
        bl[inner[0]] = 0.3; bl[inner[-1]] = 0.002
        c = simulated_case("known", parent, bl, 600, "HKY85", 78)
        c.long, c.short = inner[0], inner[-1]
        return c
    return cached("known", make)


def all_cpu_cases():
    return cases() + [collapsed_case(), impossible_case(), known_case()]


def restated(c, host=True):
    """the library's answer and the restatement of a case, computed once"""
    def make():
        got = support(c, host=True)
        return got, restate(c, got, c.start, B_CASES, 1, check_optima=c.name != "impossible")   # there f^1 and f^2 are -inf and have no slope
    return cached(("restated", c.name), make)


# ---- 1. the weights ----

@pytest.mark.parametrize("L,B", [(1, 1), (2, 3), (65, 16), (257, 5)])
def test_weights_are_the_restated_draws(L, B):
    w = E.support_weights(L, B, 5)
    assert w.dtype == np.uint16 and np.array_equal(w, restated_weights(L, B, 5))
    assert np.all(w.sum(1) == L)
    big = E.support_weights(L, B + 7, 5)
    assert np.array_equal(big[:B], w)                           # the prefix property
    hi = E.support_weights(L, B, 5 + (3 << 32))
    assert np.array_equal(hi, restated_weights(L, B, 5 + (3 << 32)))
    if L >= 65:                                                 # two columns can draw alike by chance
        assert not np.array_equal(E.support_weights(L, B, 6), w) and not np.array_equal(hi, w)


# ---- 2. the host path against the restatement ----

def test_scores_are_the_scorers_to_the_bit_host():
    for c in all_cpu_cases():
        got = restated(c)[0]
        sc = E.tree_nni_scores(c.parent, c.start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, host=True)
        assert np.array_equal(got["edge_node"], sc["edge_node"]) and got["skipped"] == sc["skipped"]
        assert got["t_star"].tobytes() == sc["t_star"].tobytes() and got["f"].tobytes() == sc["f"].tobytes(), c.name


def test_sums_counts_and_alrt_against_the_restatement_host():
    """measured: HOST_WORST"""
    worst, kinds = 0.0, set()
    for c in all_cpu_cases():
        got, ref = restated(c)
        w, close = hold(c, got, ref, B_CASES)
        print("%s: largest deviation of S %.3g, close replicates %d" % (c.name, w, close))
        worst = max(worst, w); kinds |= {r["e"]["kind"] for r in ref}
    print("largest deviation of the host path's S: %.3g" % worst)
    assert kinds == {"inner", "root3", "root2"} and worst <= S_BAR
    assert any(c.seq[c.leaves[0]].max() < 0 for c in cases())  # a leaf row of gaps only
    # a polytomy: its edge is skipped and counted; three leaves: nothing to score, a success
    got = support(poly_case(), host=True)
    assert len(got["edge_node"]) == 0 and got["skipped"] == 1 and got["sums"].shape == (0, B_CASES, 2) and got["count"].shape == (0,)
    got = support(star_case(), host=True)
    assert len(got["edge_node"]) == 0 and got["skipped"] == 0 and got["f"].shape == (0, 3)
    assert eligible(cases()[6].parent)[1] > 0


def test_a_collapsed_edge_has_no_support_host():
    """the case eta exists for: the three arrangements are one star, d is rounding noise, and S < 0 alone would toss a coin"""
    c = collapsed_case()
    got, ref = restated(c)
    i = list(got["edge_node"]).index(c.collapsed)
    assert np.all(got["t_star"][i] == 0.0) and got["count"][i] == 0
    assert np.abs(ref[i]["S"]).max() < ref[i]["eta"] / 4       # noise far inside the tie threshold: no replicate is close
    assert np.abs(got["sums"][i]).max() < ref[i]["eta"]
    assert got["count"].max() > 0.5 * B_CASES                   # the other edges of the tree are supported


def test_an_impossible_arrangement_counts_as_supporting_and_gives_no_nan():
    c = impossible_case()
    got, ref = restated(c)
    assert len(got["edge_node"]) == 1 and np.all(np.isinf(ref[0]["S"])) and ref[0]["f"][1] == ref[0]["f"][2] == -math.inf
    assert np.all(got["sums"] == -math.inf) and got["count"][0] == B_CASES and got["support"][0] == 1.0
    assert not np.isnan(got["sums"]).any() and not np.isnan(got["f"]).any() and not np.isnan(got["t_star"]).any() and got["alrt"][0] == math.inf
    # the tree itself at likelihood 0 (different bases under a cherry at distance 0) is refused with that reason
    seq = c.seq.copy(); seq[3] = (seq[2] + 1) % 4
    with pytest.raises(E.EngineError, match="log-likelihood is -inf"):
        E.tree_nni_support(c.parent, c.start, seq, c.md, replicates=5, host=True)


def test_a_long_branch_is_supported_and_a_short_one_less():
    c = known_case()
    got, ref = restated(c)
    il, is_ = list(got["edge_node"]).index(c.long), list(got["edge_node"]).index(c.short)
    own = [int(np.sum((r["S"][:, 0] < -r["eta"]) & (r["S"][:, 1] < -r["eta"]))) for r in ref]
    assert own[il] == B_CASES and own[is_] < own[il]
    assert got["count"][il] == B_CASES and got["count"][is_] < got["count"][il]


def test_alrt_at_a_local_optimum_is_above_minus_twice_min_gain():
    c = search_case()
    r = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=True)
    assert r["stop"] == "local optimum"
    got = E.tree_nni_support(r["parent"], r["blen"], c.seq, c.md, replicates=50, host=True)
    assert len(got["alrt"]) > 0 and np.all(got["alrt"] >= -2 * MIN_GAIN)


def test_count_does_not_depend_on_the_budget_and_the_first_replicates_are_a_shorter_runs():
    c = cases()[4]
    got = restated(c)[0]
    n, L = c.seq.shape
    again = support(c, host=True, mem_budget=E.support_need(n, L, B_CASES))
    assert np.array_equal(again["count"], got["count"]) and again["sums"].tobytes() == got["sums"].tobytes()
    short = support(c, host=True, B=37)
    assert short["sums"].tobytes() == got["sums"][:, :37].tobytes()
    assert not np.array_equal(support(c, host=True, seed=2)["sums"], got["sums"])


def test_entries_refuse_what_the_header_says():
    c = cases()[3]
    n, L = c.seq.shape
    kw = dict(host=True)
    for B in (0, -1, 100001):
        with pytest.raises(E.EngineError, match="replicates: 1 to 100000"):
            E.tree_nni_support(c.parent, c.start, c.seq, c.md, replicates=B, **kw)
    for L2, B in ((0, 1), (65536, 1), (5, 0), (5, 100001)):
        with pytest.raises(E.EngineError):
            E.support_weights(L2, B, 1)
    need = E.support_need(n, L, 1000)
    assert need > E.nni_need(n, L) + 2 * 1000 * L and E.support_need(n, L, 1001) >= need + 2 * 4 * L
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is %d bytes" % (need, need - 1)):
        E.tree_nni_support(c.parent, c.start, c.seq, c.md, replicates=1000, mem_budget=need - 1, **kw)
    with pytest.raises(E.EngineError, match="budget below 0"):
        E.tree_nni_support(c.parent, c.start, c.seq, c.md, replicates=10, mem_budget=-1, **kw)
    gamma = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.5, 1.0, 2.4])
    with pytest.raises(E.EngineError, match="4 discrete Gamma categories"):
        E.tree_nni_support(c.parent, c.start, c.seq, gamma, replicates=10, **kw)
    bad = c.parent.copy(); bad[1] = 1
    with pytest.raises(E.EngineError):
        E.tree_nni_support(bad, c.start, c.seq, c.md, replicates=10, **kw)
    with pytest.raises(E.EngineError, match="min_len|max_len|length"):
        E.tree_nni_support(c.parent, c.start, c.seq, c.md, replicates=10, min_len=2.0, max_len=1.0, **kw)


# ---- 3. the program ----

LABEL = re.compile(r"\)(\d\.\d{3}):")


def seq_of(back, c):
    """the rows of a parsed tree's nodes, by leaf name"""
    row = {c.names[u]: c.seq[u] for u in range(len(c.names)) if c.names[u]}
    return np.ascontiguousarray([row.get(x, np.full(c.seq.shape[1], -2, np.int8)) for x in back["names"]], np.int8)


def test_program_labels_the_tree_and_writes_the_table(tmp_path):
    c, fa, tree = program_case(tmp_path)
    base = [_bin(), fa, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", tree]
    plain, out, tsv = tmp_path / "plain.tree", tmp_path / "out.tree", tmp_path / "s.tsv"
    assert _run(base + ["-o", plain]).returncode == 0
    r = _run(base + ["-o", out, "--support", 100, "--support-seed", 7, "--support-out", tsv, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"Local supports: \d+ edge\(s\) scored over 100 replicate\(s\), 0 edge\(s\) at polytomies skipped", r.stderr), r.stderr
    assert re.search(r"sweep \S+ s, scoring \S+ s, weights \S+ s, supports \S+ s", r.stderr)
    text = out.read_text()
    assert LABEL.sub("):", text).encode() == plain.read_bytes()
    back, want = E.newick_parse(text), E.newick_parse(plain.read_text())
    assert np.array_equal(back["parent"], want["parent"]) and np.array_equal(back["blen"], want["blen"])
    assert back["names"][0] == "top" and [a for a, b in zip(back["names"], want["names"]) if b] == [b for b in want["names"] if b]
    lib = E.tree_nni_support(want["parent"], want["blen"], seq_of(want, c), c.md, replicates=100, seed=7, host=True)
    lines = tsv.read_text().splitlines()
    assert lines[0] == "node\tname\tkind\tleaves\tt0\talrt\tcount\treplicates\tsupport"
    assert lines[-2] == "# skipped: 0 edges at polytomies" and lines[-1] == "# seed: 7"
    rows = [x.split("\t") for x in lines[1:-2]]
    assert all(len(x) == 9 for x in rows) and [int(x[0]) for x in rows] == list(lib["edge_node"])
    assert [int(x[6]) for x in rows] == list(lib["count"]) and all(x[7] == "100" for x in rows)
    kids = kids_of(want["parent"])

    def leaves(u):
        return 1 if not kids[u] else sum(leaves(v) for v in kids[u])
    for x, e, cnt, alrt in zip(rows, eligible(want["parent"])[0], lib["count"], lib["alrt"]):
        u = int(x[0])
        assert x[2] == e["kind"] and int(x[3]) == leaves(u) and float(x[8]) == cnt / 100 and float(x[5]) == alrt
        assert float(x[4]) == want["blen"][u] + (want["blen"][e["s"]] if e["kind"] == "root2" else 0.0)
        assert all(repr(float(v)) == repr(float("%.17g" % float(v))) for v in x[4:6])
        assert back["names"][u] == "%.3f" % (cnt / 100)
        if e["kind"] == "root2":
            assert back["names"][e["s"]] == back["names"][u]
    labelled = {int(x[0]) for x in rows} | {e["s"] for e in eligible(want["parent"])[0] if e["kind"] == "root2"}
    assert all((back["names"][u] != want["names"][u]) == (u in labelled) for u in range(len(kids)))
    # with --nni: the labels come off to the bytes of the run without --support
    assert _run(base + ["--nni", "-o", tmp_path / "nni.tree"]).returncode == 0
    assert _run(base + ["--nni", "--support", 20, "-o", tmp_path / "nnis.tree"]).returncode == 0
    assert LABEL.sub("):", (tmp_path / "nnis.tree").read_text()).encode() == (tmp_path / "nni.tree").read_bytes()
    assert len(LABEL.findall((tmp_path / "nnis.tree").read_text())) >= len(rows)


def test_program_keeps_the_name_of_a_named_inner_node_and_labels_both_ends_of_a_root_edge(tmp_path):
    c = cases()[3]                                              # six leaves under a bifurcating root with two inner children
    kids = kids_of(c.parent)
    e = [x for x in eligible(c.parent)[0] if x["kind"] == "root2"][0]
    other = [x for x in eligible(c.parent)[0] if x["kind"] == "inner"][0]
    names = ["" if kids[u] else "s%d" % u for u in range(len(kids))]
    names[other["u"]] = "clade"
    leaves = [u for u in range(len(kids)) if not kids[u]]
    fa, tree, out = tmp_path / "in.fasta", tmp_path / "start.tree", tmp_path / "out.tree"
    rows = c.seq[leaves].copy(); rows[rows < 0] = -1
    write_fasta(fa, [names[u] for u in leaves], rows)
    tree.write_text(to_newick(c.parent, kids, names, c.start) + ";\n")
    r = _run([_bin(), fa, "--host", "-sm", sm("JC69"), "--ml-lengths", "--start-tree", tree, "--support", 30, "-o", out])
    assert r.returncode == 0, r.stderr
    back = E.newick_parse(out.read_text())
    byname = {x: u for u, x in enumerate(back["names"])}
    assert "clade" in byname and back["names"].count("clade") == 1
    kb = kids_of(back["parent"])
    top = kb[int(np.nonzero(np.asarray(back["parent"]) < 0)[0][0])]
    assert len(top) == 2 and back["names"][top[0]] == back["names"][top[1]] and re.fullmatch(r"\d\.\d{3}", back["names"][top[0]])
    assert e["s"] is not None


def test_program_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, fa, tree = program_case(tmp_path)
    ml = ["-sm", sm("HKY85"), "--ml-lengths"]
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa, "-sm", sm("HKY85"), "--support", "10"], "--support goes with --ml-lengths"),
                      ([fa] + ml + ["--support-seed", "3"], "go with --support"),
                      ([fa] + ml + ["--support-out", tmp_path / "x.tsv"], "go with --support"),
                      ([fa] + ml + ["--support", "0"], "--support must be 1 to 100000"),
                      ([fa] + ml + ["--support", "100001", "--support-out", tmp_path / "x.tsv"], "--support must be 1 to 100000"),
                      ([fa] + ml + ["--support", "100", "--mem", "0.0001"], r"--support: .*need \d+ bytes .* --mem allows 100000 bytes"),
                      ([fa] + ml + ["--nni", "--support", "100", "--mem", "0.0001", "--start-tree", tree], r"--support: .*need \d+ bytes .* --mem allows 100000 bytes")):
        r = _run([_bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


# ---- 4. the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_support_host.cpp, hu_nni_host.cpp and hu_blen_host.cpp (no HIP headers) with tests/san/support_driver.cpp under AddressSanitizer +
    UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "support_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "support_driver.cpp"), os.path.join(CSRC, "hu_support_host.cpp"),
                        os.path.join(CSRC, "hu_nni_host.cpp"), os.path.join(CSRC, "hu_blen_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "weights: 2" in r.stdout and "trees: 4" in r.stdout and "refusals: 5" in r.stdout


# ---- the device ----

DEVICE_SHAPES = [(4, 1, 1), (5, 63, 255), (5, 64, 256), (33, 65, 257), (6, 256, 1000), (33, 257, 64), (5, E.SUPPORT_LDS_COLS, 300),
                 (5, E.SUPPORT_LDS_COLS + 1, 300), (5, E.NNI_LDS_COLS + 1, 33), (130, 1000, 1000)]
RESTATED_SHAPES = [s for s in DEVICE_SHAPES if s[0] * s[1] * s[2] <= 10000000]      # all but the largest, whose fsums would take half a minute


def test_close_replicates_are_rare_on_the_devices_shapes_and_the_host_path_meets_the_bar_there():
    """by the restatement where the shape is small enough for a test's time, by the host path's sums elsewhere"""
    worst = 0.0
    for n_leaves, L, B in DEVICE_SHAPES:
        c = device_case(n_leaves, L)
        got = cached(("devhost", n_leaves, L, B), lambda: support(c, host=True, B=B))
        assert len(got["edge_node"]) > 0
        if (n_leaves, L, B) in RESTATED_SHAPES:
            w, close = hold(c, got, restate(c, got, c.start, B, 1, check_optima=False), B)
            print("n %d L %d B %d: largest deviation of S %.3g, close replicates %d" % (n_leaves, L, B, w, close))
            worst = max(worst, w)
        else:
            assert host_close(got).max() <= 0.01 * B
    print("largest deviation of the host path's S on the device's shapes: %.3g" % worst)
    assert worst <= S_BAR


def host_close(got):
    """per edge, the replicates within the bar of the tie threshold by the sums of the host path"""
    f0 = np.abs(got["f"][:, 0])[:, None, None]
    return np.sum(np.any(np.abs(got["sums"] + TIE * f0) <= S_BAR * f0, axis=2), axis=1)


def against_host(c, B, host, dev, again):
    for k in ("edge_node", "t_star", "f", "count", "sums"):
        assert dev[k].tobytes() == again[k].tobytes(), k
    assert np.array_equal(dev["edge_node"], host["edge_node"]) and dev["skipped"] == host["skipped"]
    f0 = np.abs(host["f"][:, 0])[:, None, None]
    with np.errstate(invalid="ignore"):
        dev_s = np.where(np.isinf(host["sums"]), np.where(dev["sums"] <= -DBL_MAX, 0.0, np.inf), np.abs(dev["sums"] - host["sums"]) / f0)
    worst = float(dev_s.max())
    close = host_close(host)
    assert np.all(np.abs(dev["count"] - host["count"]) <= close), (c.name, dev["count"], host["count"], close)
    return worst


@pytest.mark.gpu
def test_sums_counts_and_alrt_against_the_restatement_device():
    """measured: DEVICE_WORST"""
    _need_gpu()
    worst = 0.0
    for c in all_cpu_cases():
        ref = restated(c)[1]
        dev = support(c, host=False)
        w, close = hold(c, dev, ref, B_CASES)
        print("%s: largest deviation of the device's S %.3g" % (c.name, w))
        worst = max(worst, w)
    print("largest deviation of the device's S: %.3g" % worst)
    assert worst <= S_BAR
    for c in (poly_case(), star_case()):
        assert len(support(c, host=False)["edge_node"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L,B", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L, B):
    """the edges of a thread's stride of columns and of a workgroup's stride of replicates (256 x 4), one column and one replicate, the
    column counts on either side of the switch from pairs in LDS to pairs in global memory and of the scorer's switch: sums under the bar,
    counts equal but for close replicates, the same bits twice"""
    _need_gpu()
    c = device_case(n_leaves, L)
    host = cached(("devhost", n_leaves, L, B), lambda: support(c, host=True, B=B))
    dev, again = support(c, host=False, B=B), support(c, host=False, B=B)
    worst = against_host(c, B, host, dev, again)
    print("n %d L %d B %d: largest deviation of the device's S from the host path's %.3g" % (n_leaves, L, B, worst))
    assert worst <= S_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("L", [200, E.SUPPORT_LDS_COLS + 1])
def test_a_collapsed_edge_has_no_support_device(L):
    _need_gpu()
    c = collapsed_case(L)
    host, dev = support(c, host=True), support(c, host=False)
    i = list(dev["edge_node"]).index(c.collapsed)
    assert np.all(host["t_star"][i] == 0.0) and host["count"][i] == 0
    assert np.all(dev["t_star"][i] == 0.0) and dev["count"][i] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("L,B", [(1, 1), (65, 16), (257, 1000), (1000, 259)])
def test_the_devices_table_of_weights_is_the_hosts(L, B):
    _need_gpu()
    assert np.array_equal(E.support_weights(L, B, 9, device=0), E.support_weights(L, B, 9))


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    _need_gpu()
    c = cases()[4]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.support_need(n, L, 1000)):
        E.tree_nni_support(c.parent, c.start, c.seq, c.md, replicates=1000, mem_budget=1 << 20)


@pytest.mark.gpu
def test_tree_support_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree --ml-lengths --nni --support -> hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm on 70_otus: the labelled
    tree is a valid input of the rest of the chain, a database of 125 leaves... of the 70 sequences' tree that loads"""
    _need_gpu()
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "--ml-lengths", "--nni", "--nni-rounds", 2, "--ml-rounds", 5, "--support", 100, "-o", "sup.tree",
              "--support-out", "sup.tsv", "-v"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Local supports" in r.stderr and len(LABEL.findall((tmp_path / "sup.tree").read_text())) > 30
    r = _run([_bin("hmmufotu-amd-train-sm"), FASTA70, "sup.tree", "-o", "sup.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), FASTA70, "sup.tree", "--no-hmm", "-sm", "sup.sm", "-n", "supdb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "supdb.ptu"))
    parent = np.asarray(db["parent"])
    assert (parent < 0).sum() == 1
    leaves = len(parent) - len(set(parent[parent >= 0].tolist()))
    print("nodes %d, leaves %d" % (len(parent), leaves))
    assert leaves == 125
