"""The CPU oracle against an independent 50-digit derivation of the same formulas (tests/golden/hiprec.npz, written from the reference's
source by tests/golden/make_hiprec_golden.py, which imports neither oracle/ nor the engine).

Bounds (none of them comes from what the oracle gives):
  Model.P                 absolute 1e-13
  tree messages           1e-11 relative to max(|x|, 1); -inf components are -inf on both sides
  estimateSeq             ratio: the reference's three double operations on the stored integer counts, bit for bit, and within 4 ulp of the
                          exact quotient; unweighted wnr = count / n bit for bit; weighted wnr absolute 1e-12 (a quotient of two sums of at
                          most 190 products of weights in [0, 1]: some hundred roundings of 1.1e-16); loglik relative 1e-12
  placeSeq                outer and EM iteration counts equal; ratio, wnr, height absolute 1e-9; the constant loglik and the intended
                          root loglik relative 1e-12
  filterPlacements        the same set
  q-values                |dq| <= (10 / ln 10) 1e-9 / (1 - p) + 1e-12 q with the exact posterior p; where p > 1 - 1e-6, both sides >= 59.9
A knife-edge candidate (a convergence quantity within 1e-6 relative of 1e-5, an EM quantity that double precision cannot tell from 1e-5
— hiprec_cases.Case.knife —, or two inferred-state components within 1e-9) is compared neither in its counts nor in its unweighted wnr,
and in its lengths to 1e-6 only.  The generator allows 5 % of a database's candidates to be; the archive holds 10 of 1,260, all of the
third kind and all on JC69's two-column read (10 of that database's 210: 4.8 %).
Measured: P(t) 1.0e-15, the oracle's messages 9.1e-13 (synth's 4.2e-12), logliks 5.0e-15, placed lengths 5.3e-14, all counts equal.
The wide set (tests/golden/hiprec_wide.npz: GTR+4 and JC69, 8 leaves x 3,300 columns, twelve reads of 512 to 3,073 columns, no knife-edge
candidate) runs under the same rules and the same bounds (test_wide_*); its figures are printed as HIPREC oracle_wide_* lines and anchor
the kernels' bounds on that set (tests/test_hiprec_gpu.py: ORACLE_WIDE).  Measured: logliks 6.2e-14 (estimate) and 5.7e-14 (root), weighted
wnr 6.5e-15 absolute, placed ratio 1.2e-13 and wnr 1.9e-13 absolute (7.6e-12 relative to max(|x|, 1e-3)), height 6.6e-15, q eps 2.1e-10.
The deep set (tests/golden/hiprec_deep.npz: GTR+4 and JC69, 1,024 leaves x 96 columns, root messages down to -766 / -963 on match columns
and -1,197 / -1,420 on all-gap columns, six reads with a candidate list each, given to the oracle through Tree.assign(seeds=...); 7
knife-edge candidates of 344, all on JC69) runs under the same rules and bounds (test_deep_*): the -510 rescaling of the oracle and of
synth's numpy messages is exercised there and nowhere else.  Its figures are printed as HIPREC oracle_deep_* lines and anchor ORACLE_DEEP
in tests/test_hiprec_gpu.py.  Messages are measured there by hiprec_cases.level_shape as well.  Measured: message level 2.2e-14 (synth
1.3e-13) and shape 4.7e-12 (synth 9.3e-12), root loglik 2.8e-14, estimated and root logliks 4.9e-15, weighted wnr 2.0e-14 relative, placed
lengths 1.3e-11 and height 7.8e-13 relative to max(|x|, 1e-3), q eps 8.0e-12; counts, filter sets and taxon nodes equal.  The oracle is
right at depth too.
The deepwide set (tests/golden/hiprec_deepwide.npz: GTR+4 and JC69 at the deep set's branch lengths on 1,029 leaves x 3,300 columns, 1,200 of
them match columns; seven of the wide set's read shapes, 1,024 to 3,073 columns, with twelve given candidates each; no knife-edge candidate
among the 168) runs under the same rules and bounds (test_deepwide_*).  Its figures are printed as HIPREC oracle_deepwide_* lines and anchor
ORACLE_DEEPWIDE in tests/test_hiprec_gpu.py; they were measured before any kernel ran on this set.  Measured: message level 9.6e-15 (synth
1.4e-14) and shape 1.6e-12 (synth 8.4e-12), root loglik 6.8e-15 (synth 9.6e-15), estimated logliks 2.1e-14, weighted wnr 9.0e-15 absolute
(4.6e-14 relative), intended root loglik 1.9e-14, placed ratio 1.6e-13 and wnr 6.5e-13 absolute (5.8e-12 relative to max(|x|, 1e-3)),
height 5.7e-13 relative, q eps 2.4e-11; counts, filter sets and taxon nodes equal.
"""
import glob
import importlib.util
import os
import re

import numpy as np
import pytest

from hiprec_cases import CASES, DEEP_CASES, DEEP_LL, DEEPWIDE_CASES, DEEPWIDE_READS, WIDE_CASES, WIDE_READS, Case, level_shape, q_ok, ratio_half

REL = 1e-6
HERE = os.path.dirname(os.path.abspath(__file__))


def _oracle(c):
    from oracle import oracle_py as O
    db = c.db
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    T = O.Tree(db.parent, db.blen, db.seq, db.up, db.down, db.height, m, db.dg_r if db.dg_k > 0 else None, db.anno_id)
    return O, m, T


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-300)


def worse(worst, key, x):
    """worst[key] = max(worst[key], x) for a distance that is a number (Python's max(0.0, nan) is 0.0)"""
    x = float(x)
    assert np.isfinite(x), (key, x)
    worst[key] = max(worst[key], x)


@pytest.mark.parametrize("name", CASES)
def test_model_P(name):
    c = Case(name)
    _, m, _ = _oracle(c)
    worst = 0.0
    for i, row in enumerate(c.times()):
        for k, t in enumerate(row):
            d = np.abs(m.P(float(t)) - c.P[i, k]).max()
            assert np.isfinite(d)
            worst = max(worst, d)
    print("hiprec oracle P", name, worst)
    assert worst < 1e-13


def report(test, name, **worst):
    """the figures of the wide set, printed as tests/test_hiprec_gpu.py prints its own (DESIGN.md section 5 quotes them)"""
    print("HIPREC oracle_%s %s %s" % (test, name, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", CASES)
def test_messages(name):
    """the oracle's two-pass pruning and the database's own messages (the ones every other test feeds to oracle and engine)"""
    _messages(Case(name))


def _messages(c):
    name = c.name
    O, m, _ = _oracle(c)
    db = c.db
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up, down, seq, h = O.tree_evaluate(db.parent, db.blen, leaf_only, m, db.dg_r if db.dg_k else None)
    assert np.array_equal(seq, db.seq)
    assert np.abs(h - c.height).max() < 1e-14
    for who, (u_, d_) in dict(oracle=(up, down), synth=(db.up, db.down)).items():
        for got, want in ((u_[:, c.msg_cols], c.up), (d_[1:, c.msg_cols], c.down[1:])):
            inf = np.isneginf(want)
            assert np.array_equal(np.isneginf(got), inf), who
            err = np.abs(got[~inf] - want[~inf]) / np.maximum(np.abs(want[~inf]), 1.0)
            print("hiprec oracle messages", name, who, err.max())
            assert np.isfinite(err).all() and err.max() < 1e-11, who
        root = u_[0]                                             # treeLoglik of a column: log(pi . exp(root message))
        mx = root.max(1)
        ll = mx + np.log((np.asarray(m.pi)[None, :] * np.exp(root - mx[:, None])).sum(1))
        stored = ll if len(c.root_ll) == len(ll) else ll[c.msg_cols]                            # the wide archive: at msg_cols only
        assert (np.abs(stored - c.root_ll) <= 1e-12 * np.abs(c.root_ll)).all(), who
        assert _rel(ll.sum(), c.root_ll_sum) < 1e-12, who


@pytest.mark.parametrize("name", CASES)
def test_estimate(name):
    _estimate(Case(name))


def _estimate(c):
    name = c.name
    _, _, T = _oracle(c)
    worst = dict(ll=0.0, ll_w=0.0, wnr_w=0.0, wnr_w_rel=0.0)
    for ri in range(c.n_reads):
        st, en = int(c.start[ri]), int(c.end[ri])
        for k, u in enumerate(c.cands(ri)):
            e0 = T.estimate(c.codes[ri], st, en, u, c.dist(ri, k), weighted=False)
            e1 = T.estimate(c.codes[ri], st, en, u, c.dist(ri, k), weighted=True)
            assert e0["ratio"] == c.ratio_double(ri, k) == e1["ratio"]
            assert abs(e0["ratio"] - c.est_ratio[ri, k]) <= 4 * np.spacing(c.est_ratio[ri, k])
            if not c.knife[ri, k]:
                assert e0["wnr"] == c.wnr_unweighted(ri, k), (ri, u)
            assert np.isfinite([e0["loglik"], e1["loglik"], c.est_ll[ri, k], c.est_ll_w[ri, k]]).all(), (ri, u)
            worse(worst, "wnr_w", abs(e1["wnr"] - c.est_wnr_w[ri, k]))
            worse(worst, "wnr_w_rel", abs(e1["wnr"] - c.est_wnr_w[ri, k]) / max(abs(c.est_wnr_w[ri, k]), 1e-3))
            worse(worst, "ll", _rel(e0["loglik"], c.est_ll[ri, k]))
            worse(worst, "ll_w", _rel(e1["loglik"], c.est_ll_w[ri, k]))
    print("hiprec oracle estimate", name, worst)
    assert worst["ll"] < 1e-12 and worst["ll_w"] < 1e-12 and worst["wnr_w"] < 1e-12, worst
    return worst


@pytest.mark.parametrize("name", CASES)
def test_place(name):
    _place(Case(name))


def _place(c):
    name = c.name
    _, _, T = _oracle(c)
    worst = dict(ratio=0.0, wnr=0.0, height=0.0, const=0.0, root=0.0, length_rel=0.0, height_rel=0.0)
    for ri in range(c.n_reads):
        st, en = int(c.start[ri]), int(c.end[ri])
        for k, u in enumerate(c.cands(ri)):
            p = T.place(c.codes[ri], st, en, u, c.ratio_double(ri, k), c.wnr_unweighted(ri, k))
            pf = T.place(c.codes[ri], st, en, u, c.ratio_double(ri, k), c.wnr_unweighted(ri, k), fix_root=True)
            assert (pf["ratio"], pf["wnr"], pf["iters"], pf["em_iters"]) == (p["ratio"], p["wnr"], p["iters"], p["em_iters"])
            errs = (abs(p["ratio"] - c.pl_ratio[ri, k]), abs(p["wnr"] - c.pl_wnr[ri, k]), abs(p["height"] - c.placed_height(ri, k)))
            assert np.isfinite(errs).all() and np.isfinite([p["loglik"], pf["loglik"]]).all(), (ri, u, p, pf)
            if c.knife[ri, k]:                                   # counts not compared, lengths to REL; everything else as for any candidate
                assert max(errs) <= REL, (ri, u, errs)
            else:
                assert (p["iters"], p["em_iters"]) == (int(c.pl_outer[ri, k]), int(c.pl_em[ri, k])), (ri, u)
                for key, e in zip(("ratio", "wnr", "height"), errs):
                    worse(worst, key, e)
                # the scale tests/test_hiprec_gpu.py measures the kernels on
                worse(worst, "length_rel", max(errs[0] / max(abs(c.pl_ratio[ri, k]), 1e-3), errs[1] / max(abs(c.pl_wnr[ri, k]), 1e-3)))
                worse(worst, "height_rel", errs[2] / max(abs(c.placed_height(ri, k)), 1e-3))
            if abs(c.pl_ratio[ri, k] - 0.5) > 1e-6:
                assert p["aNode"] == int(c.pl_a_node[ri, k])
            worse(worst, "const", _rel(p["loglik"], c.pl_const_ll[ri]))
            worse(worst, "root", _rel(pf["loglik"], c.pl_root_ll[ri, k]))
    print("hiprec oracle place", name, worst)
    assert worst["ratio"] < 1e-9 and worst["wnr"] < 1e-9 and worst["height"] < 1e-9, worst
    assert worst["const"] < 1e-12, worst
    assert worst["root"] < 1e-12, worst                          # the intended root loglik (--fix-root-loglik): the project's figure for logliks
    return worst


@pytest.mark.parametrize("name", CASES)
def test_assign_filter_set_and_q_values(name):
    _assign(Case(name))


def _assign(c):
    from oracle import oracle_py as O
    _, _, T = _oracle(c)
    worst = dict(q_eps=0.0)
    for ri in range(c.n_reads):
        st, en = int(c.start[ri]), int(c.end[ri])
        seeds = c.cands(ri)
        n_cand = len(seeds)
        given = dict(seeds=seeds) if c.deep else {}      # the deep set: the read's own list in place of getSeed's
        res = T.assign(c.codes[ri], st, en, O.default_opts(maxError=c.max_error), **given)
        assert sorted(int(x) for x in res["seed_ids"]) == sorted(int(x) for x in seeds)
        assert sorted(int(x) for x in res["filt_order"]) == sorted(int(u) for u, keep in zip(seeds, c.filter_in[ri]) if keep), ri
        if ri not in c.q_reads:
            continue
        for prior in (0, 1):
            for fix in (0, 1):
                res = T.assign(c.codes[ri], st, en, O.default_opts(maxError=1e9, prior=prior, fixRootLoglik=fix), **given)
                assert res["n"] == n_cand
                qp, qt, op, ot = c.q_exact(ri, prior, fix)
                for nodes, vals in zip(res["nodes"], res["vals"]):
                    k = c.slot(ri, nodes[0])                     # narrow / wide: the seeds are the nodes 1 .. n - 1 in order
                    assert int(seeds[k]) == int(nodes[0])
                    assert q_ok(vals[4], qp[k], op[k], 1e-9), (ri, prior, fix, k, vals[4], qp[k])
                    if not ratio_half(c, ri):
                        assert q_ok(vals[5], qt[k], ot[k], 1e-9), (ri, prior, fix, k, vals[5], qt[k])
                    for q, qe, omp in ((vals[4], qp[k], op[k]),) + (() if ratio_half(c, ri) else ((vals[5], qt[k], ot[k]),)):
                        if omp >= 1e-6:                          # the eps of the conditioned bound that this q needs
                            worse(worst, "q_eps", max(0.0, (abs(q - qe) - 1e-12 * qe) * omp * np.log(10.0) / 10.0))
    return worst


# ---- the wide set (tests/golden/hiprec_wide.npz): regions of 512 to 3,073 columns under the same rules and the same fixed bounds
@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_messages(name):
    _messages(Case(name, "wide"))


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_estimate(name):
    c = Case(name, "wide")
    assert c.n_reads == len(WIDE_READS) and not c.knife.any()       # wide regions: the EM converges properly
    report("wide_estimate", name, **_estimate(c))


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_place(name):
    report("wide_place", name, **_place(Case(name, "wide")))


@pytest.mark.parametrize("name", WIDE_CASES)
def test_wide_assign_filter_set_and_q_values(name):
    report("wide_q", name, **_assign(Case(name, "wide")))


# ---- the deep set (tests/golden/hiprec_deep.npz): 1,024 leaves x 96 columns, messages down to -1,420, under the same rules and bounds
def _root_ll(root, pi):
    """treeLoglik of every column from a root message [L][4]: log(pi . exp(root message))"""
    mx = root.max(1)
    return mx + np.log((np.asarray(pi)[None, :] * np.exp(root - mx[:, None])).sum(1))


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_messages(name):
    """the oracle's two-pass pruning and synth's numpy messages where both rescale (src/PhyloTreeUnrooted.h:1495-1510): the old measure
    (1e-11 relative to max(|x|, 1)) and the depth-aware pair hiprec_cases.level_shape.  Level 1e-11: the old bound on the largest
    component.  Shape 1e-9 absolute: the relative error of the linear value that the project asks of a message of magnitude <= 1."""
    _deep_messages(Case(name, "deep"), "deep_messages")


def _deep_messages(c, test):
    name = c.name
    O, m, _ = _oracle(c)
    db = c.db
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up, down, seq, h = O.tree_evaluate(db.parent, db.blen, leaf_only, m, db.dg_r if db.dg_k else None)
    assert np.array_equal(seq, db.seq)
    assert np.abs(h - c.height).max() < 1e-14
    # the archive is deep where it says: stored messages of both kinds below the rescaling level
    whole = len(c.root_ll) == db.cs_len                          # the deepwide archive holds the root log-likelihood at msg_cols only
    assert (c.up.max(-1) < DEEP_LL).any() and (c.down.max(-1) < DEEP_LL).any()
    assert (c.root_ll < DEEP_LL).sum() >= 16 if whole else (c.root_ll.min() < DEEP_LL and (_root_ll(up[0], m.pi) < DEEP_LL).sum() >= 16)
    worst = {}
    for who, (u_, d_) in dict(oracle=(up, down), synth=(db.up, db.down)).items():
        for side, got, want in (("up", u_[c.msg_nodes][:, c.msg_cols], c.up), ("down", d_[c.msg_nodes][:, c.msg_cols], c.down)):
            level, shape = level_shape(got, want)
            inf = np.isneginf(want)
            old = (np.abs(got[~inf] - want[~inf]) / np.maximum(np.abs(want[~inf]), 1.0)).max()
            worst.update({"%s_%s_level" % (who, side): level, "%s_%s_shape" % (who, side): shape, "%s_%s_rel" % (who, side): old})
        ll = _root_ll(u_[0], m.pi)
        worst[who + "_tree_ll"] = max((np.abs((ll if whole else ll[c.msg_cols]) - c.root_ll) / np.abs(c.root_ll)).max(), _rel(ll.sum(), c.root_ll_sum))
    report(test, name, **worst)
    for k, v in worst.items():
        assert np.isfinite(v) and v < (1e-12 if k.endswith("tree_ll") else 1e-9 if k.endswith("shape") else 1e-11), (k, v)


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_estimate(name):
    report("deep_estimate", name, **_estimate(Case(name, "deep")))


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_place(name):
    report("deep_place", name, **_place(Case(name, "deep")))


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_assign_filter_set_and_q_values(name):
    report("deep_q", name, **_assign(Case(name, "deep")))


# ---- the deepwide set (tests/golden/hiprec_deepwide.npz): the deep set's branch lengths on 1,029 leaves x 3,300 columns, seven of the wide
# set's read shapes with twelve given candidates each, under the same rules and bounds
@pytest.mark.parametrize("name", DEEPWIDE_CASES)
def test_deepwide_messages(name):
    _deep_messages(Case(name, "deepwide"), "deepwide_messages")


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
def test_deepwide_estimate(name):
    c = Case(name, "deepwide")
    assert c.n_reads == len(DEEPWIDE_READS) and (c.n_cand >= 8).all() and (c.n_cand <= 12).all()
    report("deepwide_estimate", name, **_estimate(c))


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
def test_deepwide_place(name):
    report("deepwide_place", name, **_place(Case(name, "deepwide")))


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
def test_deepwide_assign_filter_set_and_q_values(name):
    report("deepwide_q", name, **_assign(Case(name, "deepwide")))


def test_the_archive_is_the_generators_output():
    """one candidate regenerated in 50-digit arithmetic gives the stored bits"""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_hiprec_golden", os.path.join(HERE, "golden", "make_hiprec_golden.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    c = Case("JC690")
    ri, k = 2, 4
    got = gen.one_candidate("JC690", ri, int(c.seeds[k]))
    assert tuple(got["dN"]) == tuple(int(x) for x in c.dN[ri, k]) and got["est_d"] == int(c.est_d[ri, k])
    for key in ("est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll"):
        assert got[key] == getattr(c, key)[ri, k], key
    assert (got["pl_outer"], got["pl_em"], got["pl_a_node"]) == (int(c.pl_outer[ri, k]), int(c.pl_em[ri, k]), int(c.pl_a_node[ri, k]))
    assert np.float32(got["margin"]) == c.margin[ri, k] and np.float32(got["state_gap"]) == c.state_gap[ri, k]
    assert np.float32(got["margin_cond"]) == c.margin_cond[ri, k]
    # and a knife-edge one: the conditioned margin that exempts it is the generator's too
    ri, k = (int(x) for x in np.argwhere(c.knife)[0])
    got = gen.one_candidate("JC690", ri, int(c.seeds[k]))
    assert np.float32(got["margin_cond"]) == c.margin_cond[ri, k] < 1 and got["pl_em"] == int(c.pl_em[ri, k])
    assert (got["pl_ratio"], got["pl_wnr"]) == (c.pl_ratio[ri, k], c.pl_wnr[ri, k])
    assert got["pl_const_ll"] == c.pl_const_ll[ri]
    # and one of the wide set: the narrowest read (512 columns) on the cheapest model
    c = Case("JC690", "wide")
    ri, k = 0, 6
    got = gen.one_candidate("JC690", ri, int(c.seeds[k]), "wide")
    assert tuple(got["dN"]) == tuple(int(x) for x in c.dN[ri, k]) and got["est_d"] == int(c.est_d[ri, k])
    for key in ("est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll"):
        assert got[key] == getattr(c, key)[ri, k], key
    assert (got["pl_outer"], got["pl_em"], got["pl_a_node"]) == (int(c.pl_outer[ri, k]), int(c.pl_em[ri, k]), int(c.pl_a_node[ri, k]))
    assert np.float32(got["margin"]) == c.margin[ri, k] and np.float32(got["margin_cond"]) == c.margin_cond[ri, k]
    assert got["pl_const_ll"] == c.pl_const_ll[ri]
    # and one of the deep set: the one-column read (a sweep over the 2,047 nodes at that column) on the cheapest model
    c = Case("JC690", "deep")
    ri, k = 4, 3
    got = gen.one_candidate("JC690", ri, int(c.cands(ri)[k]), "deep")
    assert tuple(got["dN"]) == tuple(int(x) for x in c.dN[ri, k]) and got["est_d"] == int(c.est_d[ri, k])
    for key in ("est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll"):
        assert got[key] == getattr(c, key)[ri, k], key
    assert (got["pl_outer"], got["pl_em"], got["pl_a_node"]) == (int(c.pl_outer[ri, k]), int(c.pl_em[ri, k]), int(c.pl_a_node[ri, k]))
    assert np.float32(got["margin"]) == c.margin[ri, k] and np.float32(got["margin_cond"]) == c.margin_cond[ri, k]
    # and of the deepwide set one message column, the median one of JC69, swept again over its 2,057 nodes: the stored messages of the
    # candidate nodes and the root log-likelihood of that column.  No candidate of that set is regenerated here: its sweep over the 1,024
    # or more columns of a read is a quarter of a CPU-hour.
    c = Case("JC690", "deepwide")
    k = 1
    j = int(c.msg_cols[k])
    part = gen.deep_sweep((DEEPWIDE_CASES.index("JC690"), [j], "deepwide"))
    assert sorted(part["down"]) == [int(u) for u in c.msg_nodes]
    for x, u in enumerate(c.msg_nodes):
        assert [gen.flog(v) for v in part["up"][int(u)][j]] == c.up[x, k].tolist(), u
        assert [gen.flog(v) for v in part["down"][int(u)][j]] == c.down[x, k].tolist(), u
    assert float(part["root_ll"][j]) == c.root_ll[k]


def test_only_the_generator_imports_mpmath():
    pat = re.compile(r"^\s*(import|from)\s+mpmath", re.M)
    root = os.path.dirname(HERE)
    hits = [p for d in ("tests", "oracle", "hmmufotu_amd") for p in glob.glob(os.path.join(root, d, "**", "*.py"), recursive=True)
            if pat.search(open(p).read())]
    assert [os.path.relpath(p, root) for p in hits] == [os.path.join("tests", "golden", "make_hiprec_golden.py")]
