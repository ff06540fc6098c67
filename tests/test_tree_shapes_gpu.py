"""The assignment path over the node dimension of the database: node counts that fill the seed stage's tiles exactly (64, 256, 1,024, 24,064
nodes) or overhang them by one node (257, 1,025), trees with a trifurcating top node and with polytomies, and the root anywhere in node order
(tests/tree_shapes.py).  Every other database of the suite comes from synth.make_tree: an odd node count, the root at node 0, every parent
numbered before its children.

The reference of every comparison is the CPU oracle on the SAME relabelled database (its final pick depends on node ids through the tie rule,
so a permuted database is not compared with the unpermuted run); only a shift of the root, which keeps every other node's relative order,
is also held to the identity run, bit for bit, as the oracle is (test_tree_shapes.py::test_oracle_is_invariant_under_a_shift_of_the_root).

That the seed tests bite was checked once by hand with two one-line mutations of hu_kern_sep.h, each changing a comparison and no address
(neither is committed; the run was the 28 test_seeds_* cases of this module, which all pass on the unchanged kernels):
  1. `node == db.root` -> `node == 0` in the exact pass of k_seed_topk's sampled fast path (the collection of the pairs at or below the estimated
     threshold bin).  10 of the 12 test_seeds_pair_matrix_topk cases fail, every one at a launch with topk_fast_min = 1 and no height filter, after
     its identity numbering had passed: S64-tied, S256-tied, S256p-tied, S257-sharp, S257-tied, S1024-sharp, S1024-tied, S1025-sharp and S1025-tied at
     shift(1), the first numbering behind the identity (the root, now node 1, stands in a seed list), S256p-sharp at `reverse` (a list differs behind
     its eighth seed).  S64-sharp and S256-sharp pass: there the sample holds too few near pairs and the two-pass path takes over.  The distance-only
     and reference-order cases pass, as they must: they do not run the kernel.
  2. `node0 + m != db.root` -> `node0 + m != 0` in k_seed_dscan4 (skip[m]: the root leaves its block's minimum, node 0 now does instead).
     test_seeds_distance_only_scan[S1024-sharp] and [S1025-tied] fail, both at shift(256), 8-bit distances, straight launch, on the row read of the
     root, where node 0 (identity node 1) belongs among the two seeds and is missing; every identity numbering passes, and so do
     [S1024-tied] and [S1025-sharp]: bminD only steers which blocks the top-k reads, and on four or five blocks a block whose minimum is too high is
     usually read anyway.  All pair-matrix and reference-order cases pass.
"""
import re

import numpy as np
import pytest

import tree_shapes as TS
from conftest import get_db, sim_reads

pytestmark = pytest.mark.gpu

FORMS = ("sharp", "tied")


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


def _aligned(E, db, rd, vps, opts, trace=False):
    D = E.Database.from_synth(db)
    assert D.root == TS.root_of(db) and D.n_nodes == db.n_nodes
    B = E.Batch(D, len(rd))
    if trace:
        B.set_knob("trace", 1)
    B.set_reads(rd, vps); B.align(opts)
    return D, B


# ----------------------------------------------------------------------------- a. seeds: every path x every numbering x every small database
KNOBS0 = dict(pairs32=0, topk_fast_min=16384, scan_pairs=0, topk_general=0, refsort_host=0)      # the defaults of HuKnobs


def _seed_variants(path, mh):
    """(label, hu_opts keywords, knobs, the oracle's tie mode) of every launch of a seed path"""
    out = []
    if path == "topk":          # the pair matrix + k_seed_topk: 16- / 32-bit pairs, the exact two-pass path / the sampled fast path, without / with -H
        for wide in (0, 1):
            for fast in (16384, 1):
                for h in (None, mh):
                    out.append(("pairs%d fast_min=%d maxh=%s" % (32 if wide else 16, fast, h), dict(seed_order=0, max_nseed=50, **({} if h is None else dict(max_height=h))),
                                dict(scan_pairs=1, pairs32=wide, topk_fast_min=fast), 0))
    elif path == "dscan":       # the distance-only scan + k_seed_topk_straight / k_seed_topk_d: nBlk >= 2 x max_nseed needs max_nseed = 2 on four blocks
        for wide in (0, 1):
            for gen in (0, 1):
                out.append(("dist%d general=%d" % (16 if wide else 8, gen), dict(seed_order=0, max_nseed=2), dict(scan_pairs=-1, pairs32=wide, topk_general=gen), 0))
    else:                       # the reference's order: the device sort / the host restatement, without / with -H (the compacted rows)
        for host in (0, 1):
            for h in (None, mh):
                out.append(("refsort host=%d maxh=%s" % (host, h), dict(seed_order=1, max_nseed=50, **({} if h is None else dict(max_height=h))), dict(refsort_host=host), 1))
    return out


def _seed_case(name, form, path, capfd):
    E = _engine()
    db0 = TS.make(name, form)
    reads, vps, rows = TS.reads_of(name, form)
    rd = [r.seq for r in reads]
    mh = float(np.median(db0.height))
    variants = _seed_variants(path, mh)
    launches = 0
    for label, m in TS.numberings(db0.n_nodes):
        db = db0 if label == "identity" else TS.relabel(db0, m)
        root = TS.root_of(db)
        _, H, T = TS.oracle_objects(db)
        D, B = _aligned(E, db, rd, vps, E.default_opts(), trace=True)
        try:                                           # a failing case must not leave its device objects to the later ones
            cd, st, en = B.codes()
            want = {}
            for vlabel, okw, knobs, tie in variants:
                opts = E.default_opts(**okw)
                for k, v in dict(KNOBS0, **knobs).items():
                    B.set_knob(k, v)
                capfd.readouterr()
                B.get_seed(opts)
                err = capfd.readouterr().err
                where = (name, form, label, vlabel)
                if path == "dscan":
                    assert D.n_nodes // 256 >= 2 * opts.max_nseed
                    t = re.search(r"(\d+) of (\d+) reads on the block path .* (\d+) by the exact recomputation; (\d+) of them through the general launch", err)
                    assert t and int(t.group(2)) == len(rd) and int(t.group(1)) > 0, (where, err)          # the block path ran
                    assert int(t.group(4)) > 0 or not knobs["topk_general"], (where, err)
                elif path == "refsort":
                    assert ("k_seed_refsort" in err) == (not knobs["refsort_host"]), (where, err)
                else:
                    assert "block path" not in err and "k_seed_refsort" not in err, (where, err)
                cnt, ids, sd, sN = B.seeds()
                mxh = okw.get("max_height", float("inf"))
                for i in range(len(rd)):
                    key = (i, tie, mxh, opts.max_nseed)
                    if key not in want:
                        want[key] = T.get_seed(cd[i], int(st[i]), int(en[i]), max_height=mxh, tie=tie, max_n=opts.max_nseed)
                    oid, od, oN, _ = want[key]
                    k = len(oid)
                    assert cnt[i] == k and k > 0, (where, i, cnt[i], k)
                    assert root not in ids[i, :k], (where, i, ids[i, :k])
                    assert (ids[i, :k] == oid).all(), (where, i, ids[i, :k][:8], oid[:8])
                    assert (sd[i, :k] == od).all() and (sN[i, :k] == oN).all(), (where, i)
                for what, (i, _) in rows.items():                              # the whole row of the scan's matrix for the row reads
                    d, N = B.pdist(i)
                    od, oN = T.pdist_all(cd[i], int(st[i]), int(en[i]))
                    assert (d == od).all() and (N == oN).all(), (where, what)
                launches += 1
        finally:
            B.close(); D.close()
    assert launches == len(variants) * len(TS.numberings(db0.n_nodes))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TS.SMALL)
def test_seeds_pair_matrix_topk(name, form, capfd):
    _seed_case(name, form, "topk", capfd)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["S1024", "S1025"])
def test_seeds_distance_only_scan(name, form, capfd):
    _seed_case(name, form, "dscan", capfd)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TS.SMALL)
def test_seeds_reference_order(name, form, capfd):
    _seed_case(name, form, "refsort", capfd)


# ----------------------------------------------------------------------------- b. fused level 0 of k_seed_refsort
def _large(which):
    return get_db(12000, 260, "JC69", dg_k=0, seed=3, n_match=180) if which == "L23999" else TS.make("L24064")


@pytest.mark.parametrize("which,at", [(w, a) for w in ("L23999", "L24064") for a in range(4)])
def test_fused_level_0_with_the_root_anywhere(which, at, capfd):
    """The 96 reads of test_reference_seed_order_on_a_tree_with_streaming_levels on its tree (23,999 nodes) and on one of 24,064 = 94 x 256 nodes
    (no mask word behind the last node), the root at node 0, inside a mask word (1,000), on a word boundary (12,800) and at the last node (the last
    word; root & 63 = 62 or 63): the device sort with level 0 from the scan's stopper masks against the sort that counts level 0 itself and against the
    host restatement, 16- and 32-bit pairs."""
    E = _engine()
    db0 = _large(which)
    n = db0.n_nodes
    label, m = TS.numberings(n, large=True)[at]
    reads, vps = sim_reads(db0, 96, 100)
    rd = [r.seq for r in reads]
    db = db0 if label == "identity" else TS.relabel(db0, m)
    root = TS.root_of(db)
    assert root == (0, 1000, 12800, n - 1)[at] and (at < 3 or root & 63 in (62, 63))
    D = E.Database.from_synth(db)
    assert D.root == root
    del db
    opts = E.default_opts(seed_order=1)
    for wide in (0, 1):
        lists = []
        for mode in ("fused", "host", "nofuse"):
            B = E.Batch(D, len(rd))
            B.set_knob("pairs32", wide); B.set_knob("refsort_host", int(mode == "host")); B.set_knob("ref_nofuse", int(mode == "nofuse")); B.set_knob("trace", 1)
            capfd.readouterr()
            B.set_reads(rd, vps); B.align(opts); B.get_seed(opts)
            err = capfd.readouterr().err
            if mode != "host":
                assert re.search(r"k_seed_refsort: 96 reads.* %s pairs.* 0 reads left to the host" % ("32-bit" if wide else "16-bit"), err), err
                assert ("level 0 from the scan" in err) == (mode == "fused"), err
                assert B.refsort_stats() == (0, False)
            else:
                assert "k_seed_refsort" not in err
            cnt, ids, sd, sN = B.seeds()
            lists.append((cnt.copy(), ids.copy(), sd.copy(), sN.copy()))
            B.close()
        assert (lists[0][0] == 50).all() and not (lists[0][1] == root).any()
        for other in lists[1:]:
            for a, b in zip(lists[0], other):
                assert np.array_equal(a, b), (which, label, wide)
    D.close()


# ----------------------------------------------------------------------------- c. the whole stage chain against the oracle
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TS.SMALL)
def test_stage_chain_against_the_oracle(name, form, order):
    """test_gpu_parity.sep_parity (seed scan, top-k, estimate, filter, place, q-values, stage by stage, its own bounds) in both seed orders, in the
    identity numbering, with the root at the last node and with every parent behind its children"""
    from test_gpu_parity import sep_parity
    reads, vps, _ = TS.reads_of(name, form)
    n = TS.make(name, form).n_nodes
    for label in ("identity", "shift%d" % (n - 1), "reverse"):
        db, _ = TS.relabelled(name, form, label)
        sep_parity(db, reads, vps, dict(seed_order=order, numbering=label, shape=name, form=form))


# ----------------------------------------------------------------------------- d. a shift of the root against the unshifted run
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _whole_task(E, db, rd, vps, opts, old_of_new):
    """seeds, estimates, candidates and placement records of a run, node ids mapped back to the identity numbering, floats as their bits"""
    back = np.concatenate((old_of_new, [-1]))                  # a -1 (no node) stays -1
    D, B = _aligned(E, db, rd, vps, opts)
    B.get_seed(opts); B.estimate_seq(opts); B.filter_placements(opts); B.place_seq(opts); B.calc_q_values(opts)
    cnt, ids, sd, sN = B.seeds()
    er, ew, el = B.estimates()
    cand = B.candidates()
    best = B.placements()
    coffs, cpl = B.candidate_places()
    live = np.arange(ids.shape[1])[None, :] < cnt[:, None]
    out = dict(seed_cnt=cnt, seed_id=np.where(live, back[np.where(live, ids, -1)], -1), seed_d=np.where(live, sd, 0), seed_N=np.where(live, sN, 0))
    for k, v in (("est_ratio", er), ("est_wnr", ew), ("est_loglik", el)):
        out[k] = np.where(live, _bits(v), 0)
    out["cand_offs"] = cand["offs"]; out["cand_c_node"] = back[cand["c_node"]]; out["cand_iters"] = cand["iters"]
    for k in ("ratio", "wnr", "est_loglik"):
        out["cand_" + k] = _bits(cand[k])
    for what, recs in (("best", best), ("place", cpl)):
        for f in recs.dtype.names:
            out[what + "_" + f] = back[recs[f]] if f in ("c_node", "p_node", "a_node") else _bits(recs[f])
    out["place_offs"] = coffs
    B.close(); D.close()
    return out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TS.SMALL)
def test_shift_of_the_root_against_the_unshifted_run(name, form):
    """every other node keeps its relative order under a shift, so nothing that the task computes may change but the ids: seeds, estimates,
    candidates and placement records equal the identity run's bit for bit (floats compared as integers), in both seed orders.  No tie
    explanation applies."""
    E = _engine()
    db0 = TS.make(name, form)
    reads, vps, _ = TS.reads_of(name, form)
    rd = [r.seq for r in reads]
    for order in (0, 1):
        opts = E.default_opts(seed_order=order)
        base = None
        for label, m in TS.numberings(db0.n_nodes):
            if label != "identity" and not label.startswith("shift"):
                continue
            got = _whole_task(E, db0 if label == "identity" else TS.relabel(db0, m), rd, vps, opts, TS.inverse(m))
            if base is None:
                base = got
                assert (got["seed_cnt"] == 50).all() and (got["best_c_node"] > 0).all()
                continue
            for k, v in got.items():
                assert np.array_equal(v, base[k]), (name, form, order, label, k, np.nonzero(np.atleast_1d(v != base[k]))[0][:6])


# ----------------------------------------------------------------------------- e. the device build
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["S64", "S256p", "S257"])
def test_device_build_on_polytomies_and_under_relabelling(name, form):
    """hu_tree_evaluate against the oracle's general sweep with the assertions of test_tree_pre_evaluation made root-general: every row of up (the
    root's row holds the root message), every non-root row of down, the ancestral states and the heights; whole width and a window.  Children
    are summed in node-id order, so a relabelling may move last bits: each numbering is held to the oracle on the same numbering at 1e-9."""
    E = _engine()
    import torch
    from oracle import oracle_py as O
    db0 = TS.make(name, form)
    n, L = db0.seq.shape
    md = E.model_desc(db0.model.type_id, db0.model.pi, db0.model.par, db0.dg_r if db0.dg_k else None)
    m = O.Model(db0.model.type_id, db0.model.pi, db0.model.par)
    for label in ("identity", "shift%d" % (n - 1), "reverse", "random"):
        db, _ = TS.relabelled(name, form, label)
        root = TS.root_of(db)
        nr = np.arange(n) != root
        leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
        oup, odown, oseq, oh = O.tree_evaluate(db.parent, db.blen, leaf_only, m, db.dg_r if db.dg_k else None)
        for (w0, wl) in ((0, 0), (40, 200)):
            W = wl or L
            up = torch.full((n, W, 4), 7.0, dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
            seq, h = E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr(), w0, wl)
            torch.cuda.synchronize()
            gu, gd = up.cpu().numpy(), down.cpu().numpy()
            ou, od = oup[:, w0:w0 + W], odown[:, w0:w0 + W]
            fin = np.isfinite(ou)
            assert (np.isfinite(gu) == fin).all(), (label, w0)
            assert np.abs(gu[fin] - ou[fin]).max() < 1e-9 * max(1.0, np.abs(ou[fin]).max()), (label, w0)
            assert np.abs(ou[root]).max() > 0 and np.abs(gu[root] - ou[root]).max() < 1e-9 * max(1.0, np.abs(ou[root]).max()), (label, w0)
            assert np.abs(gd[nr] - od[nr]).max() < 1e-9 * max(1.0, np.abs(od[nr]).max()), (label, w0)
            inner = ~db.is_leaf
            assert (seq[inner][:, w0:w0 + W] == oseq[inner][:, w0:w0 + W]).all(), (label, w0)
            assert (seq[db.is_leaf] == leaf_only[db.is_leaf]).all()
            assert np.abs(h - oh).max() < 1e-12 and np.abs(h - db.height).max() < 1e-12, (label, w0)


# ----------------------------------------------------------------------------- f / g. files, and the consensus accumulator's refusal
def test_files_with_a_stored_root_other_than_node_0(tmp_path):
    """S257 with the root at node 64 through hu_ptu_write (its root row) and the .ptu reader: the parsed root is 64 and the loaded database
    assigns exactly as the one made from the arrays; hu_otucs_create refuses it, naming the stored root"""
    E = _engine()
    from hmmufotu_amd import synth
    db, _ = TS.relabelled("S257", "tied", "shift64")
    reads, vps, _ = TS.reads_of("S257", "tied")
    rd = [r.seq for r in reads]
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    hp, pp = str(tmp_path / "t.hmm"), str(tmp_path / "t.ptu")
    synth.write_hmm(db.hmm, hp)
    E.write_ptu(pp, db.parent, db.blen, db.seq, db.up, db.down, db.height, md, names=db.names, annos=db.annos, anno_dist=db.anno_dist,
                model_text=db.model.text, dg_alpha=db.dg_alpha, dg_breaks=db.dg_b)
    parsed = E.parse_files(hp, pp)
    assert parsed["root"] == 64 and parsed["n_nodes"] == 257
    assert np.array_equal(parsed["parent"], db.parent) and np.array_equal(parsed["up"][64], db.up[64]) and np.array_equal(parsed["down"], db.down)
    D1 = E.Database.load(hp, pp)
    D2 = E.Database.from_synth(db)
    assert D1.root == 64 and D2.root == 64
    outs = []
    for D in (D1, D2):
        B = E.Batch(D, len(rd))
        B.set_reads(rd, vps)
        B.assign(E.default_opts())
        outs.append((B.placements().copy(), B.alignments()["align"], [x.copy() for x in B.seeds()]))
        B.close()
    assert outs[0][1] == outs[1][1]
    for a, b in zip(outs[0][2], outs[1][2]):
        assert np.array_equal(a, b)
    assert outs[0][0].tobytes() == outs[1][0].tobytes()                 # the records, bit for bit
    assert (outs[0][0]["c_node"] != 64).all() and (outs[0][0]["n_cand"] > 0).all()
    with pytest.raises(E.EngineError, match=r"hu_otucs_create: the database's stored root is node 64, not node 0"):
        D1.otu_consensus()
    D1.close(); D2.close()
