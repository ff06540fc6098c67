"""The shapes of tests/tree_shapes.py on the CPU: the helper itself, the generator and the oracle on polytomy trees and under relabelling,
and the conditions that make the GPU cases of tests/test_tree_shapes_gpu.py reach what they are for.  No GPU is needed."""
import numpy as np
import pytest

import tree_shapes as TS
from hmmufotu_amd import synth
from oracle import oracle_py as O


def _children(parent):
    return np.bincount(parent[parent >= 0], minlength=len(parent))


@pytest.mark.parametrize("name", list(TS.SHAPES))
def test_tree_has_its_node_count_preorder_numbering_and_child_counts(name):
    n_leaves, top, splice, n_nodes, tseed, _ = TS.SHAPES[name]
    parent, blen, is_leaf = TS.tree(n_leaves, top, splice, tseed)
    n = len(parent)
    assert n == n_nodes == 2 * n_leaves - 1 - splice - (top == 3) and int(is_leaf.sum()) == n_leaves
    assert parent[0] == -1 and (parent[1:] >= 0).all() and (parent[1:] < np.arange(1, n)).all()
    # preorder: a node's subtree is the run of ids right behind it
    size = np.ones(n, np.int64)
    for u in range(n - 1, 0, -1):
        size[parent[u]] += size[u]
    for u in range(1, n):
        p = parent[u]
        assert p < u < p + size[p]
    kids = _children(parent)
    assert kids[0] == top and (kids[is_leaf] == 0).all() and (kids[~is_leaf] >= 2).all()
    assert int((kids - 2)[~is_leaf].sum()) == splice + (top == 3)          # every spliced node left one more child at its parent
    if splice:
        assert (kids[1:] > 2).any()                                        # a polytomy below the top
    else:
        assert (kids[1:][~is_leaf[1:]] == 2).all()
    assert blen[0] == 0 and (blen[1:] >= 1e-5).all()


def test_make_db_without_the_keyword_is_what_it_was():
    """tree=None leaves the generator's stream alone (the committed goldens pin the whole database; this pins the call next to the keyword)"""
    a = synth.make_db(12, 60, "GTR", dg_k=4, seed=5)
    rng = np.random.default_rng(5)
    t = synth.make_tree(12, rng)
    assert np.array_equal(a.parent, t[0]) and np.array_equal(a.blen, t[1])


@pytest.mark.parametrize("name", ["S64", "S257"])
def test_relabel_and_its_inverse_are_the_identity(name):
    db = TS.make(name, "tied")
    n = db.n_nodes
    for label, m in TS.numberings(n):
        r = TS.relabel(db, m)
        root = TS.root_of(r)
        assert root == m[0] and (r.parent[m[1:]] == m[db.parent[1:]]).all()
        if label.startswith("shift"):
            others = np.delete(np.arange(n), root)
            assert np.array_equal(TS.inverse(m)[others], np.arange(1, n))          # every other node in its relative order
        if label == "reverse":
            assert root == n - 1 and (r.parent[:-1] > np.arange(n - 1)).all()       # every parent behind its children
        back = TS.relabel(r, TS.inverse(m))
        for f in ("parent", "blen", "seq", "up", "down", "height", "is_leaf", "anno_id", "anno_dist"):
            assert np.array_equal(getattr(back, f), getattr(db, f)), (label, f)
        assert back.names == db.names and back.annos == db.annos
        assert sorted(r.anno_id.tolist()) == sorted(db.anno_id.tolist())             # labels, not node ids: permuted, never mapped
    assert [x for _, x in TS.numberings(n)][1][0] == 1


@pytest.mark.parametrize("name", ["S64", "S256p", "S257"])
@pytest.mark.parametrize("form", ["sharp", "tied"])
def test_messages_on_polytomy_trees(name, form):
    """synth.evaluate_tree (children lists of any length) against the oracle's general sweep, in the identity numbering and with every parent
    behind its children; the bounds of test_tree_pre_evaluation.  The root's message stands in the root's row of up wherever the root is."""
    db0 = TS.make(name, form)
    m = O.Model(db0.model.type_id, db0.model.pi, db0.model.par)
    for label in ("identity", "reverse"):
        db, _ = TS.relabelled(name, form, label)
        root = TS.root_of(db)
        leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
        oup, odown, oseq, oh = O.tree_evaluate(db.parent, db.blen, leaf_only, m, db.dg_r if db.dg_k else None)
        fin = np.isfinite(oup)
        assert (np.isfinite(db.up) == fin).all()
        assert np.abs(db.up[fin] - oup[fin]).max() < 1e-9 * max(1.0, np.abs(oup[fin]).max())
        nr = np.arange(db.n_nodes) != root
        assert np.abs(db.down[nr] - odown[nr]).max() < 1e-9 * max(1.0, np.abs(odown[nr]).max())
        assert np.abs(oup[root]).max() > 0                                          # the root row is the root message, not an empty row
        assert (db.seq == oseq).all()
        assert np.abs(db.height - oh).max() < 1e-12


@pytest.mark.parametrize("form", ["sharp", "tied"])
def test_oracle_is_invariant_under_a_shift_of_the_root(form):
    """the yardstick of the GPU module's shift-against-identity test: the oracle's whole task on every shift of S257 gives the identity run's
    node ids after mapping and bit-equal values"""
    db0 = TS.make("S257", form)
    reads, vps, _ = TS.reads_of("S257", form)
    rd = [r.seq for r in reads]
    runs = {}
    for label, m in TS.numberings(db0.n_nodes):
        if label not in ("identity",) and not label.startswith("shift"):
            continue
        db = db0 if label == "identity" else TS.relabel(db0, m)
        _, H, T = TS.oracle_objects(db)
        for order in (0, 1):
            oo = O.default_opts(tieMode=order)
            p1 = O.pipeline_batch(H, T, rd, vps, opts=oo, mode=1)
            res = O.pipeline_batch(H, T, rd, vps, opts=oo, want_cands=True)
            back = np.concatenate((TS.inverse(m), [-1]))                             # -1 (padding) stays -1
            got = dict(seed_cnt=p1["seed_cnt"], seed_ids=back[p1["seed_ids"]], best_nodes=back[res["best_nodes"][:, :3]], iters=res["best_nodes"][:, 3],
                       best_vals=res["best_vals"].view(np.int64), n_cand=res["n_cand"], cand_node=back[res["cand_node"]], best_pos=res["best_pos"],
                       cand_est=res["cand_est"].view(np.int64), cand_ratio0=res["cand_ratio0"].view(np.int64), cand_placed=res["cand_placed"].view(np.int64))
            if label == "identity":
                runs[order] = got
                assert (got["seed_cnt"] == 50).all() and (got["n_cand"] > 0).all()
            else:
                for k, v in got.items():
                    assert np.array_equal(v, runs[order][k]), (label, order, k)


def _row_pdist(H, T, read, vp):
    a = H.align(read.seq, vp)
    assert a["ok"]
    cd = O.digitize(a["align"])
    s, e = a["csStart"] - 1, a["csEnd"] - 1
    d, N = T.pdist_all(cd, s, e)
    assert (N > 0).all()
    return cd, s, e, d / N


@pytest.mark.parametrize("name", TS.SMALL)
@pytest.mark.parametrize("form", ["sharp", "tied"])
def test_every_case_reaches_what_it_is_for(name, form):
    """A condition, not a measurement.  Sharp: the row read of the root has the root as the strict minimum of d / N over all nodes (hence of its
    block of 256: a kernel that fails to skip the root puts it first), and the row read of identity node 1 has that node first in the oracle's
    seed list, in both seed orders.  Tied: the root's row read has the root inside a tie of at least three nodes at the minimum distance.
    Under every numbering.  A generator seed that does not give this is replaced in tree_shapes.SHAPES; the condition stays."""
    db0 = TS.make(name, form)
    reads, vps, rows = TS.reads_of(name, form)
    for r in reads[24:]:
        assert 80 <= len(r.seq) <= 100
    assert [rows[w][1] for w in TS.ROW_NODES] == [0, 1, db0.n_nodes - 1, db0.n_nodes // 2]
    for label, m in TS.numberings(db0.n_nodes):
        db = db0 if label == "identity" else TS.relabel(db0, m)
        _, H, T = TS.oracle_objects(db)
        root = TS.root_of(db)
        i, node = rows["root"]
        cd, s, e, dist = _row_pdist(H, T, reads[i], vps[i])
        others = np.arange(db.n_nodes) != root
        if form == "sharp":
            assert dist[root] < dist[others].min(), (label, dist[root], dist[others].min())
            blk = np.arange(db.n_nodes) // 256 == root // 256
            assert dist[root] < dist[blk & others].min() if (blk & others).any() else True
            i1, node1 = rows["node1"]
            cd, s, e, _ = _row_pdist(H, T, reads[i1], vps[i1])
            for tie in (0, 1):
                assert T.get_seed(cd, s, e, tie=tie)[0][0] == m[node1], (label, tie)
        else:
            assert dist[root] == dist.min() and int((dist == dist[root]).sum()) >= 3, (label, int((dist == dist[root]).sum()))
        for tie in (0, 1):
            assert root not in T.get_seed(cd, s, e, tie=tie)[0]
