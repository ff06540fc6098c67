"""Tree shapes and node numberings that synth.make_tree cannot produce (plain numpy; a helper module, not a conftest).

make_tree gives a binary tree with a bifurcating root (an odd node count), the root at node 0 and every parent numbered before its
children.  Here: trees with a trifurcating top node and with polytomies below it (even node counts, among them whole multiples of the
seed stage's tiles: 64 nodes = one mask word of k_seed_refsort, 256 = HU_NODE_PAD, 1,024 = one k_seed_dscan4 workgroup), and
relabellings of a database that put the root anywhere in node order.

Reads are always simulated on the identity numbering (synth.simulate_reads assumes root 0); the same strings serve every relabelling of
that database, because neither the profile nor the columns depend on node ids."""
import copy

import numpy as np

from hmmufotu_amd import synth


# ----------------------------------------------------------------------------- trees
def tree(n_leaves, top=2, splice=0, seed=0):
    """A synth.make_tree tree; top == 3: one inner child of the root spliced out (a trifurcating top node, as FastTree writes);
    then `splice` further inner non-root nodes spliced out.  The children of a spliced node go to its parent, in its place among the
    parent's children, with their own lengths.  Renumbered in preorder.  Returns (parent, blen, is_leaf) with
    n_nodes = 2 * n_leaves - 1 - (number of spliced nodes)."""
    assert top in (2, 3)
    rng = np.random.default_rng(seed)
    parent, blen, is_leaf = synth.make_tree(n_leaves, rng)
    n = len(parent)
    kids = [[] for _ in range(n)]
    for u in range(1, n):
        kids[parent[u]].append(u)
    par = [int(p) for p in parent]
    gone = np.zeros(n, bool)

    def cut(v):
        p = par[v]
        at = kids[p].index(v)
        kids[p][at:at + 1] = kids[v]
        for c in kids[v]:
            par[c] = p
        kids[v] = []
        gone[v] = True

    if top == 3:
        inner = [c for c in kids[0] if not is_leaf[c]]
        assert inner, "the root has no inner child to splice out: take another seed"
        cut(inner[int(rng.integers(len(inner)))])
    for _ in range(splice):
        inner = [u for u in range(1, n) if not is_leaf[u] and not gone[u]]
        cut(inner[int(rng.integers(len(inner)))])
    m = n - int(gone.sum())
    new_parent = np.full(m, -1, np.int32); new_blen = np.zeros(m); new_leaf = np.zeros(m, bool)
    stack = [(0, -1)]
    k = 0
    while stack:
        u, p = stack.pop()
        new_parent[k] = p; new_blen[k] = blen[u]; new_leaf[k] = is_leaf[u]
        for c in reversed(kids[u]):
            stack.append((c, k))
        k += 1
    assert k == m
    return new_parent, new_blen, new_leaf


# name -> (n_leaves, top, splice, node count, tree seed, database seed).  The node count is what the shape is the edge of (the table of DESIGN.md
# section 4).  The seeds are chosen so that the conditions of test_tree_shapes.py::test_every_case_reaches_what_it_is_for hold.
SHAPES = {
    "S64": (33, 3, 0, 64, 1, 17),          # one full mask word, a quarter block
    "S256": (129, 3, 0, 256, 1, 1),        # nNodes == nNodesPad: one block, no padding
    "S256p": (130, 2, 3, 256, 1, 34),      # the same with polytomies below the top
    "S257": (129, 2, 0, 257, 1, 1),        # one node in the second block
    "S1024": (513, 3, 0, 1024, 1, 1),      # one k_seed_dscan4 workgroup exactly; nBlk = 4
    "S1025": (513, 2, 0, 1025, 1, 1),      # a second workgroup for one node
    "L24064": (12033, 3, 0, 24064, 1, 3),  # 94 x 256: no mask word behind the last node (the streaming levels of k_seed_refsort)
}
SMALL = ("S64", "S256", "S256p", "S257", "S1024", "S1025")
FORMS = {"sharp": ("JC69", 0), "tied": ("GTR", 4)}    # sharp: distances that single a node out; tied: many nodes at the same distance

_CACHE = {}


def make(name, form="sharp"):
    """The SynthDB of a shape (identity numbering: preorder, root 0), memoised per session.  Small shapes: cs_len 300, 200 match columns."""
    key = ("db", name, form)
    if key not in _CACHE:
        n_leaves, top, splice, n_nodes, tseed, dseed = SHAPES[name]
        model, dg_k = FORMS[form]
        t = tree(n_leaves, top, splice, tseed)
        assert len(t[0]) == n_nodes
        if name == "L24064":
            _CACHE[key] = synth.make_db(n_leaves, 260, model, dg_k=dg_k, seed=dseed, n_match=180, tree=t)
        else:
            _CACHE[key] = synth.make_db(n_leaves, 300, model, dg_k=dg_k, seed=dseed, n_match=200, tree=t)
    return _CACHE[key]


# ----------------------------------------------------------------------------- numberings
def shift(n, r):
    """new_of_old: the root (node 0) at place r, every other node in its relative order"""
    assert 0 <= r < n
    m = np.arange(n, dtype=np.int64)
    m[1:r + 1] -= 1
    m[0] = r
    return m


def reverse(n):
    """new_of_old: every parent behind its children, the root last"""
    return np.arange(n - 1, -1, -1, dtype=np.int64)


def random(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def inverse(new_of_old):
    inv = np.empty(len(new_of_old), np.int64)
    inv[new_of_old] = np.arange(len(new_of_old))
    return inv


def relabel(db, new_of_old):
    """A copy of the database with node i called new_of_old[i]: the node axis of every per-node field permuted, the values of parent
    mapped.  anno_id values stay: they are labels of taxonomy classes, not node ids."""
    new_of_old = np.asarray(new_of_old, np.int64)
    n = db.n_nodes
    assert sorted(new_of_old.tolist()) == list(range(n))
    old_of_new = inverse(new_of_old)
    out = copy.copy(db)
    for f in ("blen", "seq", "up", "down", "height", "is_leaf", "anno_id", "anno_dist"):
        v = getattr(db, f)
        if v is not None:
            setattr(out, f, np.ascontiguousarray(v[old_of_new]))
    for f in ("names", "annos"):
        v = getattr(db, f)
        if v is not None:
            setattr(out, f, [v[i] for i in old_of_new])
    p = db.parent[old_of_new]
    out.parent = np.where(p >= 0, new_of_old[np.maximum(p, 0)], -1).astype(np.int32)
    return out


def numberings(n, large=False):
    """(label, new_of_old) of every numbering the tests run a database of n nodes under"""
    if large:
        return [("identity", np.arange(n, dtype=np.int64))] + [("shift%d" % r, shift(n, r)) for r in (1000, 12800, n - 1)]
    out = [("identity", np.arange(n, dtype=np.int64))]
    out += [("shift%d" % r, shift(n, r)) for r in sorted({1, 3, 63, 64, 255, 256, 1023, n - 1}) if r < n]
    out += [("reverse", reverse(n)), ("random", random(n, 29))]
    return out


def relabelled(name, form, label):
    """(database, new_of_old) of a small shape under one of its numberings (not kept: a relabelling costs milliseconds, its messages megabytes)"""
    db = make(name, form)
    m = dict(numberings(db.n_nodes))[label]
    return (db if label == "identity" else relabel(db, m)), m


def root_of(db):
    return int(np.nonzero(db.parent < 0)[0][0])


# ----------------------------------------------------------------------------- reads
def row_read(db, node, start=20, n_bases=90):
    """A read cut from a node's own row: its bases at match columns start .. start + n_bases - 1 of the profile (a leaf's gaps left out)"""
    cols = (db.hmm.p2cs[1 + start:1 + start + n_bases] - 1).astype(np.int64)
    cols = cols[db.seq[node, cols] >= 0]
    s = synth.BASES[db.seq[node, cols]].tobytes().decode()
    return synth.SimRead(s, cols, int(node), 0.0, int(cols[0]), int(cols[-1]))


ROW_NODES = ("root", "node1", "last", "mid")


def reads_of(name, form):
    """The reads of a small database, drawn on its identity numbering: 24 amplicon reads of up to 100 bases, then row reads (80 to 100
    bases) of the root, of identity node 1 (place 0 under every shift), of the last node and of one mid node.
    Returns (reads, vpaths, {row name: (read index, identity node)})."""
    key = ("reads", name, form)
    if key not in _CACHE:
        from conftest import sim_reads
        db = make(name, form)
        reads, _ = sim_reads(db, 24, 100)
        rows = {}
        for k, (what, node, nb) in enumerate((("root", 0, 90), ("node1", 1, 96), ("last", db.n_nodes - 1, 100), ("mid", db.n_nodes // 2, 84))):
            rows[what] = (len(reads), node)
            reads.append(row_read(db, node, 20 + 3 * k, nb))
        vps = np.stack([synth.read_vpaths(db.hmm, r) for r in reads])
        _CACHE[key] = (reads, vps, rows)
    return _CACHE[key]


def oracle_objects(db):
    from conftest import oracle_objects as oo
    return oo(db)
