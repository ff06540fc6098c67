"""hmmufotu-amd-build --no-hmm: MSA + tree -> <NAME>.ptu (src/hmmufotu-build.cpp:307-503 without the csfm, hmm and msa parts).

CPU part: the Newick reader against synth.parse_newick's numbering and hand cases of the grammar (src/NewickTree.h:186-215), the
annotation steps against a Python restatement written here from src/PhyloTreeUnrooted.cpp:223-240 and :956-1006, the oracle's
ancestral rows against synth.evaluate_tree's inside the tie cap the GPU part relies on, and the program's refusals (no device).
GPU part: the program end to end on the reference's 70_otus fixture (JC69, GTR, GTR -V -k 4) and on a hand tree, read back and
compared with the oracle; hu_ptu_write_stream against hu_ptu_write; hu_tree_loglik against numpy; the built database under
hmmufotu-amd and the engine.

The hand Newick holds a quoted label with a blank, 'D d'.  A FASTA id is the first word of its header, so no MSA row can carry that
name: the parser cases keep the blank, the cases that join an MSA to the tree write the label as 'D-d' (still quoted)."""
import functools
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import get_db
from hmmufotu_amd import engine as E, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-build")
CLI = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70, TREE70, TAX70 = (os.path.join(REF, f) for f in ("70_otus.fasta.gz", "70_otus.tree", "70_otus_taxonomy.txt"))
HAND = "((A:0.1,B:0.2)0.95:0.05,C:0,'D d':-0.01,(E:0.3,F)k__Bacteria:0.2);"
HAND_JOIN = HAND.replace("'D d'", "'D-d'")


def sm(model):
    return os.path.join(REF, "gg_97_otus_%s.sm" % model)


# ----------------------------------------------------------------------------- Newick
def test_newick_70otus_numbering_and_child_order():
    _, nwk = synth.load_70otus()
    t = E.newick_parse(open(TREE70).read())
    parent, blen, names = synth.parse_newick(nwk)
    assert np.array_equal(t["parent"], parent) and np.array_equal(t["blen"], blen) and t["names"] == names
    assert len(parent) == 249
    for u, ch in enumerate(t["children"]):
        assert list(ch) == sorted(ch, reverse=True) and all(parent[c] == u for c in ch)      # file order = descending id
    assert sum(len(c) for c in t["children"]) == 248 and max(len(c) for c in t["children"]) >= 2


@pytest.mark.parametrize("text", [HAND, " (\n( A : 0.1 ,\tB:0.2 ) 0.95 :0.05 ,\nC :0, 'D d' : -0.01,( E:0.3 , F )\r\nk__Bacteria: 0.2 )\n ;\n\n"])
def test_newick_hand_cases(text):
    t = E.newick_parse(text)
    # root 0; its four children pushed in file order, so the last one, (E,F)k__Bacteria, is numbered first
    assert t["names"] == ["", "k__Bacteria", "F", "E", "D d", "C", "0.95", "B", "A"]
    assert list(t["parent"]) == [-1, 0, 1, 1, 0, 0, 0, 6, 6]
    assert list(t["blen"]) == [0.0, 0.2, 0.0, 0.3, -0.01, 0.0, 0.05, 0.2, 0.1]     # F: missing length; root: 0
    assert [list(c) for c in t["children"]] == [[6, 5, 4, 1], [3, 2], [], [], [], [], [8, 7], [], []]
    assert list(t["child_off"]) == [0, 4, 6, 6, 6, 6, 6, 8, 8, 8] and list(t["child_idx"]) == [6, 5, 4, 1, 3, 2, 8, 7]


def test_newick_single_leaf_and_numbers():
    t = E.newick_parse("(A);")
    assert t["names"] == ["", "A"] and list(t["parent"]) == [-1, 0] and list(t["blen"]) == [0.0, 0.0] and [list(c) for c in t["children"]] == [[1], []]
    t = E.newick_parse("(a:1e-3,b:.5,(c:+2,d:3.)x:1E2)r:7;")
    assert t["names"] == ["r", "x", "d", "c", "b", "a"] and list(t["blen"]) == [0.0, 100.0, 3.0, 2.0, 0.5, 1e-3]   # the root's own length is not kept


@pytest.mark.parametrize("text,offset", [("((A,B);", 6), ("(A,B);x", 6), ("", 0), (" \n", 2), ("(A,B)", 5), ("(A,B));", 5), ("(A:,B);", 3), ("(A,'B);", 7),
                                         ("(A B);", 3), ("(A,[c]B);", 3)])
def test_newick_refusals_name_the_offset(text, offset):
    with pytest.raises(E.EngineError) as ei:
        E.newick_parse(text)
    assert "error -3" in str(ei.value) and "at byte %d" % offset in str(ei.value), str(ei.value)


# ----------------------------------------------------------------------------- annotation: restated from src/PhyloTreeUnrooted.cpp:223-240, :956-1006
_PREFIX = ("d__", "k__", "p__", "c__", "o__", "f__", "g__", "s__")       # DOMAIN .. SPECIES, src/PhyloTreeUnrooted.cpp:73-80
_LEVEL = ("k__", "p__", "c__", "o__", "f__", "g__", "s__")             # TaxonLevel: Kindom .. Species; any further level has the prefix ""


def _fields(s):
    """boost::split(., is_any_of(";: "), token_compress_on): a run of separators is one cut; a cut at either end leaves an empty field"""
    out, insep = [""], False
    for c in s:
        if c in ";: ":
            if not insep:
                out.append("")
            insep = True
        else:
            out[-1] += c; insep = False
    return out


def _canonical(x):
    return len(x) > 3 and x.startswith(_PREFIX)


def _full(s):
    return all(f.startswith(_LEVEL[i] if i < 7 else "") for i, f in enumerate(_fields(s)))


def _partial(s):
    return all(_canonical(f) for f in _fields(s))


def py_annotate(parent, blen, names, anno_text=None, root_name="cellular_organisms"):
    names = list(names)
    if anno_text is not None:
        lines = anno_text.split("\n")
        if lines[-1] == "":
            lines.pop()
        m, anno = {}, ""
        for line in lines:
            parts = line.split("\t")
            if len(parts) > 1:                  # a line without a TAB leaves `anno` as the line before set it (getline on an exhausted stream)
                anno = parts[1]
            m[parts[0]] = anno
        names = [m.get(x, x) for x in names]
    names = [x if not x else ";".join(f for f in _fields(x) if _canonical(f)) for x in names]      # formatTaxonName
    annos, dist = [], np.zeros(len(parent))
    for i in range(len(parent)):
        path, p = [], i
        while not _full(names[p]) and parent[p] >= 0:
            dist[i] += blen[p]
            if _partial(names[p]):
                path.append(names[p])
            p = parent[p]
        if _full(names[p]):
            path.append(names[p])
        annos.append(";".join(reversed(path)) if path else root_name)
    return names, annos, dist


@functools.lru_cache(None)
def tree70():
    t = E.newick_parse(open(TREE70).read())
    is_leaf = np.array([len(c) == 0 for c in t["children"]])
    blen = t["blen"].copy()
    blen[is_leaf & (t["parent"] >= 0) & (blen <= 0)] = 1e-5          # fixBranchLength
    return t, is_leaf, blen


def test_annotate_70otus():
    t, is_leaf, blen = tree70()
    tax = open(TAX70).read()
    for root_name in (None, "other"):
        names, annos, dist = E.tree_annotate(t["parent"], blen, t["names"], tax, root_name)
        rn, ra, rd = py_annotate(t["parent"], blen, t["names"], tax, root_name or "cellular_organisms")
        assert names == rn and annos == ra and np.array_equal(dist, rd)            # the same serial sums: bit-equal
    assert annos[0] == "other" and "k__Bacteria;p__" in "".join(annos) and (dist > 0).any() and (dist[1:] == 0).any()
    assert all(" " not in a and ":" not in a for a in names)
    # without a file the leaves keep their numeric names, which formatName empties
    names, annos, dist = E.tree_annotate(t["parent"], blen, t["names"], None)
    rn, ra, rd = py_annotate(t["parent"], blen, t["names"], None)
    assert names == rn and annos == ra and np.array_equal(dist, rd) and all(names[i] == "" for i in np.nonzero(is_leaf)[0])


def test_annotate_hand_tree():
    #        0 ""  ── 1 full ── 2 partial ── 3 partial after a dropped field ── 4 L1 (full through the file), 5 L2 (no line)
    #            └── 6 "" ── 7 L3 (unnamed path to the root), 8 d__X (canonical, never full)
    parent = np.array([-1, 0, 1, 2, 3, 3, 0, 6, 6], np.int32)
    blen = np.array([0, 0.5, 0.25, 0.125, 0.1, 0.3, 0.7, 0.011, 0.013])
    names = ["", "k__Bacteria; p__Firmicutes", "c__Bacilli", "g__:x__foo; o__Lactobacillales", "L1", "L2", "0.87", "L3", "d__Xenobia"]
    tax = "L1\tk__Bacteria; p__Firmicutes; c__Bacilli; o__Lactobacillales; f__; g__; s__\nnobody\tk__Archaea\nL3\n"
    for rn in (None, "other"):
        got = E.tree_annotate(parent, blen, names, tax, rn)
        ref = py_annotate(parent, blen, names, tax, rn or "cellular_organisms")
        assert got[0] == ref[0] and got[1] == ref[1] and np.array_equal(got[2], ref[2])
        root = rn or "cellular_organisms"
        assert got[0] == ["", "k__Bacteria;p__Firmicutes", "c__Bacilli", "o__Lactobacillales", "k__Bacteria;p__Firmicutes;c__Bacilli;o__Lactobacillales", "", "",
                          "k__Archaea", "d__Xenobia"]        # "L3" has no TAB: it takes the annotation of the line before it
        assert got[1] == [root, "k__Bacteria;p__Firmicutes", "k__Bacteria;p__Firmicutes;c__Bacilli", "k__Bacteria;p__Firmicutes;c__Bacilli;o__Lactobacillales",
                          "k__Bacteria;p__Firmicutes;c__Bacilli;o__Lactobacillales", "k__Bacteria;p__Firmicutes;c__Bacilli;o__Lactobacillales", root,
                          "k__Archaea", "d__Xenobia"]
        assert list(got[2]) == [0, 0, 0.25, 0.125 + 0.25, 0, 0.3 + 0.125 + 0.25, 0.7, 0, 0.013 + 0.7]


# ----------------------------------------------------------------------------- the oracle's ancestral rows and the tie cap
def tie_cells(got, oseq, omsg, inner):
    """the cells of inner rows where `got` differs from the oracle's rows; every one must be DESIGN.md section 4's tie: the oracle's
    own message holds the two components within 1e-9 and `got` names the earlier one.  Returns (differing, inner cells)."""
    g, o = got[inner].astype(int), oseq[inner].astype(int)
    uu, jj = np.nonzero(g != o)
    msg = omsg[inner]
    for u, j in zip(uu, jj):
        assert g[u, j] < o[u, j] and abs(msg[u, j, g[u, j]] - msg[u, j, o[u, j]]) < 1e-9, (u, j, msg[u, j])
    return len(uu), g.size


@functools.lru_cache(None)
def oracle70(model, dg=None):
    """(db, oracle up, down, seq, heights) of the 70_otus fixture under one model; dg: (K, alpha) of synth.dgamma or None"""
    from oracle import oracle_py as O
    db = synth.make_db_70otus(model)
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    return (db,) + tuple(O.tree_evaluate(db.parent, db.blen, leaf_only, m, None))


@pytest.mark.parametrize("model", ["JC69", "GTR"])
def test_oracle_rows_against_numpy_inside_the_tie_cap(model):
    db, oup, odown, oseq, oh = oracle70(model)
    inner = ~db.is_leaf
    differ, cells = (int((db.seq[inner] != oseq[inner]).sum()), int(inner.sum()) * db.cs_len)
    print("70_otus %s: oracle vs numpy ancestral cells differing: %d of %d" % (model, differ, cells))
    assert differ * 100 < cells
    assert (db.n_nodes, db.cs_len) == (249, 1486)


# ----------------------------------------------------------------------------- the program's refusals: no device, no .ptu
def write_fasta(path, rows):
    with open(path, "w") as f:
        for name, s in rows:
            f.write(">%s some description\n" % name)
            for a in range(0, len(s), 70):
                f.write(s[a:a + 70] + "\n")


def hand_rows(rng=None, width=300):
    """6 rows for the hand tree: all-gap columns, IUPAC and lower-case letters, '.' gaps, leading / trailing gap runs"""
    rng = rng or np.random.default_rng(5)
    a = rng.choice(list("ACGT"), size=(6, width))
    a[rng.random((6, width)) < 0.08] = "-"
    a[rng.random((6, width)) < 0.03] = "."
    for ch in "RYKMSWBDHVNU":
        a[rng.integers(0, 6), rng.integers(0, width, 3)] = ch
    low = rng.random((6, width)) < 0.2
    a = np.where(low, np.char.lower(a), a)
    a[:, [0, 1, 57, 58, 59, 120, width - 1]] = "-"; a[:, 200] = "."           # columns MSA::prune drops
    a[0, :17] = "-"; a[3, -23:] = "."; a[5, :9] = "."; a[5, -4:] = "-"       # leading / trailing runs
    a[1, 130] = "A"; a[:1, 130] = "-"; a[2:, 130] = "-"                       # a column one lower-case-free residue keeps
    return [(nm, "".join(r)) for nm, r in zip(["A", "B", "C", "D-d", "E", "F"], a)]


def run_build(args, cwd):
    return subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=120)


@pytest.fixture()
def hand_inputs(tmp_path):
    fa, tr = tmp_path / "hand.fasta", tmp_path / "hand.tree"
    write_fasta(fa, hand_rows())
    tr.write_text(HAND_JOIN + "\n")
    return tmp_path, fa, tr


def _refused(r, tmp, *words):
    assert r.returncode != 0, r.stderr
    lines = [x for x in r.stderr.strip().split("\n") if x]
    assert len(lines) == 1 and all(w in lines[0] for w in words), r.stderr
    assert not [f for f in os.listdir(tmp) if f.endswith((".ptu", ".hmm", ".msa", ".csfm"))]


def test_program_is_built():
    assert os.path.exists(BIN), "hmmufotu-amd-build missing: run __graft_entry__.build()"


def test_refusals_of_options(hand_inputs):
    tmp, fa, tr = hand_inputs
    ok = ["--no-hmm", "-sm", sm("GTR"), "-n", "db"]
    _refused(run_build([fa, tr, "-sm", sm("GTR"), "-n", "db"], tmp), tmp, "profile training is not provided here; pass --no-hmm and supply <NAME>.hmm (HMMER3 or hmmufotu-train-hmm)")
    _refused(run_build([fa, tr, "--no-hmm", "-s", "GTR", "-n", "db"], tmp), tmp, "-s", "GTR", "-sm", "data directory")
    for k in ("1", "9"):
        _refused(run_build([fa, tr] + ok + ["-V", "-k", k], tmp), tmp, "-k must be an integer between 2 and 8")
    nwk = tmp / "x.nwk"; nwk.write_text(HAND_JOIN)
    _refused(run_build([fa, nwk] + ok, tmp), tmp, "Unrecognized TREE-FILE format, must be in Newick format")
    _refused(run_build([fa, tr] + ok + ["--fmt", "fastq"], tmp), tmp, "Unsupported sequence format 'fastq'")
    _refused(run_build([fa, tr] + ok + ["-a", tmp / "no_such_taxonomy.txt"], tmp), tmp, "Unable to open", "no_such_taxonomy.txt")
    bad = tmp / "bad.tree"; bad.write_text("((A,B);")
    _refused(run_build([fa, bad] + ok, tmp), tmp, "Unable to read Newick tree", "at byte 6")


def test_refusals_of_inputs(hand_inputs):
    tmp, fa, tr = hand_inputs
    ok = ["--no-hmm", "-sm", sm("JC69"), "-n", "db"]
    rows = hand_rows()
    f2 = tmp / "five.fasta"; write_fasta(f2, rows[:3] + rows[4:])                 # leaf D-d has no row
    _refused(run_build([f2, tr] + ok, tmp), tmp, "Unmatched MSA and Tree. Found 5 leaf sequences from MSA but expecting 6 leaves in the Phylogenetic Tree")
    f3 = tmp / "twice.fasta"; write_fasta(f3, rows + [rows[1]])
    _refused(run_build([f3, tr] + ok, tmp), tmp, "Non-unique seq name B found in your MSA data")
    f4 = tmp / "ragged.fasta"; write_fasta(f4, rows[:5] + [("F", rows[5][1][:-1])])
    _refused(run_build([f4, tr] + ok, tmp), tmp, "Unable to load MSA", "299 columns")


# ============================================================================= GPU
def read_ptu(path, dg_k=0, want_msgs=True):
    """the whole .ptu as PTUnrooted::save lays it out (src/PhyloTreeUnrooted.cpp:537-567), the tail included"""
    b = open(path, "rb").read()
    o = [0]

    def get(fmt):
        v = struct.unpack_from("<" + fmt, b, o[0]); o[0] += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def s():
        k = get("Q"); v = b[o[0]:o[0] + k]; o[0] += k
        return v

    assert b[:8] == b"HmmUFOtu"; o[0] = 8
    ver = get("3i"); n = get("Q"); L = get("i")
    nodes = []
    for i in range(n):
        assert get("q") == i
        name = s(); assert get("?") is False
        seqname = s(); seq = np.frombuffer(s(), np.int8); anno = s(); ad = get("d")
        nodes.append((name.decode(), seqname.decode(), seq, anno.decode(), ad))
    ne = get("Q")
    edges = []
    for _ in range(ne):
        a, c, flag, ln, N = get("qq?dQ")
        assert N == 4 * L
        edges.append((a, c, flag, ln, b[o[0]:o[0] + 8 * N] if want_msgs else None)); o[0] += 8 * N
    root = get("q"); root_msg = b[o[0]:o[0] + 32 * L]; o[0] += 32 * L
    heights = [get("qd") for _ in range(n)]
    index = [get("Iq") for _ in range(get("I"))]
    tail = b[o[0]:]
    dg = None
    if dg_k:
        size = 1 + 4 + 8 + 8 * (dg_k + 1) + 8 * dg_k
        blk = tail[-size:]; tail = tail[:-size]
        assert blk[0] == 1 and struct.unpack_from("<i", blk, 1)[0] == dg_k
        dg = dict(alpha=struct.unpack_from("<d", blk, 5)[0], breaks=np.frombuffer(blk, np.float64, dg_k + 1, 13), rates=np.frombuffer(blk, np.float64, dg_k, 13 + 8 * (dg_k + 1)))
    else:
        assert tail[-1] == 0; tail = tail[:-1]
    return dict(ver=ver, n=n, L=L, nodes=nodes, edges=edges, root=root, root_msg=root_msg, heights=heights, index=index, model_text=tail.decode(), dg=dg)


def fasta_ids(path):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rt") as f:
        return [line[1:].split()[0] for line in f if line.startswith(">")]


def check_messages(got_up, got_down, oup, odown):
    """the bound of tests/test_gpu_parity.py::test_tree_pre_evaluation"""
    fin = np.isfinite(oup)
    assert (np.isfinite(got_up) == fin).all()
    assert np.abs(got_up[fin] - oup[fin]).max() < 1e-9 * max(1.0, np.abs(oup[fin]).max())
    assert np.isfinite(got_down[1:]).all() and np.abs(got_down[1:] - odown[1:]).max() < 1e-9 * max(1.0, np.abs(odown[1:]).max())


def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


def check_tree_of_file(ptu, t, fasta, dg_k=0):
    """children in Newick file order as hu_tree_info_children returns them, and the MSA index as (FASTA row, node) in ascending row"""
    ti = E.tree_info(ptu)
    assert [list(c) for c in ti["children"]] == [list(c) for c in t["children"]]
    raw = read_ptu(ptu, dg_k, want_msgs=False)
    ids = fasta_ids(fasta)
    leaves = [i for i, c in enumerate(t["children"]) if len(c) == 0]
    want = sorted((ids.index(t["names"][i]), i) for i in leaves)
    assert raw["index"] == want and [r for r, _ in raw["index"]] == sorted(r for r, _ in raw["index"])
    # every node's neighbour list: parent first, then the children in file order
    k = 0
    for u in range(raw["n"]):
        nb = ([int(t["parent"][u])] if u else []) + [int(c) for c in t["children"][u]]
        assert [(e[0], e[1]) for e in raw["edges"][k:k + len(nb)]] == [(u, v) for v in nb]
        k += len(nb)
    return ti, raw


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["JC69", "GTR"])
def test_70otus_end_to_end(tmp_path, model):
    need_gpu()
    r = run_build([FASTA70, TREE70, "--no-hmm", "-sm", sm(model), "-a", TAX70, "-n", "db70", "-v", "-f", "0.5"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["db70.ptu"]                  # no .hmm, .msa, .csfm
    for line in ("MSA database created for 125 X 1486 aligned sequences", "Phylogenetic Tree constructed with total 249 nodes", "Final Tree log-liklihood: ",
                 "-f belongs to the profile training and is ignored", "Evaluating Phylogenetic Tree at all other 248 nodes", "Phylogenetic Tree index saved"):
        assert line in r.stderr, (line, r.stderr)
    ptu = str(tmp_path / "db70.ptu")
    f = E.parse_files(None, ptu)
    db, oup, odown, oseq, oh = oracle70(model)
    assert (f["n_nodes"], f["L"], f["root"]) == (249, 1486, 0) and f["model"].type == db.model.type_id and f["model"].dg_k == 0
    assert np.array_equal(f["parent"], db.parent) and np.array_equal(f["blen"], db.blen)
    assert np.array_equal(f["seq"][db.is_leaf], db.seq[db.is_leaf]) and np.abs(f["height"] - db.height).max() < 1e-12
    check_messages(f["up"], f["down"], oup, odown)
    differ, cells = tie_cells(f["seq"], oseq, oup, ~db.is_leaf)
    print("70_otus %s: ancestral cells decided by exact-arithmetic ties: %d of %d" % (model, differ, cells))
    assert differ * 100 < cells
    t, is_leaf, blen = tree70()
    ti, raw = check_tree_of_file(ptu, t, FASTA70)
    rn, ra, rd = py_annotate(t["parent"], blen, t["names"], open(TAX70).read())
    assert ti["names"] == rn and ti["annos"] == ra and np.array_equal(ti["anno_dist"], rd)
    assert raw["model_text"] == db.model.name + "\n" + open(sm(model)).read()
    ll = float(r.stderr.split("Final Tree log-liklihood: ")[1].split()[0])
    pi = np.asarray(db.model.pi if model == "GTR" else [0.25] * 4)
    ref_ll = np.log((np.exp(oup[0]) * pi).sum(-1)).sum()
    assert abs(ll - ref_ll) <= 1e-5 * abs(ref_ll)                          # the line is printed with six significant digits


@pytest.mark.gpu
def test_var_k4_on_70otus_gtr(tmp_path):
    need_gpu()
    import torch
    from oracle import oracle_py as O
    r = run_build([FASTA70, TREE70, "--no-hmm", "-sm", sm("GTR"), "-a", TAX70, "-n", "dbv", "-V", "-k", "4", "-v"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Re-evaluating Phylogenetic Tree at all 249 nodes" in r.stderr and "Estimated alpha = 1.66" in r.stderr, r.stderr
    ptu = str(tmp_path / "dbv.ptu")
    db = oracle70("GTR")[0]
    n, L = db.seq.shape
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, None)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    alpha = E.dg_estimate_shape(E.tree_count_mutations(db.parent, L, up.data_ptr()))
    assert 1.6 < alpha < 1.72                                                 # a numpy count over the fixture's messages gives 1.6616
    raw = read_ptu(ptu, 4, want_msgs=False)
    assert raw["dg"]["alpha"] == alpha                                       # bit-equal
    b, rt = E.dg_model(4, alpha)
    assert np.array_equal(raw["dg"]["breaks"], b) and np.array_equal(raw["dg"]["rates"], rt)
    f = E.parse_files(None, ptu)
    assert f["model"].dg_k == 4 and list(f["model"].dg_rate)[:4] == list(rt)
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    oup, odown, oseq, oh = O.tree_evaluate(db.parent, db.blen, leaf_only, m, rt)
    check_messages(f["up"], f["down"], oup, odown)
    differ, cells = tie_cells(f["seq"], oseq, oup, ~db.is_leaf)
    assert differ * 100 < cells
    check_tree_of_file(ptu, tree70()[0], FASTA70, 4)


@pytest.mark.gpu
def test_var_on_invariant_columns_keeps_the_fixed_rate_model(tmp_path):
    need_gpu()
    rows = [(nm, "ACGTTGCA" * 12 + "--" + "GATTACA" * 6) for nm in ["A", "B", "C", "D-d", "E", "F"]]
    write_fasta(tmp_path / "same.fa", rows); (tmp_path / "hand.tre").write_text(HAND_JOIN)
    r = run_build(["same.fa", "hand.tre", "--no-hmm", "-sm", sm("GTR"), "-V"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert r.stderr.strip() == "Unable to estimate the shape parameter with near invariant rates, reducing to fixed rate model"
    assert sorted(os.listdir(tmp_path)) == ["hand.tre", "same.fa", "same.fa.ptu"]          # NAME defaults to the MSA file name
    raw = read_ptu(str(tmp_path / "same.fa.ptu"), 0, want_msgs=False)
    assert raw["dg"] is None and raw["L"] == 8 * 12 + 7 * 6
    assert E.parse_files(None, str(tmp_path / "same.fa.ptu"))["model"].dg_k == 0


@pytest.mark.gpu
def test_hand_tree_end_to_end(hand_inputs):
    need_gpu()
    from oracle import oracle_py as O
    tmp, fa, tr = hand_inputs
    r = run_build([fa, tr, "--no-hmm", "-sm", sm("GTR"), "-n", "hand", "-r", "other"], tmp)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    ptu = str(tmp / "hand.ptu")
    f = E.parse_files(None, ptu)
    rows = dict(hand_rows())
    first = dict(synth._IUPAC_FIRST)
    code = lambda s: np.array([first.get(c.upper(), -2 if c in "-._" else -1) for c in s], np.int8)
    t = E.newick_parse(HAND_JOIN)
    raw_rows = {i: code(rows[nm]) for i, nm in enumerate(t["names"]) if nm in rows}
    keep = (np.stack(list(raw_rows.values())) >= 0).any(0)
    assert 280 <= keep.sum() < 300 and not keep[[0, 1, 57, 58, 59, 120, 200, 299]].any() and keep[130]
    assert f["L"] == keep.sum() and f["n_nodes"] == 9 and np.array_equal(f["parent"], t["parent"])
    is_leaf = np.array([len(c) == 0 for c in t["children"]])
    for i, row in raw_rows.items():
        assert np.array_equal(f["seq"][i], row[keep]), i
    assert (np.stack(list(raw_rows.values())) >= -2).all()
    blen = t["blen"].copy(); blen[[2, 4, 5]] = 1e-5                           # F (missing), 'D-d' (-0.01), C (0)
    assert np.array_equal(f["blen"], blen)
    db = synth.make_db_70otus("GTR")
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    leaf_only = np.where(is_leaf[:, None], f["seq"], 0).astype(np.int8)
    oup, odown, oseq, oh = O.tree_evaluate(t["parent"], blen, leaf_only, m, None)
    check_messages(f["up"], f["down"], oup, odown)
    tie_cells(f["seq"], oseq, oup, ~is_leaf)
    assert np.abs(f["height"] - oh).max() < 1e-12
    ti, raw = check_tree_of_file(ptu, t, fa)
    rn, ra, rd = py_annotate(t["parent"], blen, t["names"], None, "other")
    assert ti["names"] == rn and ti["annos"] == ra and np.array_equal(ti["anno_dist"], rd) and ra[0] == "other" and ra[2] == "k__Bacteria"


# ----------------------------------------------------------------------------- the writer
def _edge_map(raw):
    return {(a, c): (flag, ln, msg) for a, c, flag, ln, msg in raw["edges"]}


def _file_order(parent):
    """file order (descending id, as a reference-built file has it) and MSA rows in another order than the nodes"""
    n = len(parent)
    children = [sorted(np.nonzero(parent == u)[0].tolist(), reverse=True) for u in range(n)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in children])]); idx = np.concatenate([np.asarray(c, np.int32) for c in children if c])
    leaves = [u for u in range(n) if not children[u]]
    rows = np.full(n, -1, np.int32); rows[leaves] = np.random.default_rng(2).permutation(len(leaves))
    return off, idx, rows, children, leaves


def _check_file_order(base, fo, parent, children, rows, leaves, dg_k):
    """fo differs from hu_ptu_write's file only in the order of the edge records and in the index block"""
    n = len(parent)
    A, B = read_ptu(base, dg_k), read_ptu(fo, dg_k)
    for key in ("ver", "n", "L", "root", "root_msg", "heights", "model_text"):
        assert A[key] == B[key], key
    assert all(a[:2] == b[:2] and np.array_equal(a[2], b[2]) and a[3:] == b[3:] for a, b in zip(A["nodes"], B["nodes"]))
    assert (A["dg"] is None) == (B["dg"] is None) and (A["dg"] is None or all(np.array_equal(A["dg"][k], B["dg"][k]) for k in A["dg"]))
    assert _edge_map(A) == _edge_map(B) and len(_edge_map(B)) == 2 * (n - 1)            # the same records ...
    order = [(u, v) for u in range(n) for v in ([int(parent[u])] if parent[u] >= 0 else []) + children[u]]
    assert [(e[0], e[1]) for e in B["edges"]] == order and [(e[0], e[1]) for e in A["edges"]] != order      # ... in another order
    assert B["index"] == sorted((int(rows[u]), u) for u in leaves) and A["index"] == list(enumerate(leaves))
    assert os.path.getsize(base) == os.path.getsize(fo)


def test_ptu_write_stream_host_messages(tmp_path):
    """host-resident messages take the plain loop and need no device: the same file as hu_ptu_write, and the child order and index block on request"""
    import filecmp
    db = get_db(60, 300, "GTR", dg_k=4)
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    kw = dict(names=db.names, annos=db.annos, anno_dist=db.anno_dist, model_text=db.model.text, dg_alpha=db.dg_alpha, dg_breaks=db.dg_b)
    base, same, fo, ref = (str(tmp_path / f) for f in ("plain.ptu", "stream.ptu", "fileorder.ptu", "synth.ptu"))
    args = (db.parent, db.blen, db.seq, db.up, db.down, db.height, md)
    E.write_ptu(base, *args, **kw); E.write_ptu_stream(same, *args, staging_bytes=12345, **kw)
    synth.write_ptu(db, ref)
    assert filecmp.cmp(base, same, shallow=False) and filecmp.cmp(base, ref, shallow=False)
    off, idx, rows, children, leaves = _file_order(db.parent)
    E.write_ptu_stream(fo, *args, child_off=off, child_idx=idx, msa_row_of_leaf=rows, **kw)
    _check_file_order(base, fo, db.parent, children, rows, leaves, 4)
    f = E.parse_files(None, fo)
    assert np.array_equal(f["up"], db.up) and np.array_equal(f["down"][1:], db.down[1:]) and np.array_equal(f["parent"], db.parent)
    for bad in (dict(child_off=off, child_idx=idx[::-1].copy()), dict(child_off=off[:-1].tolist() + [off[-1] - 1], child_idx=idx),
                dict(msa_row_of_leaf=np.zeros(len(db.parent), np.int32))):
        with pytest.raises(E.EngineError):
            E.write_ptu_stream(str(tmp_path / "bad.ptu"), *args, **dict(kw, **bad))
    assert not os.path.exists(tmp_path / "bad.ptu")


def _writer_case(tmp_path, parent, blen, leaf_only, md, kw, dg_k):
    import filecmp
    import torch
    n, L = leaf_only.shape
    up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    seq, h = E.tree_evaluate(parent, blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    base = str(tmp_path / "plain.ptu")
    E.write_ptu(base, parent, blen, seq, up.data_ptr(), down.data_ptr(), h, md, msgs_on_device=True, **kw)
    row = 32 * L
    for k, staging in enumerate((row, 3 * row, 2 * row + row // 2 + 1, 1, 0, 1 << 30)):       # one edge, three, an odd count between, below one, default, beyond the file
        p = str(tmp_path / ("s%d.ptu" % k))
        E.write_ptu_stream(p, parent, blen, seq, up.data_ptr(), down.data_ptr(), h, md, msgs_on_device=True, staging_bytes=staging, **kw)
        assert filecmp.cmp(base, p, shallow=False), staging
    hp = str(tmp_path / "host.ptu")                                             # host-resident messages: the plain loop
    E.write_ptu_stream(hp, parent, blen, seq, up.cpu().numpy(), down.cpu().numpy(), h, md, **kw)
    assert filecmp.cmp(base, hp, shallow=False)
    off, idx, rows, children, leaves = _file_order(parent)
    fo = str(tmp_path / "fileorder.ptu")
    E.write_ptu_stream(fo, parent, blen, seq, up.data_ptr(), down.data_ptr(), h, md, msgs_on_device=True, child_off=off, child_idx=idx, msa_row_of_leaf=rows,
                       staging_bytes=5 * row, **kw)
    _check_file_order(base, fo, parent, children, rows, leaves, dg_k)
    with pytest.raises(E.EngineError):                                                  # a child order that is no permutation of the children
        E.write_ptu_stream(str(tmp_path / "bad.ptu"), parent, blen, seq, up.data_ptr(), down.data_ptr(), h, md, msgs_on_device=True, child_off=off,
                           child_idx=idx[::-1].copy(), **kw)


@pytest.mark.gpu
def test_ptu_write_stream_against_ptu_write(tmp_path):
    need_gpu()
    db = get_db(60, 300, "GTR", dg_k=4)
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    kw = dict(names=db.names, annos=db.annos, anno_dist=db.anno_dist, model_text=db.model.text, dg_alpha=db.dg_alpha, dg_breaks=db.dg_b)
    _writer_case(tmp_path, db.parent, db.blen, leaf_only, md, kw, 4)


@pytest.mark.gpu
def test_ptu_write_stream_five_columns(tmp_path):
    need_gpu()
    db = get_db(60, 300, "GTR", dg_k=4)
    rng = np.random.default_rng(4)
    parent, blen = synth.make_tree(9, rng)[:2]
    n = len(parent)
    is_leaf = np.ones(n, bool); is_leaf[parent[parent >= 0]] = False
    leaf_only = np.where(is_leaf[:, None], rng.integers(-1, 4, (n, 5)), 0).astype(np.int8); leaf_only[leaf_only == -1] = -2
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, None)
    _writer_case(tmp_path, np.asarray(parent, np.int32), np.asarray(blen, np.float64), leaf_only, md, dict(model_text=db.model.text), 0)


# ----------------------------------------------------------------------------- the tree log-likelihood
def numpy_loglik(pi, v):
    """dot_product_scaled(pi, v) per column (src/PhyloTreeUnrooted.h:1505-1510)"""
    mx = v.max(-1)
    sc = np.where(np.isfinite(mx) & (mx < -510), -510 - mx, 0.0)
    with np.errstate(divide="ignore"):
        return np.log((np.exp(v + sc[:, None]) * pi).sum(-1)) - sc


@pytest.mark.gpu
def test_tree_loglik():
    need_gpu()
    import torch
    from oracle import oracle_py as O
    db = get_db(60, 300, "GTR", dg_k=4)
    n, L = db.seq.shape
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    per, tot = E.tree_loglik(n, L, 0, md, up.data_ptr())
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    oup = O.tree_evaluate(db.parent, db.blen, leaf_only, m, db.dg_r)[0]
    ref = numpy_loglik(np.asarray(db.model.pi), oup[0])
    assert np.all(np.abs(per - ref) <= 1e-9 * np.abs(ref)) and abs(tot - ref.sum()) <= 1e-9 * abs(ref.sum())
    s = 0.0
    for x in per:
        s += x
    assert tot == s                                                            # the serial sum
    # by hand: a column below -510 (exp underflows without the scaling), one at the threshold, an ordinary one, one with -inf entries;
    # read from node 1 of 2 so that the root offset is used
    v = np.array([[-800.0, -801.5, -805.0, -1200.0], [-510.0, -510.0, -511.0, -512.0], [-1.0, -2.0, -3.0, -4.0], [-np.inf, -900.0, -np.inf, -np.inf],
                  [-0.5, -np.inf, -np.inf, -np.inf]])
    buf = torch.zeros((2, 5, 4), dtype=torch.float64, device="cuda:0"); buf[1] = torch.from_numpy(v).to("cuda:0")
    torch.cuda.synchronize()
    per, tot = E.tree_loglik(2, 5, 1, md, buf.data_ptr())
    pi = np.asarray(db.model.pi)
    ref = numpy_loglik(pi, v)
    assert np.isfinite(ref).all() and ref[0] < -790 and ref[3] < -890
    assert np.all(np.abs(per - ref) <= 1e-9 * np.abs(ref)) and abs(tot - ref.sum()) <= 1e-9 * abs(ref.sum())
    exact = np.log(pi[0]) - 800 + np.log1p((pi[1] * np.exp(-1.5) + pi[2] * np.exp(-5.0) + pi[3] * np.exp(-400.0)) / pi[0])
    assert abs(per[0] - exact) <= 1e-9 * abs(exact)
    with pytest.raises(E.EngineError):
        E.tree_loglik(2, 5, 2, md, buf.data_ptr())


# ----------------------------------------------------------------------------- downstream: the built database under hmmufotu-amd and the engine
@pytest.mark.gpu
def test_built_database_downstream(tmp_path):
    need_gpu()
    from oracle import oracle_py as O, parity
    r = run_build([FASTA70, TREE70, "--no-hmm", "-sm", sm("JC69"), "-a", TAX70, "-n", "db"], tmp_path)
    assert r.returncode == 0, r.stderr
    db = synth.make_db_70otus()
    synth.write_hmm(db.hmm, str(tmp_path / "db.hmm"))
    rng = np.random.default_rng(9)
    reads = []
    leaves = np.nonzero(db.is_leaf)[0]
    while len(reads) < 64:                                                     # error-free 250-base slices of leaf rows
        u = int(rng.choice(leaves))
        s = "".join("ACGT"[c] for c in db.seq[u] if c >= 0)
        if len(s) >= 300:
            a = int(rng.integers(0, len(s) - 250)); reads.append(s[a:a + 250])
    with open(tmp_path / "reads.fq", "w") as f:
        for i, s in enumerate(reads):
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    c = subprocess.run([CLI, "db", "reads.fq", "-o", "out.tsv"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    lines = open(tmp_path / "out.tsv").read().strip().split("\n")
    assert len(lines) >= 1 + 60, len(lines)
    D = E.Database.load(str(tmp_path / "db.hmm"), str(tmp_path / "db.ptu"))
    ix = E.SeedIndex(db.parent, db.seq, db.hmm)
    vps = ix.lookup(reads)
    B = E.Batch(D, len(reads)); B.set_reads(reads, vps); B.assign(E.default_opts())
    recs = B.alignments(want_align=False)["recs"]; best = B.placements(); cand = B.candidates()
    m = O.Model(db.model.type_id, db.model.pi, db.model.par)
    H = O.Hmm(db.hmm.K, db.hmm.L, db.hmm.EM, db.hmm.EI, db.hmm.T, db.hmm.p2cs, 0)
    T = O.Tree(db.parent, db.blen, db.seq, db.up, db.down, db.height, m, None, db.anno_id)
    res = O.pipeline_batch(H, T, reads, vps, opts=O.default_opts(tieMode=1), threads=4, want_cands=True)
    assert (recs["status"] == res["aln_ints"][:, 7]).all() and (recs["status"] == E.READ_OK).all() and np.array_equal(recs["cost"], res["cost"])
    assert (best["n_cand"] == res["n_cand"]).all()
    per = []
    for i in range(len(reads)):
        k = int(res["n_cand"][i]); a, b = int(cand["offs"][i]), int(cand["offs"][i + 1])
        per.append(parity.classify_read(res["cand_node"][i, :k], res["cand_est"][i, :k], res["cand_ratio0"][i, :k], cand["c_node"][a:b], db.parent,
                                        pos=int(res["best_pos"][i])))
    tot = parity.summarize(per)
    print("built 70_otus database, 64 reads:", tot)
    assert tot["set_differs"] == 0 and tot["swaps_unexplained"] == 0 and tot["best_unexplained"] == 0, tot
    B.close(); D.close()
