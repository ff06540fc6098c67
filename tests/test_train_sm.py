"""hmmufotu-amd-train-sm: MSA + tree -> a substitution model file (src/hmmufotu-train-sm.cpp:77-243).

Every check is a Python restatement written here from the reference's description: which rows are compared
(src/PhyloTreeUnrooted.cpp:449-494 with the node predicates of src/PhyloTreeUnrooted.h:199-267 and libc's rand() through ctypes),
the per-column counts (src/DNASubModel.cpp:52-112, src/SeqUtils.cpp:37-54) in numpy, and the trainers of the six models.

CPU part: the program's refusals, the training sets of 70_otus and of a hand tree, the trainers over hand-made matrices, the text.
GPU part: hu_sm_counts against numpy at every row length where the kernel's piece loop changes shape, the program on 70_otus for all
types and both methods, on a 1,399-node synthetic tree, and the chain train -> hmmufotu-amd-build --no-hmm -sm.

Recorded on 70_otus (249 nodes, 125 rows): 33 Gojobori candidates of which 2 pass the distance test, 34 Goldman items."""
import ctypes as C
import ctypes.util
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest

from hmmufotu_amd import engine as E, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-train-sm")
BUILD = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-build")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70, TREE70 = os.path.join(REF, "70_otus.fasta.gz"), os.path.join(REF, "70_otus.tree")
TYPES = ["GTR", "TN93", "HKY85", "F81", "K80", "JC69"]
N_PAR = {"GTR": 16, "TN93": 3, "HKY85": 2, "F81": 1, "K80": 1, "JC69": 0}
MAX_PDIST = 0.15
#   root: four children (multifurcating).  X: both children are tips, T2 has three children.  Y: T3 is a one-child tip and the outer
#   child f is itself a leaf.  Z: the outer child W is two levels above its leaves, so randomLeaf draws twice.
HAND = "(((a,b)T1,(c,d,e)T2)X,((g)T3,f)Y,L0,((m,n)T4,((h,i)U,(j,k)V)W)Z);"
libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")


# ----------------------------------------------------------------------------- the restatement
def py_training_set(t, row_of, method):
    """the items of getModelTraningSetGojobori / Goldman; draws from libc's rand() exactly where randomLeaf does"""
    parent, children = t["parent"], [[int(c) for c in ch] for ch in t["children"]]
    n_nb = lambda u: len(children[u]) + (1 if parent[u] >= 0 else 0)
    is_leaf = lambda u: n_nb(u) == 1
    is_tip = lambda u: (not is_leaf(u)) and all(is_leaf(c) for c in children[u])
    items = []
    for u in range(len(parent)):
        ch = children[u]
        if method.lower() == "gojobori":
            if len(ch) == 2 and (is_tip(ch[0]) or is_tip(ch[1])):
                tip, outer = ch
                if not is_tip(tip):
                    tip, outer = outer, tip
                node = outer
                while not is_leaf(node):
                    node = children[node][libc.rand() % len(children[node])]
                items.append((row_of[node], row_of[children[tip][0]], row_of[children[tip][-1]]))
        else:
            if is_tip(u) and n_nb(u) > 2:
                items.append((-1, row_of[ch[0]], row_of[ch[-1]]))
    return np.array(items, np.int32).reshape(-1, 3)


def py_dn(a, b):
    both = (a >= 0) & (b >= 0)
    return int((both & (a != b)).sum()), int(both.sum())


def py_counts(rows, items):
    """counts [k][4][4], dn [k][4], base [n][4] as hu_sm_counts defines them"""
    k = len(items)
    counts, dn = np.zeros((k, 4, 4), np.int32), np.zeros((k, 4), np.int32)
    for i, (r0, r1, r2) in enumerate(items):
        b1, b2 = rows[r1].astype(int), rows[r2].astype(int)
        if r0 < 0:      # calcTransFreq2Seq; the distances are those of (row1, row1) and (row1, row2)
            ok = (b1 >= 0) & (b2 >= 0)
            np.add.at(counts[i], (b1[ok], b2[ok]), 1)
            dn[i] = py_dn(b1, b1) + py_dn(b1, b2)
        else:           # calcTransFreq3Seq
            b0 = rows[r0].astype(int)
            anc = np.where((b0 == b1) | (b0 == b2), b0, np.where(b1 == b2, b1, -1))
            ok = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (anc >= 0)
            for b in (b0, b1, b2):
                np.add.at(counts[i], (anc[ok], b[ok]), 1)
            dn[i] = py_dn(b0, b1) + py_dn(b0, b2)
    base = np.stack([(rows == b).sum(1) for b in range(4)], 1).astype(np.int32)
    return counts, dn, base


def py_pass(items, dn):
    with np.errstate(divide="ignore", invalid="ignore"):
        p1, p2 = dn[:, 0] / dn[:, 1].astype(float), dn[:, 2] / dn[:, 3].astype(float)
    return np.where(items[:, 0] < 0, p1 <= MAX_PDIST, (p1 <= MAX_PDIST) & (p2 <= MAX_PDIST))       # a NaN fails


def py_train(typ, mats, f):
    """(pi, par) of trainParams over the matrices of the reference's vector (those that passed); None where it would print NaN"""
    A, Cc, G, T = 0, 1, 2, 3
    f = np.asarray(f, float)
    pi = f / f.sum() if typ in ("GTR", "TN93", "HKY85", "F81") else np.full(4, 0.25)
    mats = [np.asarray(m, float) for m in mats]
    if typ == "GTR":
        Q, n = np.zeros((4, 4)), 0
        for P in mats:
            P = (P + P.T) / 2.0
            Z = P.sum(1)
            Qv = np.zeros((4, 4))
            with np.errstate(divide="ignore", invalid="ignore"):
                for i in range(4):
                    for j in range(4):
                        if i != j:
                            Qv[i, j] = P[i, j] / Z[i]
                            Qv[i, i] -= Qv[i, j]
            off = Qv[~np.eye(4, dtype=bool)]
            if (Qv == 0).all() or not (off >= 0).all():
                continue
            n += 1
            Q += Qv / -np.trace(Qv)
        if n == 0:
            return None
        Q /= n
        R = Q / pi[None, :]
        np.fill_diagonal(R, 0.0)
        R = (R + R.T) / 2.0
        return pi, list(R.ravel())
    Tr = sum(P[A, G] + P[G, A] for P in mats)
    Ty = sum(P[Cc, T] + P[T, Cc] for P in mats)
    Tv = sum(P[A, Cc] + P[A, T] + P[Cc, A] + P[Cc, G] + P[G, Cc] + P[G, T] + P[T, A] + P[T, G] for P in mats)
    if typ in ("TN93", "HKY85", "K80") and Tv == 0:
        return None
    if typ == "TN93":
        kr, ky = Tr / Tv, Ty / Tv
        beta = 1 / (2 * (pi[A] * pi[Cc] + pi[A] * pi[T] + pi[Cc] * pi[G] + pi[G] * pi[T] + kr * (pi[A] * pi[G]) + ky * (pi[Cc] * pi[T])))
        return pi, [kr, ky, beta]
    if typ == "HKY85":
        kappa = (Tr + Ty) / Tv
        return pi, [kappa, 1 / (2 * (pi[A] + pi[G]) * (pi[Cc] + pi[T]) + 2 * kappa * (pi[A] * pi[G] + pi[Cc] * pi[T]))]
    if typ == "K80":
        return pi, [(Tr + Ty) / Tv]
    if typ == "F81":
        return pi, [1 / (1 - (pi ** 2).sum())]
    return pi, []


def close(got, want, rel=1e-13):
    got, want = np.asarray(got, float), np.asarray(want, float)
    return got.shape == want.shape and bool((np.abs(got - want) <= rel * np.abs(want)).all())


def check_model(md, typ, want):
    pi, par = want
    assert md.type == TYPES.index(typ) and md.dg_k == 0
    assert close(list(md.pi), pi), (list(md.pi), pi)
    assert close(list(md.par)[:N_PAR[typ]], par), (list(md.par), par)


def parse_text(typ, text):
    """hu_model_parse_text the way hmmufotu-amd-build hands it a model file: the type word, then the file"""
    md = E.ModelDesc()
    b = (typ + "\n" + text).encode()
    assert E.load_library().hu_model_parse_text(b, C.c_int64(len(b)), C.byref(md)) == 0
    return md


# ----------------------------------------------------------------------------- inputs
def read_fasta(path):
    op = gzip.open if str(path).endswith(".gz") else open
    names, seqs = [], []
    with op(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0]); seqs.append([])
            else:
                seqs[-1].append(line.strip())
    return names, ["".join(s) for s in seqs]


def encode_rows(seqs):
    """the pruned, encoded alignment: the codes of hu_msa_encode_table, the columns without a residue dropped"""
    a = np.frombuffer("".join(seqs).encode(), np.uint8).reshape(len(seqs), -1)
    rows = E.msa_encode_table()[a]
    return np.ascontiguousarray(rows[:, (rows >= 0).any(0)])


def row_of_leaves(t, names):
    at = {nm: i for i, nm in enumerate(names)}
    return np.array([at[t["names"][i]] if len(ch) == 0 else -1 for i, ch in enumerate(t["children"])], np.int32)


@functools.lru_cache(None)
def otus70():
    names, seqs = read_fasta(FASTA70)
    t = E.newick_parse(open(TREE70).read())
    return t, row_of_leaves(t, names), encode_rows(seqs)


def py_model(t, row_of, rows, typ, method):
    """the whole restatement for one input, from an unseeded rand(): (pi, par) or None, candidates, passed"""
    libc.srand(1)                                  # the state of a process that never called srand
    items = py_training_set(t, row_of, method)
    counts, dn, base = py_counts(rows, items)
    ok = py_pass(items, dn)
    f = base[row_of[row_of >= 0]].sum(0)
    return py_train(typ, [counts[i] for i in np.nonzero(ok)[0]], f), len(items), int(ok.sum())


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for nm, s in zip(names, seqs):
            f.write(">%s made up\n" % nm)
            for a in range(0, len(s), 60):
                f.write(s[a:a + 60] + "\n")


def run(args, cwd, binary=BIN):
    return subprocess.run([binary] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=120)


def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ============================================================================= CPU
def test_program_is_built():
    assert os.path.exists(BIN), "hmmufotu-amd-train-sm missing: run __graft_entry__.build()"


def test_refusals(tmp_path):
    t = E.newick_parse(HAND)
    leaves = [t["names"][i] for i, ch in enumerate(t["children"]) if len(ch) == 0]
    rng = np.random.default_rng(2)
    seqs = ["".join(rng.choice(list("ACGT-"), 90)) for _ in leaves]
    fa, tr = tmp_path / "hand.fasta", tmp_path / "hand.tree"
    write_fasta(fa, leaves, seqs); tr.write_text(HAND + "\n")

    def refused(args, *words):
        r = run(args, tmp_path)
        lines = [x for x in r.stderr.strip().split("\n") if x]
        assert r.returncode != 0 and r.stdout == "" and len(lines) == 1 and all(w in lines[0] for w in words), (r.returncode, r.stderr)
        assert "device" not in r.stderr            # refused before a device is asked for: this test runs without one

    nwk = tmp_path / "hand.nwk"; nwk.write_text(HAND)
    refused([fa, nwk], "Unrecognized TREE-FILE format, must be in Newick format")
    refused([fa, tr, "--fmt", "msa"], "'msa'", "not read here")
    msa = tmp_path / "hand.msa"; msa.write_bytes(b"HmmUFOtu")
    refused([msa, tr], "'msa'", "not read here")                                   # the format guessed from the name
    refused([fa, tr, "--fmt", "fastq"], "Unsupported sequence format 'fastq'")
    refused([fa, tr, "-s", "GTR2"], "Unknown DNA substitution model type 'GTR2'")
    refused([fa, tr, "--sub-model", "gtr"], "Unknown DNA substitution model type 'gtr'")    # the type is case-sensitive, the method is not
    refused([fa, tr, "-m", "Felsenstein"], "Unknown DNA substitution model training method 'Felsenstein'")
    f2 = tmp_path / "short.fasta"; write_fasta(f2, leaves[:-1], seqs[:-1])
    refused([f2, tr, "-m", "GOLDMAN"], "Unmatched MSA and Tree. Found %d leaf sequences from MSA but expecting %d leaves in the Phylogenetic Tree" % (len(leaves) - 1, len(leaves)))
    assert not os.path.exists(tmp_path / "out.sm")


def test_hand_tree_has_the_cases_it_is_for():
    t = E.newick_parse(HAND)
    ch = {t["names"][i]: [t["names"][c] for c in c_] for i, c_ in enumerate(t["children"])}
    assert len(ch[""]) == 4 and ch["T3"] == ["g"] and len(ch["T2"]) == 3 and ch["X"] == ["T1", "T2"] and ch["Y"] == ["T3", "f"] and ch["f"] == []


@pytest.mark.parametrize("method", ["Gojobori", "Goldman", "gOLDMAN"])
def test_training_set_of_the_hand_tree(method):
    t = E.newick_parse(HAND)
    n = len(t["parent"])
    leaf = np.array([len(c) == 0 for c in t["children"]])
    row_of = np.full(n, -1, np.int32)
    row_of[leaf] = np.random.default_rng(4).permutation(int(leaf.sum()))
    for seed in (1, 7, 12345):                     # other draws reach other leaves below W and T2
        libc.srand(seed); got = E.sm_training_set(t["parent"], t["child_off"], t["child_idx"], row_of, method)
        libc.srand(seed); want = py_training_set(t, row_of, method)
        assert np.array_equal(got, want), (got, want)
    at = {nm: row_of[i] for i, nm in enumerate(t["names"])}
    if method == "Gojobori":
        assert len(got) == 4                                                       # X, Y, Z, W in some id order; not the root
        assert any(tuple(it) == (at["f"], at["g"], at["g"]) for it in got)        # Y: a leaf as outer, the one-child tip's child twice
        assert any(tuple(it[1:]) == (at["a"], at["b"]) and it[0] in (at["c"], at["d"], at["e"]) for it in got)     # X: both tips, the first one taken
    else:
        assert sorted(map(tuple, got)) == sorted((-1, at[x], at[y]) for x, y in [("a", "b"), ("c", "e"), ("m", "n"), ("h", "i"), ("j", "k")])     # not T3


def test_training_set_of_70otus():
    t, row_of, rows = otus70()
    assert rows.shape == (125, 1486) and len(t["parent"]) == 249
    libc.srand(1); goj = E.sm_training_set(t["parent"], t["child_off"], t["child_idx"], row_of, "Gojobori")
    libc.srand(1); want = py_training_set(t, row_of, "Gojobori")
    assert np.array_equal(goj, want) and len(goj) == 33
    ok = py_pass(want, py_counts(rows, want)[1])
    assert int(ok.sum()) == 2
    gold = E.sm_training_set(t["parent"], t["child_off"], t["child_idx"], row_of, "Goldman")
    assert np.array_equal(gold, py_training_set(t, row_of, "Goldman")) and len(gold) == 34 and (gold[:, 0] == -1).all()
    # hu_sm_item_pass on the restated distances, a NaN among them
    dn = np.array([[0, 10, 3, 20], [2, 10, 3, 20], [0, 0, 0, 5], [0, 0, 9, 9], [3, 20, 0, 0], [15, 100, 15, 100]], np.int32)
    items = np.array([[5, 1, 2], [5, 1, 2], [5, 1, 2], [-1, 1, 2], [-1, 1, 2], [0, 1, 2]], np.int32)
    assert list(E.sm_item_pass(items, dn)) == [True, False, False, False, True, True] == list(py_pass(items, dn))
    with pytest.raises(E.EngineError):
        E.sm_training_set(t["parent"], t["child_off"], t["child_idx"], np.full(249, -1, np.int32), "Goldman")      # leaves without rows


def hand_matrices():
    """(matrices, passed): ordinary count matrices, an all-zero one, one with a zero row, one the distances fail"""
    rng = np.random.default_rng(8)
    mats = []
    for _ in range(5):
        m = rng.integers(0, 12, (4, 4)).astype(float)
        m[np.arange(4), np.arange(4)] += rng.integers(200, 400, 4)
        mats.append(m)
    mats.append(np.zeros((4, 4)))
    z = mats[0].copy(); z[2, :] = 0; z[:, 2] = 0                                    # symmetrised, row G stays zero
    mats.append(z)
    mats.append(mats[1] * 3 + 1)                                                    # would change every sum if it were used
    passed = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    return np.array(mats), passed


@pytest.mark.parametrize("typ", TYPES)
def test_trainers_against_the_restatement(typ):
    mats, passed = hand_matrices()
    f = [1234, 987, 1500, 1011]
    md, used = E.sm_train(typ, mats, passed, f, info=True)
    check_model(md, typ, py_train(typ, mats[passed], f))
    assert used == (5 if typ == "GTR" else 7)                                       # GTR drops the all-zero matrix and the one with a zero row
    md2 = E.sm_train(typ, mats[:5], np.ones(5, bool), f)
    if typ == "GTR":
        assert list(md2.par) == list(md.par)                                        # the dropped ones add nothing
    if typ in ("K80", "JC69"):
        assert list(md.pi) == [0.25] * 4
    # the text: parses back to exactly what was written
    text = E.sm_write_text(md)
    assert text.startswith("# DNA Substitution Model\nType: %s\n" % typ) and text.endswith("\n")
    back = parse_text(typ, text)
    assert back.type == md.type and list(back.pi) == list(md.pi) and list(back.par)[:N_PAR[typ]] == list(md.par)[:N_PAR[typ]]
    if typ == "GTR":
        q = np.array([[float(x) for x in line.split()] for line in text.split("Q:\n")[1].strip().split("\n")])
        assert q.shape == (4, 4) and np.abs(q.sum(1)).max() <= 1e-15 and abs(np.trace(q) + 1) <= 1e-15
        assert abs((np.array(md.pi) * np.diag(q)).sum() + 1) > 1e-3                 # scaled by the trace, not by the pi-weighted rate
        assert text.count("\n") == 2 + 1 + 5 + 5


@pytest.mark.parametrize("typ", TYPES)
def test_empty_training_sets_are_refused(typ):
    mats, passed = hand_matrices()
    f = [10, 20, 30, 40]
    none = np.zeros(len(mats), bool)
    diag = np.array([np.diag([5.0, 6, 7, 8])] * 2)                                  # no change observed at all
    ti_only = np.array([[[9.0, 0, 2, 0], [0, 9, 0, 3], [2, 0, 9, 0], [0, 3, 0, 9]]])     # transitions, no transversion
    if typ == "GTR":
        for m, p in ((mats, none), (mats[5:7], np.ones(2, bool)), (diag, np.ones(2, bool)), (np.zeros((0, 4, 4)), np.zeros(0, bool))):
            with pytest.raises(E.EngineError, match="valid rate matrix"):
                E.sm_train(typ, m, p, f)
            assert py_train(typ, [x for x, k in zip(m, p) if k], f) is None
        check_model(E.sm_train(typ, ti_only, [True], f), typ, py_train(typ, ti_only, f))
    elif typ in ("TN93", "HKY85", "K80"):
        for m, p in ((mats, none), (diag, np.ones(2, bool)), (ti_only, np.ones(1, bool))):
            with pytest.raises(E.EngineError, match="Tv == 0"):
                E.sm_train(typ, m, p, f)
            assert py_train(typ, [x for x, k in zip(m, p) if k], f) is None
    else:
        check_model(E.sm_train(typ, mats, none, f), typ, py_train(typ, [], f))       # F81 and JC69 use no matrix
    if typ in ("GTR", "TN93", "HKY85", "F81"):
        with pytest.raises(E.EngineError, match="no residue"):
            E.sm_train(typ, mats, passed, [0, 0, 0, 0])


# ============================================================================= GPU
def count_rows(n_rows, L, rng):
    """rows with gaps and invalid codes, an all-gap row (1), two identical rows (2, 3), and with 0, 4, 5 all different on the first half"""
    rows = rng.integers(0, 4, (n_rows, L)).astype(np.int8)
    rows[rng.random((n_rows, L)) < 0.15] = -2
    rows[rng.random((n_rows, L)) < 0.05] = -1
    rows[1] = -2
    rows[3] = rows[2]
    k = (L + 1) // 2
    rows[0, :k], rows[4, :k], rows[5, :k] = 0, 1, 2
    rows[6] = np.where(rng.random(L) < 0.1, rng.integers(0, 4, L), rows[7]).astype(np.int8)      # a close pair
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 15, 16, 17, 255, 256, 257, 4097])
def test_sm_counts_against_numpy(L):
    need_gpu()
    rng = np.random.default_rng(100 + L)
    rows = count_rows(12, L, rng)
    one = np.array([[0, 4, 5]], np.int32)
    items = np.concatenate([one, [[2, 3, 2], [1, 0, 4], [0, 1, 1], [-1, 1, 2], [-1, 6, 7], [-1, 3, 3], [7, 6, 6]],
                            rng.integers(0, 12, (292, 3))]).astype(np.int32)
    items[8::3, 0] = -1                                                             # pairs among the triples
    assert len(items) == 300 and (items[:, 0] == -1).sum() > 90
    for its in (one, items):
        got = E.sm_counts(rows, its)
        counts, dn, base = py_counts(rows, its)
        assert np.array_equal(got["counts"], counts) and np.array_equal(got["dn"], dn) and np.array_equal(got["base"], base)
        assert np.array_equal(got["pass"], py_pass(its, dn))
    assert (dn[2] == 0).all() and not got["pass"][2]                                # N == 0 fails
    assert np.array_equal(got["counts"][0], py_counts(rows[:, (L + 1) // 2:], one)[0][0])     # where all three differ nothing is counted
    if L >= 255:
        assert counts[1].sum() > 0 and got["pass"].any() and not got["pass"].all()
    # one row, one pair of the row with itself
    solo = E.sm_counts(rows[:1], [[-1, 0, 0]])
    c1, d1, b1 = py_counts(rows[:1], np.array([[-1, 0, 0]], np.int32))
    assert np.array_equal(solo["counts"], c1) and np.array_equal(solo["dn"], d1) and np.array_equal(solo["base"], b1)
    assert solo["counts"][0].sum() == np.trace(solo["counts"][0]) == (rows[0] >= 0).sum()
    none = E.sm_counts(rows, np.zeros((0, 3), np.int32))                            # base counts alone
    assert np.array_equal(none["base"], base) and none["counts"].shape == (0, 4, 4)
    with pytest.raises(E.EngineError, match="rows"):
        E.sm_counts(rows, [[0, 12, 1]])
    with pytest.raises(E.EngineError, match="rows"):
        E.sm_counts(rows, [[-2, 0, 1]])


@pytest.mark.gpu
@pytest.mark.parametrize("method,candidates,passed", [("Gojobori", 33, 2), ("goldman", 34, 34)])
@pytest.mark.parametrize("typ", TYPES)
def test_program_on_70otus(tmp_path, typ, method, candidates, passed):
    need_gpu()
    r = run([FASTA70, TREE70, "-s", typ, "-m", method, "-v"], tmp_path)
    assert r.returncode == 0, r.stderr
    t, row_of, rows = otus70()
    want, n_items, n_ok = py_model(t, row_of, rows, typ, method)
    assert (n_items, n_ok) == (candidates, passed)
    for line in ("MSA loaded", "MSA pruned", "MSA database created for 125 X 1486 aligned sequences", "Newick Tree read",
                 "Phylogenetic Tree constructed with total 249 nodes", "MSA loaded into Phylogenetic Tree",
                 "Training set (%s): %d candidates, %d within p-distance 0.15" % (method.capitalize(), candidates, passed),
                 "DNA Substitution Model trained", "Model written"):
        assert line in r.stderr.split("\n"), (line, r.stderr)
    check_model(parse_text(typ, r.stdout), typ, want)
    quiet = run([FASTA70, TREE70, "--sub-model", typ, "--method", method, "-o", "m.sm"], tmp_path)
    assert quiet.returncode == 0 and quiet.stderr == "" and quiet.stdout == "" and (tmp_path / "m.sm").read_text() == r.stdout


@functools.lru_cache(None)
def synth_inputs():
    """the 1,399-node tree of tests/test_build.py (seed 21), sequences evolved along a quarter of its branch lengths so that most
    sibling leaves lie within 0.15 of each other; sparse gaps; as (names, sequences, Newick)"""
    rng = np.random.default_rng(21)
    parent, blen, is_leaf = synth.make_tree(700, rng, 0.05)
    seq = synth.evolve_sequences(parent, blen * 0.25, 300, synth.load_model("GTR"), np.ones(300), rng)
    seq[rng.random(seq.shape) < 0.03] = -2
    kids = [[] for _ in parent]
    for u in range(1, len(parent)):
        kids[parent[u]].append(u)
    text = {}
    for u in range(len(parent) - 1, -1, -1):            # preorder numbering: children after their parent
        text[u] = ("n%d" % u if is_leaf[u] else "(" + ",".join(text.pop(c) for c in kids[u]) + ")") + (":%.6f" % blen[u] if u else "")
    leaves = np.nonzero(is_leaf)[0]
    order = rng.permutation(leaves)                     # MSA rows in another order than the tree's leaves
    return ["n%d" % u for u in order], ["".join("ACGT-"[c] for c in seq[u]) for u in order], text[0] + ";"


@pytest.mark.gpu
@pytest.mark.parametrize("typ", ["GTR", "TN93"])
def test_program_on_a_synthetic_tree(tmp_path, typ):
    need_gpu()
    names, seqs, nwk = synth_inputs()
    write_fasta(tmp_path / "syn.fa", names, seqs); (tmp_path / "syn.tre").write_text(nwk + "\n")
    r = run(["syn.fa", "syn.tre", "-s", typ, "-v"], tmp_path)
    assert r.returncode == 0, r.stderr
    t = E.newick_parse(nwk)
    assert len(t["parent"]) == 1399
    want, n_items, n_ok = py_model(t, row_of_leaves(t, names), encode_rows(seqs), typ, "Gojobori")
    assert n_ok >= 200, (n_items, n_ok)                                             # hundreds of matrices
    assert "Training set (Gojobori): %d candidates, %d within p-distance 0.15" % (n_items, n_ok) in r.stderr
    check_model(parse_text(typ, r.stdout), typ, want)


@pytest.mark.gpu
def test_trained_model_builds_a_database(tmp_path):
    need_gpu()
    r = run([FASTA70, TREE70, "-o", "own.sm"], tmp_path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    text = (tmp_path / "own.sm").read_text()
    md = parse_text("GTR", text)
    b = run([FASTA70, TREE70, "--no-hmm", "-sm", "own.sm", "-n", "own"], tmp_path, BUILD)
    assert b.returncode == 0, b.stderr
    f = E.parse_files(None, str(tmp_path / "own.ptu"))
    assert f["model"].type == 0 and list(f["model"].pi) == list(md.pi) and list(f["model"].par) == list(md.par)
    assert abs(sum(md.pi) - 1) < 1e-15 and np.allclose(np.array(md.par).reshape(4, 4), np.array(md.par).reshape(4, 4).T, rtol=0, atol=0)
