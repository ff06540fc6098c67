"""Writing the reference's seed index file, <DB>.csfm: hu_suffix_array (device), hu_csfm_encode (host, from a given
suffix array), hu_csfm_write (device + host), hmmufotu-amd-build --csfm, and the reader's handling of the 20-byte head.

Expected bytes come from oracle/_ref/csfm_ref — the reference's own libcds and libdivsufsort — for the 70_otus alignment
(tests/golden/70_otus.csfm.gz) and four small alignments (tests/golden/csfm_write_{a,b,c,d}.*, made by make_csfm_write_golden.py):
  a  7 rows x 42 columns, no T anywhere (a padding symbol in the wavelet tree), three identical rows back to back, an all-gap row (two
     adjacent separators), a row with an inner gap run, lower case and N          b  one row, ACGT-ACGTTTGA (concatLen 13)
  c  40 identical random rows of 300 bases (N = 12,041)                             d  three rows of one column: A, -, C (N = 6)
  70otus_pruned  the 70_otus alignment without its all-gap columns (MSA::prune: 1,486 of 7,682), as hmmufotu-amd-build --csfm indexes it
csfm_ref writes no saveProgInfo head and takes csSeq from UNWEIGHTED counts: the library tests pass that csSeq, computed here with numpy,
and compare file[20:]; the program test compares csSeq with a numpy restatement over msa_stats' weighted counts and every other byte with
csfm_ref's.  Every comparison is byte equality.  The suffix arrays the host tests feed the encoder are numpy prefix doubling over
np.lexsort, itself checked against sorted() over the byte suffixes."""
import functools
import gzip
import os
import subprocess
import ctypes as C

import numpy as np
import pytest

from conftest import get_db
from hmmufotu_amd import engine as E, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(G, "ref_data")
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-build")
CLI = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd")
CASES = ["70_otus", "a", "b", "c", "d", "70otus_pruned"]
HEAD = 20                                    # saveProgInfo: "HmmUFOtu" + three int32
CS_AT = HEAD + 8 + 3 + 1 + 2 + 4 + 1024      # the csSeq string: size_t length, then the blank and the csLen characters


def read_fasta(path):
    rows = []
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        for l in f:
            l = l.strip()
            if l.startswith(">"):
                rows.append("")
            elif rows:
                rows[-1] += l
    return rows


@functools.lru_cache(None)
def case(name):
    """(rows as a uint8 [n][L] array, golden bytes of csfm_ref)"""
    if name == "70otus_pruned":
        a = case("70_otus")[0]
        return np.ascontiguousarray(a[:, (codes(a) >= 0).any(0)]), gzip.open(os.path.join(G, "csfm_write_70otus_pruned.csfm.gz"), "rb").read()
    if name == "70_otus":
        rows, gold = read_fasta(os.path.join(REF, "70_otus.fasta.gz")), os.path.join(G, "70_otus.csfm.gz")
    else:
        rows, gold = read_fasta(os.path.join(G, "csfm_write_%s.fa" % name)), os.path.join(G, "csfm_write_%s.csfm.gz" % name)
    a = np.frombuffer("".join(rows).encode(), np.uint8).reshape(len(rows), len(rows[0]))
    return a, gzip.open(gold, "rb").read()


def codes(a):
    return E.msa_encode_table()[a]


def text_of(a):
    """buildConcatSeq: residues as code + 1, a 0 behind every row, one more 0 at the end"""
    e = codes(a)
    assert (e != -1).all()
    parts = []
    for r in e:
        parts += [(r[r >= 0] + 1).astype(np.uint8), np.zeros(1, np.uint8)]
    return np.concatenate(parts + [np.zeros(1, np.uint8)])


def np_suffix_array(t):
    """prefix doubling with np.lexsort; a suffix that ends inside the compared window sorts first (second key 0)"""
    t = np.asarray(t)
    n = len(t)
    rank, h = t.astype(np.int64) + 1, 1
    while True:
        nxt = np.zeros(n, np.int64)
        if h < n:
            nxt[:n - h] = rank[h:]
        order = np.lexsort((nxt, rank))
        head = np.ones(n, bool)
        head[1:] = (rank[order][1:] != rank[order][:-1]) | (nxt[order][1:] != nxt[order][:-1])
        dense = np.cumsum(head)
        rank = np.empty(n, np.int64); rank[order] = dense
        if dense[-1] == n:
            return order.astype(np.int32)
        h *= 2


@functools.lru_cache(None)
def case_sa(name):
    t = text_of(case(name)[0])
    return t, np_suffix_array(t)


def unweighted_cs(a):
    """csfm_ref's csSeq and csIdentity: the first maximum of the raw residue counts when it is >= the raw gap count, else '-'"""
    e = codes(a)
    cnt = np.stack([(e == b).sum(0) for b in range(4)])
    gap = (e < 0).sum(0)
    cs = "".join("ACGT"[int(c.argmax())] if c.max() >= g else "-" for c, g in zip(cnt.T, gap))
    return cs, cnt.max(0) / a.shape[0]


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_numpy_suffix_array_against_sorted(name):
    t, sa = case_sa(name)
    raw = bytes(t)
    assert sa.tolist() == sorted(range(len(raw)), key=lambda i: raw[i:])         # bytes compare like the suffixes: a proper prefix first


def test_case_shapes():
    assert [len(case_sa(k)[0]) for k in ("b", "c", "d")] == [14, 12041, 6]
    a = case("a")[0]
    t = text_of(a)
    assert a.shape == (7, 42) and 4 not in t and (a[0] == a[1]).all() and (a[1] == a[2]).all() and (codes(a)[3] == -2).all()
    assert bytes([0, 0]) in bytes(t[:-1]) and (a >= 97).any() and (a == ord("N")).any()
    assert case("70_otus")[0].shape == (125, 7682) and case("70otus_pruned")[0].shape == (125, 1486)
    assert np.array_equal(case_sa("70_otus")[0], case_sa("70otus_pruned")[0])          # pruning drops no residue: one text, another concat2CS


@functools.lru_cache(None)
def ptu_head():
    import tempfile
    db = get_db(60, 300, "GTR", dg_k=4)
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    with tempfile.TemporaryDirectory() as t:
        p = os.path.join(t, "h.ptu")
        E.write_ptu(p, db.parent, db.blen, db.seq, db.up, db.down, db.height, md, model_text=db.model.text, dg_alpha=db.dg_alpha, dg_breaks=db.dg_b)
        return open(p, "rb").read(HEAD)


@pytest.mark.parametrize("name", CASES)
def test_encode_gives_the_reference_bytes(tmp_path, name):
    a, gold = case(name)
    cs, ident = unweighted_cs(a)
    p = tmp_path / "x.csfm"
    E.csfm_encode(p, a, cs, ident, case_sa(name)[1])
    got = p.read_bytes()
    assert got[:HEAD] == ptu_head() and got[:8] == b"HmmUFOtu"
    assert len(got) - HEAD == len(gold) and got[HEAD:] == gold
    E.csfm_encode(p, [bytes(r) for r in a], cs.encode(), list(ident), case_sa(name)[1].tolist())       # rows as a list of bytes
    assert p.read_bytes() == got


class _Hmm:          # every 5th column a match column, as tests/test_csfm.py
    def __init__(self, cs_len):
        cols = np.arange(3, cs_len, 5)
        self.K = len(cols)
        self.p2cs = np.zeros(self.K + 2, np.int32); self.p2cs[1:self.K + 1] = cols + 1; self.p2cs[self.K + 1] = cs_len + 1


def test_reader_takes_the_file_with_and_without_its_head(tmp_path):
    a, gold = case("70_otus")
    cs, ident = unweighted_cs(a)
    with_head, bare = tmp_path / "head.csfm", tmp_path / "bare.csfm"
    E.csfm_encode(with_head, a, cs, ident, case_sa("70_otus")[1])
    bare.write_bytes(with_head.read_bytes()[HEAD:])
    hits = [l.rstrip("\n").split("\t") for l in open(os.path.join(G, "csfm_70otus_hits.tsv"))]
    hmm = _Hmm(a.shape[1])
    checked = crossed = 0
    for k in sorted({len(h[0]) for h in hits}):
        ixs = [E.SeedIndex(None, None, hmm, k, csfm=p) for p in (with_head, bare)]
        assert ixs[0].positions == ixs[1].positions and ixs[0].size == ixs[1].size
        for pat, s, e, n in hits:
            if len(pat) != k:
                continue
            got = ixs[0].locate_first(pat)
            assert got == ixs[1].locate_first(pat) and got[2] == int(n), pat
            if got[:2] != (int(s), int(e)):        # the reference's accessSA walk left its sequence through the front: tests/test_csfm.py::test_first_hit_is_locate_first
                nocc, sq, off, col = ixs[0].occurrences(pat)
                assert off[0] < 4 and col[0] + 1 == got[0], pat
                crossed += 1
            checked += 1
    assert checked == len(hits) >= 400 and crossed <= 60
    short = tmp_path / "short.csfm"; short.write_bytes(with_head.read_bytes()[:HEAD + 4])
    with pytest.raises(E.EngineError):
        E.SeedIndex(None, None, hmm, 20, csfm=short)


def test_refusals(tmp_path):
    lib = E.load_library()
    a = case("b")[0]
    cs, ident = unweighted_cs(a)
    sa = case_sa("b")[1]
    p = tmp_path / "no.csfm"
    with pytest.raises(E.EngineError) as ei:                                       # a text symbol above 4, before a device is asked for
        E.suffix_array(np.array([1, 2, 5, 0], np.uint8))
    assert "error -1" in str(ei.value) and "symbol 5 at text position 2" in str(ei.value)
    one = np.zeros(1, np.uint8); out = np.zeros(1, np.int32)
    for n in (0, 2 ** 31, 2 ** 40):                                                # N out of range: refused before the text is read or anything allocated
        assert lib.hu_suffix_array(C.c_int(0), one.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int64(n), out.ctypes.data_as(C.POINTER(C.c_int32)), None, None) == -1
        assert "2^31" in lib.hu_last_error().decode()
    with pytest.raises(E.EngineError):                                             # a row length that is not cs_len
        E.csfm_encode(p, [b"ACGT-ACGTTTGA", b"ACGT"], cs, ident, sa)
    with pytest.raises(E.EngineError):
        E.csfm_encode(p, a, cs[:-1], ident, sa)
    rows = a.tobytes()
    idp = np.ascontiguousarray(ident).ctypes.data_as(C.POINTER(C.c_double)); sap = sa.ctypes.data_as(C.POINTER(C.c_int32))
    for bad_cs in (cs[:-1].encode(), cs.encode() + b"A"):
        assert lib.hu_csfm_encode(str(p).encode(), C.c_int64(1), C.c_int64(13), rows, bad_cs, idp, sap) == -1
        assert "consensus sequence" in lib.hu_last_error().decode()
    assert lib.hu_csfm_encode(str(p).encode(), C.c_int64(1), C.c_int64(65536), rows, cs.encode(), idp, sap) == -1
    assert lib.hu_csfm_encode(str(p).encode(), C.c_int64(2 ** 31), C.c_int64(13), rows, cs.encode(), idp, sap) == -1 and "2^31" in lib.hu_last_error().decode()
    bad = np.array([list(b"ACGT-ACGTTTGA"), list(b"ACG.-AC*TTTGA")], np.uint8)    # neither gap nor residue: named by row and column
    with pytest.raises(E.EngineError) as ei:
        E.csfm_encode(p, bad, cs, ident, np.arange(int((codes(bad) >= 0).sum()) + 3, dtype=np.int32))
    assert "row 2, column 8" in str(ei.value) and "'*'" in str(ei.value)
    with pytest.raises(E.EngineError) as ei:                                       # no permutation
        E.csfm_encode(p, a, cs, ident, np.zeros(14, np.int32))
    assert "permutation" in str(ei.value)
    assert not p.exists()


# ============================================================================= GPU
def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


def sa_text(name):
    rng = np.random.default_rng(17)
    T = E.suffix_array_tile()

    def rnd(n):
        t = rng.integers(0, 5, n).astype(np.uint8); t[-1] = 0
        return t
    if name in CASES:
        return case_sa(name)[0]
    return {"n1": lambda: np.zeros(1, np.uint8), "n2": lambda: np.array([3, 0], np.uint8), "n6": lambda: np.array([1, 0, 0, 2, 0, 0], np.uint8),
            "equal5000": lambda: np.concatenate([np.full(5000, 2, np.uint8), np.zeros(1, np.uint8)]),
            "acac4097": lambda: np.array(([1, 2] * 2049)[:4097], np.uint8),
            "T-1": lambda: rnd(T - 1), "T": lambda: rnd(T), "T+1": lambda: rnd(T + 1), "2T+1": lambda: rnd(2 * T + 1),
            "64k+1": lambda: rnd(64 * 37 + 1)}[name]()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1", "n2", "n6", "a", "b", "c", "d", "70_otus", "equal5000", "acac4097", "T-1", "T", "T+1", "2T+1", "64k+1"])
def test_suffix_array(name):
    need_gpu()
    t = sa_text(name)
    want = case_sa(name)[1] if name in CASES else np_suffix_array(t)
    sa, rounds, sec = E.suffix_array(t, info=True)
    print("%s: N = %d, %d doubling rounds, %.2f ms on the device" % (name, len(t), rounds, sec * 1e3))
    assert sa.dtype == np.int32 and np.array_equal(sa, want)
    assert rounds <= int(np.ceil(np.log2(max(len(t), 2)))) + 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_csfm_write_gives_the_reference_bytes(tmp_path, name):
    need_gpu()
    a, gold = case(name)
    cs, ident = unweighted_cs(a)
    p = tmp_path / "x.csfm"
    E.csfm_write(p, a, cs, ident)
    got = p.read_bytes()
    assert got[:HEAD] == ptu_head() and got[HEAD:] == gold
    t = E.csfm_write_timing()
    assert t["rounds"] >= 0 and t["device"] >= t["suffix_array"] > 0


@pytest.mark.gpu
def test_program_writes_the_csfm_beside_the_same_ptu(tmp_path):
    need_gpu()
    fasta, tree, tax = (os.path.join(REF, f) for f in ("70_otus.fasta.gz", "70_otus.tree", "70_otus_taxonomy.txt"))
    args = [fasta, tree, "--no-hmm", "-sm", os.path.join(REF, "gg_97_otus_JC69.sm"), "-a", tax, "-n", "db", "-v"]
    plain, both = tmp_path / "plain", tmp_path / "both"
    for d, extra in ((plain, []), (both, ["--csfm"])):
        d.mkdir()
        r = subprocess.run([BIN] + args + extra, cwd=str(d), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(plain)) == ["db.ptu"] and sorted(os.listdir(both)) == ["db.csfm", "db.ptu"]
    assert "CSFM index built" in r.stderr and "CSFM saved" in r.stderr
    assert (plain / "db.ptu").read_bytes() == (both / "db.ptu").read_bytes()
    a, gold = case("70otus_pruned")
    st = E.msa_stats(case("70_otus")[0])
    keep = st["keep"]
    assert keep.sum() == a.shape[1] and np.array_equal(case("70_otus")[0][:, keep], a)
    cs = "".join("ACGT"[int(w.argmax())] if w.max() >= g else "-" for w, g in zip(st["res_wcount"][:, keep].T, st["gap_wcount"][keep]))      # MSA::calculateCS
    got = (both / "db.csfm").read_bytes()
    L = a.shape[1]
    lo, hi = CS_AT + 8 + 1, CS_AT + 8 + 1 + L
    assert got[:HEAD] == ptu_head() and got[lo:hi] == cs.encode()
    assert got[HEAD:lo] == gold[:lo - HEAD] and got[hi:] == gold[hi - HEAD:] and len(got) == len(gold) + HEAD
    assert cs != unweighted_cs(a)[0] or got[HEAD:] == gold                         # the weights matter on this alignment, or the files agree entirely
    # hmmufotu-amd on the reads of tests/test_build_program.py::test_built_database_downstream: the same TSV with this .csfm as with csfm_ref's
    db = synth.make_db_70otus()
    rng = np.random.default_rng(9)
    reads, leaves = [], np.nonzero(db.is_leaf)[0]
    while len(reads) < 64:
        s = "".join("ACGT"[c] for c in db.seq[int(rng.choice(leaves))] if c >= 0)
        if len(s) >= 300:
            k = int(rng.integers(0, len(s) - 250)); reads.append(s[k:k + 250])
    golden_dir = tmp_path / "golden"; golden_dir.mkdir()
    (golden_dir / "db.ptu").write_bytes((both / "db.ptu").read_bytes()); (golden_dir / "db.csfm").write_bytes(gold)
    out = []
    for d in (both, golden_dir):
        synth.write_hmm(db.hmm, str(d / "db.hmm"))
        with open(d / "reads.fq", "w") as f:
            for i, s in enumerate(reads):
                f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        c = subprocess.run([CLI, "db", "reads.fq", "-o", "out.tsv", "-v"], cwd=str(d), capture_output=True, text=True, timeout=300)
        assert c.returncode == 0 and "seed index read from the .csfm" in c.stderr, c.stderr
        out.append((d / "out.tsv").read_bytes())
    assert out[0] == out[1] and out[0].count(b"\n") >= 1 + 60


@pytest.mark.gpu
def test_program_refuses_a_byte_outside_the_alphabet(tmp_path):
    need_gpu()
    rows = [("A", "ACGTACGTAC--GTACGTAC"), ("B", "ACGTACGTACGTGTAC*TAC"), ("C", "ACGAACGTAC--GTACGTAC")]
    with open(tmp_path / "m.fa", "w") as f:
        for nm, s in rows:
            f.write(">%s\n%s\n" % (nm, s))
    (tmp_path / "m.tree").write_text("(A:0.1,B:0.2,C:0.3);\n")
    r = subprocess.run([BIN, "m.fa", "m.tree", "--no-hmm", "-sm", os.path.join(REF, "gg_97_otus_JC69.sm"), "-n", "db", "--csfm"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Unable to build CSFM index" in r.stderr and "row 2, column 17" in r.stderr and "'*'" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == ["m.fa", "m.tree"]


def test_program_help_names_the_flag():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--csfm" in r.stderr and "<NAME>.csfm" in r.stderr
