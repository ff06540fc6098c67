"""hmmufotu-amd-anneal: primer coverage of a database (the reference's hmmufotu-anneal, src/hmmufotu-anneal.cpp:246-290).

CPU: the match rule of DegenAlphabet::isMatch per alignment byte, the hit threshold, the report header, the CLI's option checks.
GPU: hu_anneal_batch / Database.anneal / the CLI against a numpy restatement that runs isMatch over every node's codes on the
oracle's unseeded GLOBAL alignment of each primer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import get_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-anneal")
REF_SEQ = os.path.join(ROOT, "oracle", "_ref", "libref_seq.so")

IUPAC = {"U": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT", "V": "ACG", "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}
ANNEAL_HEADER = ("id\tdescription\tsequence\tstrand\tCS_start\tCS_end\talignment\ttotal_nodes\ttotal_leaves\thit_nodes\thit_leaves\t"
                 "efficiency_nodes\tefficiency_leaves")


def _encode(c: str) -> int:
    """IUPACNucl's sym_map: A C G T, a degenerate letter as the first base of its expansion, gaps -2, the rest -1"""
    if c in "ACGT":
        return "ACGT".index(c)
    if c in IUPAC:
        return "ACGT".index(IUPAC[c][0])
    return -2 if c in "-._" else -1


def _bit(code: int) -> int:
    return {-2: 4, -1: 5}.get(code, code)


def restated_table() -> np.ndarray:
    """isMatch(c, b) (src/DegenAlphabet.cpp:70-76) as the set of node codes b that c matches: c itself and its expansion"""
    t = np.zeros(256, np.uint8)
    for c in range(128):
        for ch in chr(c) + IUPAC.get(chr(c), ""):
            t[c] |= 1 << _bit(_encode(ch))
    t[128:] = 1 << 5
    return t


def leaf_flags(parent) -> np.ndarray:
    """PTUNode::isLeaf: one neighbour (src/PhyloTreeUnrooted.h:199)"""
    parent = np.asarray(parent)
    deg = (parent >= 0).astype(np.int64)
    np.add.at(deg, parent[parent >= 0], 1)
    return deg == 1


def restate_hits(align: str, cs_start: int, cs_end: int, seq: np.ndarray, is_leaf: np.ndarray, max_dist: float):
    """SeqUtils::pDist(aln.align, node seq, csStart - 1, csEnd - 1) <= maxDist over every node (src/SeqUtils.cpp:77-85)"""
    tab = restated_table()
    reg = np.frombuffer(align[cs_start - 1:cs_end].encode("latin1"), np.uint8)
    codes = seq[:, cs_start - 1:cs_end].astype(np.int64)
    cls = np.where(codes >= 0, codes, np.where(codes == -2, 4, 5))
    mism = ((tab[reg][None, :].astype(np.int64) >> cls) & 1) == 0
    d = mism.sum(axis=1)
    hit = np.array([float(x) / (cs_end - cs_start + 1) <= max_dist for x in d])
    return int(hit.sum()), int((hit & is_leaf).sum())


COMPL = {"A": "T", "T": "A", "C": "G", "G": "C", "U": "A", "Y": "R", "R": "Y", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B",
         "D": "H", "H": "D", "N": "N"}


def revcom_case(s: str) -> str:
    """PrimarySeq::revcom with IUPACNucl::getComplementSymbol (src/IUPACNucl.h:73-75): a lower-case letter is complemented in lower case"""
    return "".join((COMPL.get(c.upper(), c.upper()).lower() if c.islower() else COMPL.get(c, c)) for c in reversed(s))


def restore_case(a, text):
    """buildGlobalAlign (src/BandedHMMP7.cpp:1035-1046) writes a matched base as it was read: the M states of the trace take the upper-case
    letters of the region in order, and the one whose base was read in lower case is lower-case"""
    reg = list(a["align"][a["csStart"] - 1:a["csEnd"]])
    j, c = a["seqStart"] - 1, 0
    for st in a["trace"]:
        if st == "I":
            j += 1
        elif st == "M":
            while not reg[c].isupper():
                c += 1
            if text[j].islower():
                reg[c] = reg[c].lower()
            c += 1; j += 1
    return a["align"][:a["csStart"] - 1] + "".join(reg) + a["align"][a["csEnd"]:]


def restate_anneal(H, primers, seq, parent, identity, strand):
    """the per-primer loop of src/hmmufotu-anneal.cpp:246-290 on the oracle's alignments of the upper-cased bases, with the alignment in
    the case the primer was read; None where no strand aligns"""
    max_dist = 1 - identity
    is_leaf = leaf_flags(parent)
    out = []
    for p in primers:
        st, cost, aln = ".", np.inf, None
        if strand & 1:
            st = "+"
            a = H.align(p.upper())
            if a["ok"]:
                aln, cost = dict(a, align=restore_case(a, p)), a["cost"]
        if strand & 2:
            rc = revcom_case(p)
            a = H.align(rc.upper())
            if a["ok"] and a["cost"] < cost:
                st, aln = "-", dict(a, align=restore_case(a, rc))
        if aln is None:
            out.append(None)
            continue
        hn, hl = restate_hits(aln["align"], aln["csStart"], aln["csEnd"], seq, is_leaf, max_dist)
        out.append(dict(strand=st, cs_start=aln["csStart"], cs_end=aln["csEnd"], alignment=aln["align"][aln["csStart"] - 1:aln["csEnd"]],
                        n_nodes=len(parent), n_leaves=int(is_leaf.sum()), hit_nodes=hn, hit_leaves=hl))
    return out


def make_primers(db, n, rng, length=20):
    """primers cut from leaf sequences: exact, with degenerate letters (N, U, 2- and 3-way codes), with an inserted base (lower-case
    insert letters in the alignment), with a dropped base (gaps), reverse-complemented, and one palindrome (equal costs: '+' kept)"""
    from hmmufotu_amd.synth import revcom
    leaves = np.flatnonzero(db.is_leaf) if db.is_leaf is not None else np.flatnonzero(leaf_flags(db.parent))
    out = []
    while len(out) < n:
        k = len(out)
        row = db.seq[rng.choice(leaves)]
        bases = np.flatnonzero(row >= 0)
        if len(bases) < length + 10:
            continue
        i0 = int(rng.integers(0, len(bases) - length - 2))
        s = list("".join("ACGT"[row[c]] for c in bases[i0:i0 + length]))
        kind = k % 6
        if kind == 1:
            for j, ch in zip(rng.choice(length, 4, replace=False), ("N", "R", "V", "D" if k % 12 == 1 else "U")):
                s[j] = ch
        elif kind == 2:
            s.insert(length // 2, "ACGT"[int(rng.integers(4))]); s.insert(length // 2, "ACGT"[int(rng.integers(4))])
        elif kind == 3:
            del s[length // 2]
        elif kind == 5:
            s[int(rng.integers(length))] = "ACGT"[int(rng.integers(4))]; s[3] = "Y"; s[7] = "B"; s[9] = "H"
        p = "".join(s)
        out.append(revcom(p) if kind == 4 or k % 5 == 4 else p)
    half = "GATCCATGCA"
    out[n // 2] = half + revcom(half)
    return out


def _lib():
    from hmmufotu_amd import engine as E
    return E


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_match_table_is_the_restated_ismatch():
    E = _lib()
    assert np.array_equal(E.anneal_match_table(), restated_table())


@pytest.mark.skipif(not os.path.exists(REF_SEQ), reason="oracle/_ref/libref_seq.so not built (needs the reference tree)")
def test_match_table_against_the_reference_encode():
    """per byte 0..127: encode(c) and the encodings of its IUPAC expansion, with the reference's own alphabet (ref_encode)"""
    E = _lib()
    lib = C.CDLL(REF_SEQ)
    lib.ref_encode.argtypes = [C.c_char]
    enc = lambda ch: (lambda v: -1 if v == -100 else v)(lib.ref_encode(ch.encode("latin1")))
    tab = E.anneal_match_table()
    for c in range(128):
        want = 0
        for ch in chr(c) + IUPAC.get(chr(c), ""):
            want |= 1 << _bit(enc(ch))
        assert tab[c] == want, (c, chr(c), tab[c], want)
    assert all(tab[c] == 1 << 5 for c in range(128, 256))


def test_hit_threshold_at_the_boundaries():
    E = _lib()
    for identity, length, want in [(0.9, 20, 1), (0.8, 20, 3), (0.75, 20, 5), (1.0, 20, 0), (0.0, 20, 20), (0.9, 10, 0), (0.5, 7, 3), (0.95, 1, 0)]:
        md = 1 - identity
        got = E.anneal_max_mismatch(md, length)
        assert got == want, (identity, length, got)
        assert got == max(d for d in range(-1, length + 1) if d < 0 or d / length <= md)
    assert E.anneal_max_mismatch(1 - 0.9, 0) == -1


def test_header_is_the_reference_anneal_header():
    E = _lib()
    lib = E.load_library()
    lib.hu_anneal_header.restype = C.c_char_p
    assert lib.hu_anneal_header().decode() == ANNEAL_HEADER


@pytest.mark.parametrize("args,msg", [(["-i", "1.5"], "-i|--identity must between 0 and 1"), (["--identity", "nan"], "-i|--identity must between 0 and 1"),
                                      (["-s", "0"], "-s|--strand must be 1, 2 or 3"), (["--strand", "4"], "-s|--strand must be 1, 2 or 3")])
def test_cli_option_validation(args, msg, tmp_path):
    p = subprocess.run([CLI, str(tmp_path / "db"), str(tmp_path / "p.fa")] + args, capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr.strip() == msg and p.stdout == ""


def test_cli_usage_and_positional_count(tmp_path):
    p = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "Usage:" in p.stderr
    p = subprocess.run([CLI, str(tmp_path / "db")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr.startswith("Error:\n")


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def _oracle_hmm(db):
    from oracle import oracle_py as O
    h = db.hmm
    return O.Hmm(h.K, h.L, h.EM, h.EI, h.T, h.p2cs, 0)


def _check(D, H, primers, seq, parent, identity, strand):
    got = D.anneal(primers, identity=identity, strand=strand)
    want = restate_anneal(H, primers, seq, parent, identity, strand)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, primers[i], identity, strand, g, w)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["synthetic", "70_otus"])
def test_anneal_against_the_restatement(which):
    from hmmufotu_amd import engine as E, synth
    db = get_db() if which == "synthetic" else synth.make_db_70otus()
    rng = np.random.default_rng(5 if which == "synthetic" else 6)
    primers = make_primers(db, 44, rng)         # > 5 tiles of 8 primers, regions all over the profile
    H = _oracle_hmm(db)
    D = E.Database.from_synth(db)
    try:
        seen = set()
        for strand in (3, 1, 2):
            for identity in (1.0, 0.9, 0.8, 0.75):
                got = _check(D, H, primers, db.seq, db.parent, identity, strand)
                seen |= {g["strand"] for g in got if g}
                if strand == 3 and identity == 0.9:
                    pal = got[len(primers) // 2]
                    assert pal["strand"] == "+"
                    assert any(any(c.islower() for c in g["alignment"]) for g in got if g)
                    assert any("-" in g["alignment"] for g in got if g)
        assert seen == {"+", "-"}
    finally:
        D.close()


@pytest.mark.gpu
def test_anneal_root_with_one_child_is_a_leaf():
    """a new root above the old one: it has one neighbour, so it counts as a leaf (src/PhyloTreeUnrooted.h:199)"""
    from hmmufotu_amd import engine as E
    db = get_db()
    n = db.n_nodes
    old_root = int(np.flatnonzero(db.parent < 0)[0])
    parent = np.append(db.parent, -1).astype(np.int32); parent[old_root] = n
    blen = np.append(db.blen, 0.0); blen[old_root] = 0.01
    seq = np.concatenate([db.seq, db.seq[old_root:old_root + 1]])
    up = np.concatenate([db.up, db.up[old_root:old_root + 1]]); down = np.concatenate([db.down, db.down[old_root:old_root + 1]])
    height = np.append(db.height, db.height[old_root] + 0.01)
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k > 0 else None)
    D = E.Database.from_arrays(db.hmm, parent, blen, seq, up, down, height, md)
    try:
        assert leaf_flags(parent)[n] and D.num_leaves() == int(leaf_flags(parent).sum()) == int(leaf_flags(db.parent).sum()) + 1
        primers = make_primers(db, 12, np.random.default_rng(8))
        _check(D, _oracle_hmm(db), primers, seq, parent, 0.9, 3)
    finally:
        D.close()


@pytest.mark.gpu
def test_anneal_invalid_node_codes():
    """node codes -1 (the planes hold them as v = 0 like gaps): the lower-case inserts of the primers' alignments match only them"""
    from hmmufotu_amd import engine as E
    db = get_db()
    H = _oracle_hmm(db)
    primers = [p for p in make_primers(db, 48, np.random.default_rng(9))]
    ins_cols = set()
    for p in primers:
        a = H.align(p)
        if a["ok"]:
            ins_cols |= {c for c in range(a["csStart"] - 1, a["csEnd"]) if a["align"][c].islower()}
    assert ins_cols
    seq = db.seq.copy()
    rng = np.random.default_rng(10)
    for c in ins_cols:
        seq[rng.random(db.n_nodes) < 0.6, c] = -1
    seq[rng.random(seq.shape) < 0.02] = -1
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k > 0 else None)
    D = E.Database.from_arrays(db.hmm, db.parent, db.blen, seq, db.up, db.down, db.height, md)
    try:
        for identity in (0.9, 0.75):
            _check(D, H, primers, seq, db.parent, identity, 3)
    finally:
        D.close()


@pytest.mark.gpu
def test_anneal_refuses_a_column_window():
    from hmmufotu_amd import engine as E
    db = get_db()
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k > 0 else None)
    half = db.cs_len // 2
    D = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, db.up[:, :half], db.down[:, :half], db.height, md, win_start=0, win_len=half)
    try:
        with pytest.raises(E.EngineError, match="column window"):
            D.anneal(make_primers(db, 3, np.random.default_rng(1)))
    finally:
        D.close()


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path):
    from hmmufotu_amd import synth
    db = get_db()
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    primers = make_primers(db, 30, np.random.default_rng(12))
    fa = tmp_path / "primers.fasta"
    fa.write_text("".join(">p%d %s\n%s\n" % (i, "primer number %d" % i if i % 3 else "", p) for i, p in enumerate(primers)))
    H = _oracle_hmm(db)
    for identity, strand in ((0.8, 3), (0.9, 2)):
        out = tmp_path / ("o_%s_%d.tsv" % (identity, strand))
        p = subprocess.run(["timeout", "-k", "10", "300", CLI, pre, str(fa), "-o", str(out), "-i", str(identity), "-s", str(strand), "--batch", "7"],
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        lines = out.read_text().split("\n")
        assert lines[0] == ANNEAL_HEADER and lines[-1] == ""
        want = restate_anneal(H, primers, db.seq, db.parent, identity, strand)
        assert len(lines) - 2 == len(want)
        for i, (line, w) in enumerate(zip(lines[1:-1], want)):
            exp = ["p%d" % i, "primer number %d" % i if i % 3 else "", primers[i], w["strand"], str(w["cs_start"]), str(w["cs_end"]), w["alignment"],
                   str(w["n_nodes"]), str(w["n_leaves"]), str(w["hit_nodes"]), str(w["hit_leaves"]),
                   "%g" % (w["hit_nodes"] / w["n_nodes"]), "%g" % (w["hit_leaves"] / w["n_leaves"])]
            assert line.split("\t") == exp, (i, line, exp)


def _mixed_case(primers, rng):
    """every third primer all lower-case, every third one with random letters lower-cased"""
    out = []
    for i, p in enumerate(primers):
        if i % 3 == 1:
            p = p.lower()
        elif i % 3 == 2:
            p = "".join(c.lower() if rng.random() < 0.4 else c for c in p)
        out.append(p)
    return out


def test_revcom_keeps_case():
    from hmmufotu_amd import engine as E
    for s in ("acgtNuRyKm", "ACGTUYRSWKMBVDHN", "acgtuyrswkmbvdhn", "aCgT-X.n"):
        assert E.revcom_as_read(s) == revcom_case(s)
    assert revcom_case("aCgTu") == "aAcGt"


@pytest.mark.gpu
def test_anneal_mixed_case_primers():
    """primers read in lower or mixed case: the alignment keeps a matched base's case (a lower-case one matches only node code -1)"""
    from hmmufotu_amd import engine as E, synth
    db = synth.make_db_70otus()
    rng = np.random.default_rng(21)
    primers = _mixed_case(make_primers(db, 30, rng), rng)
    H = _oracle_hmm(db)
    D = E.Database.from_synth(db)
    try:
        for strand in (3, 2):
            for identity in (0.9, 0.75):
                got = _check(D, H, primers, db.seq, db.parent, identity, strand)
                assert any(any(c.islower() for c in g["alignment"]) for g in got if g)
    finally:
        D.close()


@pytest.mark.gpu
def test_cli_mixed_case_fields(tmp_path):
    """id, description and sequence as the reference's SeqIO gives them (ref_seqio_read when built), rows as restated"""
    from hmmufotu_amd import synth
    db = get_db()
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    rng = np.random.default_rng(22)
    primers = _mixed_case(make_primers(db, 12, rng), rng)
    fa = tmp_path / "mixed.fasta"
    fa.write_text("".join(">m%d \t some  desc %d\n%s\n%s\n" % (i, i, p[:9], p[9:]) for i, p in enumerate(primers)))
    out = tmp_path / "o.tsv"
    p = subprocess.run(["timeout", "-k", "10", "300", CLI, pre, str(fa), "-o", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = [ln.split("\t") for ln in out.read_text().split("\n")[1:-1]]
    want = restate_anneal(_oracle_hmm(db), primers, db.seq, db.parent, 0.9, 3)
    assert [r[:3] for r in rows] == [["m%d" % i, "some  desc %d" % i, pr] for i, pr in enumerate(primers)]
    for r, w in zip(rows, want):
        assert r[3:11] == [w["strand"], str(w["cs_start"]), str(w["cs_end"]), w["alignment"], str(w["n_nodes"]), str(w["n_leaves"]),
                           str(w["hit_nodes"]), str(w["hit_leaves"])]
    if os.path.exists(REF_SEQ):
        lib = C.CDLL(REF_SEQ)
        lib.ref_seqio_read.restype = C.c_long
        buf = C.create_string_buffer(1 << 16)
        k = lib.ref_seqio_read(str(fa).encode(), b"fasta", buf, C.c_long(len(buf)))
        assert k == len(primers)
        ref = [ln.split("\x1f") for ln in buf.value.decode().split("\n")[:-1]]
        assert [r[:3] for r in rows] == ref
