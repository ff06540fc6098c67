"""hmmufotu-amd --otu-table / --otu-cs: a run that summarises its sample from the batches as they finish, and the
library entries behind it: hu_batch_get_summary, hu_sum_accept, hu_otucs_add_batch, hu_otucs_add_counts.

CPU: every refusal of the new options (one line on stderr, before a device is asked for) and hu_sum_accept on hand-made records.
GPU, library: the summary records against a numpy restatement from the rows hu_batch_get_alignments downloads; the counts hu_otucs_add_batch
leaves against those of hu_otucs_add on the downloaded rows under the same mask.  The database has an odd cs_len (rows are never 16-byte
aligned) whose first and last columns are match columns, so a read can cover columns 0 .. cs_len - 1.
GPU, end to end: the table and the FASTA of one run against hmmufotu-amd-sum and hmmufotu-amd-otu-cs on that run's own assignment file,
with all four filters set and --otu-q on a printed Q_taxon value.  Integers and bytes throughout: no tolerance anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsv_consumers as C  # noqa: E402
from conftest import get_db  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SYMBOLS = np.frombuffer(b"ACGTUMRWSYKVHDBN", np.uint8)          # is_symbol of hmmufotu_amd/csrc/hu_sum_rule.h
NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
LIB_DB = dict(n_leaves=60, cs_len=1333, model="GTR", dg_k=4, seed=17)          # the seed: see _lib_db


def _bin(name):
    p = os.path.join(HERE, "..", "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return os.path.abspath(p)


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=300, **kw)


# ------------------------------------------------------------------------------------------------ CPU
def test_refusals_run_without_a_device(tmp_path):
    exe = _bin("hmmufotu-amd")
    env = dict(os.environ, **NO_DEVICE)
    t, c = str(tmp_path / "a.otu"), str(tmp_path / "a.fa")
    p = _run([exe, "--help"], env=env)
    assert p.returncode == 0 and "--otu-table FILE" in p.stderr and "--no-tsv" in p.stderr
    need = "need --otu-table or --otu-cs"
    for args, msg in (
            (["--otu-table", t, "--align-only"], "cannot be used with --align-only"),
            (["--otu-cs", c, "--align-only"], "cannot be used with --align-only"),
            (["--otu-q", "1", "--align-only"], "cannot be used with --align-only"),
            (["--otu-table", t, "--col-windows", "2"], "cannot be used with --col-windows above 1"),
            (["--otu-cs", c, "--otu-no-gap", "--col-windows", "3"], "cannot be used with --col-windows above 1"),
            (["--otu-q", "1"], need), (["--otu-aln-iden", "0.5"], need), (["--otu-hmm-iden", "0.5"], need), (["--otu-min-reads", "2"], need),
            (["--otu-no-gap"], need), (["--otu-effN", "1"], need), (["--sample", "s"], need), (["--use-dbname"], need),
            (["--no-tsv"], "--no-tsv needs --otu-table or --otu-cs"),
            (["--no-tsv", "--otu-table", t, "-o", str(tmp_path / "x.tsv")], "--no-tsv cannot be used with -o, -a, --chimera-out or --chimera-info"),
            (["--no-tsv", "--otu-cs", c, "-a", str(tmp_path / "x.aln")], "--no-tsv cannot be used with"),
            (["--no-tsv", "--otu-table", t, "-C", "--chimera-out", str(tmp_path / "x.chi")], "--no-tsv cannot be used with"),
            (["--no-tsv", "--otu-table", t, "-C", "--chimera-info"], "--no-tsv cannot be used with"),
            (["--otu-cs", c, "--otu-effN", "-1"], "--otu-effN must be non-negative"),
            (["--otu-cs", c, "--otu-effN", "nan"], "--otu-effN must be non-negative"),
            (["--otu-table", t, "--otu-min-reads", "-1"], "--otu-min-reads must be non-negative integer"),
            (["--otu-table"], "needs a value")):
        p = _run([exe, "db", "reads.fa"] + args, env=env)
        assert p.returncode not in (0, -6, -11) and msg in p.stderr, (args, p.returncode, p.stderr)
        assert len(p.stderr.strip().split("\n")) == 1 and "device" not in p.stderr, (args, p.stderr)
        assert not os.path.exists(t) and not os.path.exists(c)


def _rec(in_main=1, taxon=5, q=10.0, n_cols=100, n_sym=90, n_match=80, n_match_sym=72):
    return (in_main, taxon, q, n_cols, n_sym, n_match, n_match_sym)


def test_sum_accept_on_hand_made_records():
    from hmmufotu_amd import engine as E
    R = lambda rows: np.array(rows, E.SUM_DTYPE)
    base = R([_rec(), _rec(in_main=0), _rec(taxon=-1), _rec(q=float("nan")), _rec(taxon=0, q=0.0)])
    assert E.sum_accept(base).tolist() == [1, 0, 0, 0, 1]
    # Q_taxon is compared as the assignment file prints it: 0.123456789 shows as 0.123457, 1234567.4 as 1.23457e+06
    q = R([_rec(q=0.123456789), _rec(q=0.12345651), _rec(q=1234567.4), _rec(q=1234574.9), _rec(q=float("inf"))])
    assert E.sum_accept(q, min_q=0.123457).tolist() == [1, 1, 1, 1, 1]          # a threshold exactly at the printed value
    assert E.sum_accept(q, min_q=0.1234570001).tolist() == [0, 0, 1, 1, 1]
    assert E.sum_accept(q, min_q=1234570.0).tolist() == [0, 0, 1, 1, 1]
    assert E.sum_accept(q, min_q=1234570.5).tolist() == [0, 0, 0, 0, 1]
    # the identities are id / n in double, compared with >=
    a = R([_rec(n_cols=4, n_sym=3), _rec(n_cols=3, n_sym=1), _rec(n_cols=7, n_sym=7), _rec(n_cols=0, n_sym=0)])
    assert E.sum_accept(a, min_aln=0.75).tolist() == [1, 0, 1, 0]               # 3 / 4 at the threshold; 0 / 0 rejects
    assert E.sum_accept(a, min_aln=0.7500000001).tolist() == [0, 0, 1, 0]
    assert E.sum_accept(a, min_aln=1.0 / 3.0).tolist() == [1, 1, 1, 0]
    assert E.sum_accept(a, min_aln=0.0).tolist() == [1, 1, 1, 1]                 # 0 skips the test, the 0 / 0 with it
    h = R([_rec(n_match=0, n_match_sym=0), _rec(n_match=10, n_match_sym=9), _rec(n_match=10, n_match_sym=8), _rec(n_match=3, n_match_sym=0)])
    assert E.sum_accept(h, min_hmm=0.9).tolist() == [0, 1, 0, 0]                # n_match = 0: 0 / 0 is NaN, which no threshold accepts
    assert E.sum_accept(h, min_hmm=1e-300).tolist() == [0, 1, 1, 0]
    assert E.sum_accept(h, min_hmm=0.0).tolist() == [1, 1, 1, 1]
    assert E.sum_accept(h, min_q=10.0, min_aln=0.9, min_hmm=0.8).tolist() == [0, 1, 1, 0]
    assert E.sum_accept(h, min_q=10.0, min_aln=0.91, min_hmm=0.8).tolist() == [0, 0, 0, 0]
    assert len(E.sum_accept(R([]))) == 0


# ------------------------------------------------------------------------------------------------ GPU, library
def _lib_db():
    """119 nodes, cs_len 1,333 (odd: row r starts at byte 1,333 r), 243 match columns; the seed is the first one whose profile has its
    first and last match column at the two ends of the consensus, so that a read can have the region 1 .. cs_len"""
    db = get_db(**LIB_DB)
    assert db.cs_len % 2 == 1 and db.hmm.p2cs[1] == 1 and db.hmm.p2cs[db.hmm.K] == db.cs_len
    return db


def _row_read(db, node, c0, c1, rng=None, n_mut=0):
    """the bases of a node's own row over columns [c0, c1) as a read, n_mut of them changed"""
    from hmmufotu_amd import synth
    cols = c0 + np.nonzero(db.seq[node, c0:c1] >= 0)[0]
    b = np.array(db.seq[node, cols])
    for k in (rng.choice(len(b), n_mut, replace=False) if n_mut else []):
        b[k] = (b[k] + 1 + rng.integers(3)) % 4
    return synth.SimRead(synth.BASES[b].tobytes().decode(), cols, node, 0.0, c0, c1 - 1)


def _vps(db, reads):
    from hmmufotu_amd import synth
    return np.stack([synth.read_vpaths(db.hmm, r) for r in reads])


def _restate_summary(db, recs, rows, best):
    """hu_batch_get_summary from the downloaded rows: the counts of hu_tsv::align_identity / hmm_identity over CS_start - 1 .. CS_end - 1"""
    from hmmufotu_amd import engine as E
    L = db.cs_len
    match = np.zeros(L, bool); match[np.asarray(db.hmm.p2cs[1:]) - 1] = True
    out = np.zeros(len(recs), E.SUM_DTYPE)
    for r in range(len(recs)):
        ok = recs["status"][r] == E.READ_OK
        out["in_main"][r] = int(ok)
        placed = best["c_node"][r] >= 0
        out["taxon"][r] = best["a_node"][r] if placed else -1
        out["q_taxon"][r] = best["q_taxon"][r] if placed else np.nan
        if ok:
            lo, hi = int(recs["cs_start"][r]) - 1, int(recs["cs_end"][r]) - 1
            sym = np.isin(rows[r, lo:hi + 1], SYMBOLS)
            out["n_cols"][r] = hi - lo + 1; out["n_sym"][r] = sym.sum()
            out["n_match"][r] = match[lo:hi + 1].sum(); out["n_match_sym"][r] = (sym & match[lo:hi + 1]).sum()
    return out


@pytest.fixture(scope="module")
def lib():
    """one single-end batch of 233 reads (200 of one leaf, 31 simulated, one that cannot be aligned, one over the whole consensus) and one
    paired batch of 70 (one pair that cannot be aligned, one merged over the whole consensus), assigned once; rows and records downloaded"""
    from hmmufotu_amd import engine as E, synth
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    db = _lib_db()
    L = db.cs_len
    rng = np.random.default_rng(7)
    leaves = np.nonzero(db.is_leaf)[0]
    heavy = int(leaves[3])
    whole_leaf = int(next(u for u in leaves if db.seq[u, 0] >= 0 and db.seq[u, L - 1] >= 0))
    single = [_row_read(db, heavy, 300, 900, rng, 1) for _ in range(200)]
    single += synth.simulate_reads(db, 31, 120, rng, mean_cols=600, sd_cols=30)
    bad = single[200]
    single.append(synth.SimRead(bad.seq[:25] + "?" + bad.seq[26:], bad.cols, bad.node, bad.rc, bad.cs_start, bad.cs_end))
    single.append(_row_read(db, whole_leaf, 0, L))
    ins = synth.simulate_reads(db, 69, 100000, rng, amplicon_start=200, amplicon_cols=800, jitter=20)
    ins.append(_row_read(db, whole_leaf, 0, L))
    fw, mt = [list(x) for x in zip(*[synth.split_pair(r, 90) for r in ins])]
    fw[0] = synth.SimRead(fw[0].seq[:25] + "?" + fw[0].seq[26:], fw[0].cols, fw[0].node, fw[0].rc, fw[0].cs_start, fw[0].cs_end)
    D = E.Database.from_synth(db)
    opts = E.default_opts()
    out = dict(db=db, D=D, E=E, batches=[])
    for reads, mates in ((single, None), (fw, mt)):
        B = E.Batch(D, len(reads))
        if mates is None:
            B.set_reads([r.seq for r in reads], _vps(db, reads))
        else:
            B.set_reads([r.seq for r in reads], _vps(db, reads), [r.seq for r in mates], _vps(db, mates))
        B.assign(opts)
        al = B.alignments()
        rows = np.frombuffer("".join(al["align"]).encode("latin1"), np.uint8).reshape(len(reads), L).copy()
        out["batches"].append(dict(B=B, recs=al["recs"], rows=rows, best=B.placements(), summary=B.summary()))
    yield out
    for b in out["batches"]:
        b["B"].close()
    D.close()


@pytest.mark.gpu
def test_inputs_of_the_library_tests_are_what_they_claim(lib):
    E, db = lib["E"], lib["db"]
    L = db.cs_len
    s, p = lib["batches"]
    assert len(s["recs"]) == 233 and len(p["recs"]) == 70 and 233 % 64 and 70 % 64
    assert s["recs"]["status"][231] != E.READ_OK and p["recs"]["status"][0] != E.READ_OK          # cannot be aligned
    assert (s["recs"]["status"][:231] == E.READ_OK).all() and (p["recs"]["status"][1:] == E.READ_OK).all()
    for b, r in ((s, 232), (p, 69)):                                                            # the whole consensus: columns 0 .. L - 1
        assert b["recs"]["status"][r] == E.READ_OK and b["recs"]["cs_start"][r] == 1 and b["recs"]["cs_end"][r] == L
    # a merged pair: the row holds more bases than one mate has (90), from the first column of its region to the last
    r = 5
    lo, hi = p["recs"]["cs_start"][r] - 1, p["recs"]["cs_end"][r] - 1
    assert np.isin(p["rows"][r, lo:hi + 1], SYMBOLS).sum() > 100 and np.isin(p["rows"][r, [lo, hi]], SYMBOLS).all()
    # more reads of one OTU than one work item of k_otucs_count holds (HU_OTUCS_CHUNK = 64)
    taxa = s["best"]["a_node"][s["summary"]["in_main"] == 1]
    assert np.bincount(taxa).max() >= 65


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_summary_against_the_restatement(lib, which):
    b = lib["batches"][which]
    want = _restate_summary(lib["db"], b["recs"], b["rows"], b["best"])
    got = b["summary"]
    for k in ("in_main", "taxon", "n_cols", "n_sym", "n_match", "n_match_sym"):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(got[k] != want[k])[0][:10])
    assert np.array_equal(got["q_taxon"], want["q_taxon"], equal_nan=True)
    ok = got["in_main"] == 1
    assert (got["n_sym"][ok] > 0).all() and (got["n_match_sym"][ok] <= got["n_sym"][ok]).all() and (got["n_cols"][~ok] == 0).all()
    assert (got["n_sym"][ok] < got["n_cols"][ok]).any() and (got["n_match"][ok] < got["n_cols"][ok]).any()
    # the same records again: the call leaves the batch as it was
    assert np.array_equal(b["B"].summary().tobytes(), got.tobytes())


def _assert_same_counts(a, b, db):
    for u in range(db.n_nodes):
        (fa, ga), (fb, gb) = a.counts(u), b.counts(u)
        assert np.array_equal(fa, fb) and np.array_equal(ga, gb), "counts of node %d differ at columns %s" % (u, np.nonzero((fa != fb).any(0) | (ga != gb))[0][:10])


def _countable(b):
    return (b["summary"]["in_main"] == 1) & (b["summary"]["taxon"] >= 0)


@pytest.mark.gpu
def test_add_batch_against_add_on_the_downloaded_rows(lib):
    E, db, D = lib["E"], lib["db"], lib["D"]
    s, p = lib["batches"]
    rng = np.random.default_rng(3)
    for what in ("none", "all", "filtered", "half", "two batches"):
        got, want = D.otu_consensus(), D.otu_consensus()
        total = 0
        for b in ((s, p) if what == "two batches" else (s,) if what != "half" else (p,)):
            ok = _countable(b)
            if what == "none":
                mask = np.zeros(len(ok), np.uint8)
            elif what == "filtered":
                sm = b["summary"][ok]
                thr = (float(np.sort(sm["q_taxon"])[len(sm) // 10]), float(np.sort(sm["n_sym"] / sm["n_cols"])[len(sm) // 10]),
                       float(np.sort(sm["n_match_sym"] / sm["n_match"])[len(sm) // 10]))
                mask = E.sum_accept(b["summary"], *thr)
                assert 0 < mask.sum() < ok.sum() and not (mask & ~ok).any()
            elif what == "half":
                mask = (ok & (rng.random(len(ok)) < 0.5)).astype(np.uint8)
            else:
                mask = ok.astype(np.uint8)
            got.add_batch(b["B"], mask)
            m = mask.astype(bool)
            if m.any():
                want.add(b["best"]["a_node"][m], b["rows"][m])
            total += int(m.sum())
        _assert_same_counts(got, want, db)
        f, g = got.counts(int(s["best"]["a_node"][0]))
        assert what == "none" or (f.sum(0) + g == (f.sum(0) + g)[0]).all()          # every accepted row counts once in every column
        if what in ("all", "two batches"):
            n_here = sum(int((f.sum(0) + g)[0]) for f, g in (got.counts(u) for u in range(db.n_nodes)))
            assert n_here == total >= 220
        got.close(); want.close()


@pytest.mark.gpu
def test_add_batch_refusals_change_nothing(lib):
    E, db, D = lib["E"], lib["db"], lib["D"]
    s, p = lib["batches"]
    cs, ref = D.otu_consensus(), D.otu_consensus()
    mask = _countable(s).astype(np.uint8)
    cs.add_batch(s["B"], mask); ref.add_batch(s["B"], mask)
    bad = _countable(p).astype(np.uint8); bad[0] = 1                       # the pair that cannot be aligned
    with pytest.raises(E.EngineError, match="no alignment"):
        cs.add_batch(p["B"], bad)
    with pytest.raises(E.EngineError, match="flags for"):
        cs.add_batch(p["B"], mask)
    D2 = E.Database.from_synth(db)
    other = D2.otu_consensus()
    with pytest.raises(E.EngineError, match="another database"):
        other.add_batch(s["B"], mask)
    B = E.Batch(D, 4)
    B.set_reads(["ACGT" * 10] * 4, np.zeros((4, 2, 6), np.int32))
    with pytest.raises(E.EngineError, match="not finished"):
        cs.add_batch(B, np.ones(4, np.uint8))
    with pytest.raises(E.EngineError, match="not finished"):
        B.summary()
    B.close()
    _assert_same_counts(cs, ref, db)
    other.close(); D2.close(); cs.close(); ref.close()


@pytest.mark.gpu
def test_add_counts_is_the_inverse_of_counts(lib):
    E, db, D = lib["E"], lib["db"], lib["D"]
    s, p = lib["batches"]
    L = db.cs_len
    a, b, both = D.otu_consensus(), D.otu_consensus(), D.otu_consensus()
    a.add_batch(s["B"], _countable(s).astype(np.uint8)); b.add_batch(p["B"], _countable(p).astype(np.uint8))
    both.add_batch(s["B"], _countable(s).astype(np.uint8)); both.add_batch(p["B"], _countable(p).astype(np.uint8))
    for u in range(db.n_nodes):                                             # the merge of two replicas: b's counts into a
        f, g = b.counts(u)
        if f.any() or g.any():
            a.add_counts(u, f, g)
    _assert_same_counts(a, both, db)
    rng = np.random.default_rng(9)
    u = int(np.nonzero(db.is_leaf)[0][-1])
    f0, g0 = a.counts(u)
    f1 = rng.integers(0, 1000, (4, L)).astype(np.uint32); g1 = rng.integers(0, 1000, L).astype(np.uint32)
    a.add_counts(u, f1, g1); a.add_counts(u, f1, g1)
    f2, g2 = a.counts(u)
    assert np.array_equal(f2, f0 + 2 * f1) and np.array_equal(g2, g0 + 2 * g1)
    for bad in (-1, db.n_nodes):
        with pytest.raises(E.EngineError, match="node"):
            a.add_counts(bad, f1, g1)
    with pytest.raises(E.EngineError, match="freq must be"):
        a.add_counts(u, f1[:, :-1], g1)
    assert len(a.infer([u], 2.0)[0]) == L
    a.close(); b.close(); both.close()


# ------------------------------------------------------------------------------------------------ GPU, end to end
def _write_fasta(path, seqs, tag="r"):
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">%s%d\n%s\n" % (tag, i, s))


def _identities(db, rec):
    """(alignIdentity, hmmIdentity) of one record of an assignment file, as hu_tsv_reader.h computes them"""
    match = np.zeros(db.cs_len, bool); match[np.asarray(db.hmm.p2cs[1:]) - 1] = True
    lo, hi = C.c_atol(rec["CS_start"]) - 1, C.c_atol(rec["CS_end"]) - 1
    sym = np.isin(np.frombuffer(rec["alignment"].encode("latin1"), np.uint8)[lo:hi + 1], SYMBOLS)
    m = match[lo:hi + 1]
    return float(sym.sum()) / (hi - lo + 1), float((sym & m).sum()) / float(m.sum())


def _thresholds(db, text):
    """the four filters from a plain run's assignment file: each cuts about a twentieth of the placed reads, --otu-q as Q_taxon is printed"""
    recs = [r for r in C.scan(text)[1] if C.c_atol(r["taxon_id"]) >= 0]
    k = len(recs) // 20
    q = sorted(recs, key=lambda r: C.c_atof(r["Q_taxon"]))[k]["Q_taxon"]
    ids = [_identities(db, r) for r in recs]
    aln, hmm = sorted(a for a, _ in ids)[k], sorted(h for _, h in ids)[k]
    return ["-q", q, "--aln-iden", repr(aln), "--hmm-iden", repr(hmm), "-n", "2"]


def _as_otu_opts(flt):
    ren = {"-q": "--otu-q", "--aln-iden": "--otu-aln-iden", "--hmm-iden": "--otu-hmm-iden", "-n": "--otu-min-reads"}
    return [ren.get(x, x) for x in flt]


def _summarise(pre, tsv, flt, out_dir, tag):
    """hmmufotu-amd-sum and hmmufotu-amd-otu-cs on an assignment file: (table lines from the second on, FASTA bytes)"""
    tab, fa = os.path.join(out_dir, tag + ".sum.otu"), os.path.join(out_dir, tag + ".sum.fa")
    p = _run([_bin("hmmufotu-amd-sum"), pre, tsv, "-o", tab] + flt)
    assert p.returncode == 0, p.stderr
    p = _run([_bin("hmmufotu-amd-otu-cs"), pre, tsv, "-c", fa] + flt)
    assert p.returncode == 0, p.stderr
    return open(tab).read().split("\n")[1:], open(fa, "rb").read()


def _table_and_fasta(tab, fa):
    lines = open(tab).read().split("\n")
    assert lines[0].startswith("# HmmUFOtu v1.5.1 OTU table generated by ") and lines[0].endswith("hmmufotu-amd")
    return lines[1:], open(fa, "rb").read()


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """300 single-end reads on the 70_otus database, a plain run for the thresholds, then THE run: -o run.tsv with the table and the FASTA
    beside it, and the two summary programs on run.tsv"""
    from hmmufotu_amd import engine as E, synth
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    d = str(tmp_path_factory.mktemp("run_summary"))
    db = synth.make_db_70otus("JC69")
    pre = os.path.join(d, "otus70")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    rng = np.random.default_rng(5)
    reads = synth.simulate_reads(db, 300, 150, rng, mean_cols=500, sd_cols=30)
    fa = os.path.join(d, "reads.fasta")
    _write_fasta(fa, [r.seq for r in reads])
    exe = _bin("hmmufotu-amd")
    p = _run([exe, pre, fa, "-s", "1"])
    assert p.returncode == 0, p.stderr
    flt = _thresholds(db, p.stdout)
    tsv, tab, cs = os.path.join(d, "run.tsv"), os.path.join(d, "a.otu"), os.path.join(d, "a.fa")
    common = [exe, pre, fa, "-s", "1"]
    opts = ["--otu-table", tab, "--otu-cs", cs, "--sample", tsv] + _as_otu_opts(flt)
    p = _run(common + ["--batch", "64", "--inflight", "2", "-o", tsv, "-v"] + opts)
    assert p.returncode == 0, p.stderr
    assert open(tsv).read().split("\n")[2:] == _run([exe, pre, fa, "-s", "1"]).stdout.split("\n")[2:]          # the assignment file is the plain run's
    want = _summarise(pre, tsv, flt, d, "run")
    return dict(db=db, d=d, pre=pre, fa=fa, exe=exe, flt=flt, tsv=tsv, common=common, opts=opts, got=_table_and_fasta(tab, cs), want=want, verbose=p.stderr)


@pytest.mark.gpu
def test_one_run_writes_what_the_summary_programs_write(e2e):
    db, flt = e2e["db"], e2e["flt"]
    (tab, fasta), (wtab, wfasta) = e2e["got"], e2e["want"]
    assert tab == wtab
    assert fasta == wfasta
    # the inputs are not degenerate: most reads count, each kind of rejection happens, the boundary of --otu-q is met, an OTU is dropped
    recs = C.scan(open(e2e["tsv"]).read())[1]
    q, aln, hmm = C.c_atof(flt[1]), float(flt[3]), float(flt[5])
    placed = [r for r in recs if C.c_atol(r["taxon_id"]) >= 0]
    by_q = [r for r in placed if not C.c_atof(r["Q_taxon"]) >= q]
    ids = [_identities(db, r) for r in placed]
    by_aln, by_hmm = [a for a, _ in ids if not a >= aln], [h for _, h in ids if not h >= hmm]
    acc = [r for r, (a, h) in zip(placed, ids) if C.c_atof(r["Q_taxon"]) >= q and a >= aln and h >= hmm]
    print("records %d, placed %d, accepted %d; rejected by -q %d, --aln-iden %d, --hmm-iden %d" % (len(recs), len(placed), len(acc), len(by_q), len(by_aln), len(by_hmm)))
    assert len(acc) >= 150 and len(placed) - len(acc) >= 10 and by_q and by_aln and by_hmm
    assert any(r["Q_taxon"] == flt[1] for r in acc)                           # a read sits exactly on the --otu-q threshold and counts
    counts = np.bincount([C.c_atol(r["taxon_id"]) for r in acc])
    rows = [l.split("\t") for l in tab[1:] if l]
    assert tab[0] == "otuID\t%s\ttaxonomy" % e2e["tsv"]
    assert [int(t[0]) for t in rows] == [u for u in np.nonzero(counts >= 2)[0]] and [int(t[1]) for t in rows] == [counts[int(t[0])] for t in rows]
    assert (counts == 1).any(), "no OTU is dropped by --otu-min-reads"
    assert fasta.count(b">") == len(rows) > 3
    m = re.search(r"summary: \S+ busy seconds .* (\d+) reads counted in (\d+) OTUs", e2e["verbose"])
    assert m and int(m.group(1)) == len(acc) and int(m.group(2)) == len(rows), e2e["verbose"]
    # the table feeds hmmufotu-amd-merge unchanged: merged with the table of hmmufotu-amd-sum it gives what that table gives with itself
    d = e2e["d"]
    merged = []
    for first in ("a.otu", "run.sum.otu"):
        out = os.path.join(d, "merged_" + first)
        p = _run([_bin("hmmufotu-amd-merge"), os.path.join(d, first), os.path.join(d, "run.sum.otu"), "-o", out])
        assert p.returncode == 0, p.stderr
        merged.append(open(out).read().split("\n")[1:])
    assert merged[0] == merged[1] and len(merged[0]) == len(tab)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["no-tsv", "one-batch", "two-replicas", "cs-alone"])
def test_the_summary_does_not_depend_on_how_the_run_is_cut(e2e, how):
    d = e2e["d"]
    tab, cs = os.path.join(d, how + ".otu"), os.path.join(d, how + ".fa")
    opts = ["--otu-table", tab, "--otu-cs", cs, "--sample", e2e["tsv"]] + _as_otu_opts(e2e["flt"])
    env = dict(os.environ)
    if how == "no-tsv":
        args = ["--batch", "64", "--inflight", "2", "--no-tsv"] + opts
    elif how == "one-batch":
        args = ["--batch", "300", "--inflight", "1", "--no-tsv"] + opts
    elif how == "two-replicas":
        args = ["--batch", "64", "--inflight", "2", "--gpus", "2", "--no-tsv"] + opts
        env["HU_CLI_SHARE_GPU"] = "1"
    else:                                                                     # --otu-cs may be given without --otu-table
        args = ["--batch", "64", "--inflight", "2", "--no-tsv"] + opts[2:]
    before = set(os.listdir(d))
    p = _run(e2e["common"] + args, env=env)
    assert p.returncode == 0, p.stderr
    assert p.stdout == "", "--no-tsv writes no assignment line"
    new = set(os.listdir(d)) - before
    assert new == ({how + ".fa"} if how == "cs-alone" else {how + ".otu", how + ".fa"}), new
    if how != "cs-alone":
        assert _table_and_fasta(tab, cs)[0] == e2e["want"][0]
    assert open(cs, "rb").read() == e2e["want"][1]


def _chimeras(db, rng, n):
    """reads spliced from two simulated reads of the same amplicon: the first half of one, the second half of the other"""
    from hmmufotu_amd import synth
    out = []
    while len(out) < n:
        a, b = synth.simulate_reads(db, 2, 200, rng, amplicon_start=300, amplicon_cols=700, jitter=0)
        cut = (a.cols[0] + a.cols[-1]) // 2
        s = a.seq[:int((a.cols < cut).sum())] + b.seq[int((b.cols < cut).sum()):]
        if len(s) >= 100:
            out.append(s)
    return out


@pytest.mark.gpu
def test_with_the_chimera_check_the_flagged_reads_do_not_count(e2e):
    from hmmufotu_amd import synth
    db, d, pre, flt = e2e["db"], e2e["d"], e2e["pre"], e2e["flt"]
    rng = np.random.default_rng(17)
    seqs = [r.seq for r in synth.simulate_reads(db, 120, 200, rng, amplicon_start=300, amplicon_cols=700, jitter=0)] + _chimeras(db, rng, 40)
    fa = os.path.join(d, "chi.fasta")
    _write_fasta(fa, seqs, "c")
    tsv, tab, cs = os.path.join(d, "chi.tsv"), os.path.join(d, "chi.otu"), os.path.join(d, "chi.fa")
    # --fix-root-loglik: with the reference's constant root log-likelihood every log-odds is 0 and no read is ever flagged
    p = _run([e2e["exe"], pre, fa, "-s", "1", "-C", "--fix-root-loglik", "-v", "--batch", "64", "--inflight", "2", "-o", tsv, "--otu-table", tab, "--otu-cs", cs] + _as_otu_opts(flt))
    assert p.returncode == 0, p.stderr
    m = re.search(r"(\d+) reads processed, (\d+) assigned, (\d+) flagged as chimera", p.stderr)
    assert m and int(m.group(1)) == 160, p.stderr
    print("-C: %s of 160 reads flagged" % m.group(3))
    assert int(m.group(3)) >= 1 and int(m.group(2)) + int(m.group(3)) <= 160
    got, want = _table_and_fasta(tab, cs), _summarise(pre, tsv, flt, d, "chi")
    assert got[0][0] == "otuID\t%s\ttaxonomy" % tsv                          # the default sample name: the -o file
    assert got[0] == want[0] and got[1] == want[1] and len(got[0]) > 3


@pytest.mark.gpu
def test_paired_end_run(e2e):
    from hmmufotu_amd import synth
    db, d, pre = e2e["db"], e2e["d"], e2e["pre"]
    rng = np.random.default_rng(23)
    ins = synth.simulate_reads(db, 100, 100000, rng, amplicon_start=300, amplicon_cols=300, jitter=20)          # ~260 bases: the mates of 150 overlap
    fw, mt = zip(*[synth.split_pair(r, 150) for r in ins])
    f1, f2 = os.path.join(d, "pe_1.fasta"), os.path.join(d, "pe_2.fasta")
    _write_fasta(f1, [r.seq for r in fw], "p"); _write_fasta(f2, [synth.revcom(r.seq) for r in mt], "p")
    tsv, tab, cs = os.path.join(d, "pe.tsv"), os.path.join(d, "pe.otu"), os.path.join(d, "pe.fa")
    p = _run([e2e["exe"], pre, f1, f2, "-s", "1"])                          # the filters of a paired run from its own plain run, as for the single reads
    assert p.returncode == 0, p.stderr
    flt = _thresholds(db, p.stdout)
    p = _run([e2e["exe"], pre, f1, f2, "-s", "1", "--batch", "64", "--inflight", "2", "-v", "-o", tsv, "--otu-table", tab, "--otu-cs", cs] + _as_otu_opts(flt))
    assert p.returncode == 0, p.stderr
    got, want = _table_and_fasta(tab, cs), _summarise(pre, tsv, flt, d, "pe")
    assert got[0] == want[0] and got[1] == want[1]
    # at least half the pairs count, as of the single reads; the table holds those of them whose OTU has a second read
    m = re.search(r"(\d+) reads counted in (\d+) OTUs", p.stderr)
    in_table = sum(int(l.split("\t")[1]) for l in got[0][1:] if l)
    print("paired: %s of 100 pairs counted, %d of them in the %s OTUs of the table" % (m.group(1), in_table, m.group(2)))
    assert 100 >= int(m.group(1)) >= 50 and int(m.group(1)) >= in_table >= 2 * int(m.group(2)) > 0
