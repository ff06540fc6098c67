"""The align stage at the read lengths where hu_align_batch changes its fill kernel, or where a fill changes its own lane layout.

hu_align_batch picks one Viterbi fill per batch from the batch's longest read (plan_viterbi, hu_engine.hip) and says which under the
`trace` knob.  Every batch here is compared with the oracle by test_gpu_parity._check_alignments (status, the six coordinates, the cost
bit for bit, trace string, aligned row, used_full, digitised codes and region ends) AND asserts the fill named in that trace line
against the tables written out below.  The tables are not computed from the engine's constants on purpose: moving a threshold must
fail here until someone edits them.

No read of any batch is excused: oracle `ok` and engine status 1 for every one (asserted by _check_alignments).
"""
import re

import numpy as np
import pytest

from conftest import get_db, oracle_objects, sim_reads
from test_gpu_parity import LONG_DB, _check_alignments, _engine

pytestmark = pytest.mark.gpu

MODES = (0, 2)

# rows per lane 4 -> 8 (256 | 257), wave -> workgroup decision bytes (512 | 513), 9 * (L + 1) * 8 bytes of LDS crossing 64 KB (909 | 910:
# hipFuncSetAttribute decides) and 96 KB (1364 | 1365: the HBM-staged kernel takes over); partly filled last lanes on both sides of each
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 252, 253, 254, 255, 256, 257, 258, 259, 260, 263, 264, 265, 505, 509, 510, 511, 512, 513, 514,
           909, 910, 1363, 1364, 1365, 1366)


def _expected_fill(max_len):
    """the default fill by the longest read of a batch"""
    if max_len <= 256:
        return "k_viterbi_wave<4>"
    if max_len <= 512:
        return "k_viterbi_wave<8>"
    if max_len <= 1364:
        return "k_viterbi_dec"
    return "k_viterbi"


def _expected_lds(fill, max_len, halo):
    """dynamic LDS of the fill: three rows of min(halo, 512) doubles for the wave kernels, nine diagonals of max_len + 1 doubles for the
    workgroup kernels (plus the halo rows and 32 bytes per thread for the row-per-thread ones), none for the HBM-staged kernel"""
    diag = 9 * (max_len + 1) * 8
    if fill.startswith("k_viterbi_wave"):
        return 3 * min(halo, 512) * 8
    if fill.startswith("k_viterbi_dec2"):
        return diag + 3 * halo * 8 + 32 * int(fill[15:18])
    return 0 if fill == "k_viterbi" else diag


TRACE_RE = re.compile(r"\[hu\] align: (\d+) sequences, longest (\d+), fill (\S+(?: \d>)?), (\d+) bytes of LDS, (\d+) redone for values, (\d+) by the full-DP fallback")


def _trace(err):
    m = TRACE_RE.findall(err)
    assert len(m) == 1, err[-800:]
    n, longest, fill, lds, values, full = m[0]
    return dict(n=int(n), longest=int(longest), fill=fill, lds=int(lds), values=int(values), full=int(full))


class _Oracle:
    """H.align with its answers kept: the same read comes back in the ragged and the knob batches"""

    def __init__(self, H):
        self.H, self.memo = H, {}

    def align(self, seq, vp):
        key = (seq, np.asarray(vp).tobytes())
        if key not in self.memo:
            self.memo[key] = self.H.align(seq, vp)
        return self.memo[key]


_ORACLES = {}


def _oracle(db, mode):
    key = (id(db), mode)
    if key not in _ORACLES:
        _ORACLES[key] = _Oracle(oracle_objects(db, mode)[1])
    return _ORACLES[key]


def _long_db():
    return get_db(LONG_DB["n_leaves"], LONG_DB["cs_len"], "GTR", dg_k=4, **LONG_DB["db_kw"])


_POOL = {}


def _pool(db, n, read_len, **kw):
    """n simulated reads of (nearly) read_len bases, drawn once per database"""
    key = (id(db), n, read_len, tuple(sorted(kw.items())))
    if key not in _POOL:
        _POOL[key] = sim_reads(db, n, read_len, **kw)[0]
    return _POOL[key]


def _exact(db, src, L, rng):
    """src cut to exactly L bases with the seeds alignSeq would find for the cut read; beyond its own length random bases are appended
    and the 3' seed, which would lie in them, is dropped (as test_reads_longer_than_the_profile does)"""
    from hmmufotu_amd import synth
    if L <= len(src.seq):
        rd = synth.SimRead(src.seq[:L], src.cols[:L], src.node, src.rc, src.cs_start, src.cs_end)
        vp = synth.read_vpaths(db.hmm, rd)
    else:
        rd = synth.SimRead(src.seq + "".join(rng.choice(list("ACGT"), size=L - len(src.seq))), src.cols, src.node, src.rc, src.cs_start, src.cs_end)
        vp = synth.read_vpaths(db.hmm, src)
        vp[1] = 0
    assert len(rd.seq) == L
    return rd, vp.copy()


def _length_reads(L):
    """The reads of the single-length batch of L: two with every seed alignSeq finds (both ends from 100 bases on, the 5' end below), one
    with the 5' seed only, one with none (full DP: its one phase has exactly L rows).  Below 20 bases there are no seeds: one read."""
    db = _long_db()
    pool = _pool(db, 8, 1300)
    rng = np.random.default_rng(1000 + L)
    seqs, vps = [], []
    for k in range(4 if L >= 20 else 1):
        rd, vp = _exact(db, pool[(L + k) % len(pool)], L, rng)
        if L >= 20:
            assert vp[0, 0] > 0 and (L < 100 or L > len(pool[(L + k) % len(pool)].seq) or vp[1, 0] > 0), (L, k, vp)
        else:
            assert not vp.any()
        if k == 2:
            vp[1] = 0
        if k == 3:
            vp[:] = 0
        seqs.append(rd.seq); vps.append(vp)
    return seqs, np.stack(vps)


def _halo(db, vps):
    """columns of the widest phase + 2 as hu_align_batch counts them; the unseeded read's phase spans the whole profile"""
    assert any(not v.any() for v in vps)
    return db.hmm.K + 2


_SINGLE = {}


def _single(E, L, mode, capfd):
    """the single-length batch of L under align_mode `mode`, checked against the oracle and against the fill table; kept for the ragged batches"""
    if (L, mode) not in _SINGLE:
        db = _long_db()
        seqs, vps = _length_reads(L)
        got, err = _check_alignments(E, db, _oracle(db, mode), seqs, vps, opts=E.default_opts(align_mode=mode), knobs=dict(trace=1), capfd=capfd)
        t = _trace(err)
        fill = _expected_fill(L)
        assert (t["n"], t["longest"], t["fill"]) == (len(seqs), L, fill), t
        assert t["lds"] == _expected_lds(fill, L, _halo(db, vps)), t
        assert t["full"] == 0, t                      # the seeded reads align inside their bands; the unseeded one is a full DP from the start
        assert [g["used_full"] for g in got] == [not v.any() for v in vps]
        print("align edges: L=%d mode=%d %s" % (L, mode, t))
        _SINGLE[(L, mode)] = (seqs, vps, got, t)
    return _SINGLE[(L, mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", LENGTHS)
def test_length_matrix(L, mode, capfd):
    """one batch per length, so that L is the batch's longest read and decides the fill"""
    _single(_engine(), L, mode, capfd)


RAGGED = {"wave8": ((1, 20, 40, 64, 150, 256, 257, 400, 512), "k_viterbi_wave<8>"),
          "dec": ((1, 20, 40, 64, 150, 256, 257, 400, 512, 513), "k_viterbi_dec"),
          "dec_lds_above_64k": ((40, 150, 300, 1300), "k_viterbi_dec")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("longest_first", [False, True])
@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_batch(case, longest_first, mode, capfd):
    """One plan for a ragged batch: the longest read decides for all, so short reads run under eight rows per lane, or under the workgroup
    kernel with diagonals of 514 / 1,301 rows.  Every read must come out as in the batch of its own length, field for field."""
    E = _engine()
    db = _long_db()
    lengths, fill = RAGGED[case]
    seqs, vps, want = [], [], []
    for L in (reversed(lengths) if longest_first else lengths):
        s, v, got, _ = _single(E, L, mode, capfd)
        seqs += s; vps += list(v); want += got
    vps = np.stack(vps)
    got, err = _check_alignments(E, db, _oracle(db, mode), seqs, vps, opts=E.default_opts(align_mode=mode), knobs=dict(trace=1), capfd=capfd)
    t = _trace(err)
    assert (t["n"], t["longest"], t["fill"]) == (len(seqs), max(lengths), fill), t
    assert t["lds"] == _expected_lds(fill, max(lengths), _halo(db, vps)) and t["full"] == 0, t
    if case == "dec_lds_above_64k":
        assert t["lds"] == 9 * 1301 * 8 > 64 * 1024
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(seqs[i]))
    print("align edges: ragged %s longest_first=%d mode=%d %s" % (case, longest_first, mode, t))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("read_len", [150, 300])
def test_band_height(read_len, mode, capfd):
    """k_viterbi_wave keeps a seed band of up to 64 rows (one per lane) and hands wider ones to the value-filing redo: seeds of 62 ... 66
    bases at three offsets, on 150-base reads (four rows per lane) and 300-base ones (eight)."""
    E = _engine()
    from hmmufotu_amd import synth
    db = _long_db()
    pool = _pool(db, 8, 1300)
    cs2p = synth.cs2profile(db.hmm)
    rng = np.random.default_rng(7)
    seqs, vps = [], []
    for seed_len in (62, 63, 64, 65, 66):
        for sf in (0, 5, 17):
            rd, _ = _exact(db, pool[len(seqs) % len(pool)], read_len, rng)
            v = synth.seed_vpath(db.hmm, cs2p, rd, sf, seed_len)
            assert v[0] > 0 and v[0] <= v[1] and v[2] == sf + 1 and v[3] - v[2] + 1 == seed_len, v     # a band of exactly seed_len rows
            vp = np.zeros((2, 6), np.int32); vp[0] = v
            seqs.append(rd.seq); vps.append(vp)
    vps = np.stack(vps)
    above = int((vps[:, 0, 3] - vps[:, 0, 2] + 1 > 64).sum())
    assert above == 6
    got, err = _check_alignments(E, db, _oracle(db, mode), seqs, vps, opts=E.default_opts(align_mode=mode), knobs=dict(trace=1), capfd=capfd)
    t = _trace(err)
    assert (t["n"], t["longest"], t["fill"]) == (15, read_len, _expected_fill(read_len)), t
    assert not any(g["used_full"] for g in got) and t["full"] == 0, t
    assert t["values"] >= above, t                     # the rest is what k_viterbi_trace_dec flags on its own
    print("align edges: band height read_len=%d mode=%d: %d bands above 64 rows, %d more flagged by the traceback, %s" % (read_len, mode, above, t["values"] - above, t))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("read_len", [100, 300])
@pytest.mark.parametrize("K", [509, 510, 511, 512])
def test_phase_width(K, read_len, mode, capfd):
    """The wave kernel stages the row above a phase in LDS only while the phase's columns + 2 fit min(halo, 512); wider phases read it
    from the scratch.  A full DP against K = 510 | 511 match states sits on that switch."""
    E = _engine()
    db = get_db(20, 700, "GTR", dg_k=0, n_match=K)
    assert db.hmm.K == K
    pool = _pool(db, 4, 300, cols=580)
    rng = np.random.default_rng(K)
    seqs, vps = [], []
    for k in range(4):
        rd, vp = _exact(db, pool[k], read_len, rng)
        assert vp[0, 0] > 0 and vp[1, 0] > 0, vp
        if k % 2:
            vp[:] = 0
        seqs.append(rd.seq); vps.append(vp)
    vps = np.stack(vps)
    got, err = _check_alignments(E, db, _oracle(db, mode), seqs, vps, opts=E.default_opts(align_mode=mode), knobs=dict(trace=1), capfd=capfd)
    t = _trace(err)
    fill = _expected_fill(read_len)
    assert (t["n"], t["longest"], t["fill"], t["lds"]) == (4, read_len, fill, 3 * min(K + 2, 512) * 8), t
    assert [g["used_full"] for g in got] == [False, True, False, True] and t["full"] == 0, t
    print("align edges: phase width K=%d read_len=%d mode=%d %s" % (K, read_len, mode, t))


def test_pairs_with_mates_in_different_classes(capfd):
    """In a paired batch the longest read is taken over both mates: 250-base reads (four rows per lane on their own) with 300-base mates
    and the reverse all run under k_viterbi_wave<8>, and k_merge_rows joins their rows.  Half of the inserts are shorter than 550 bases,
    so their mates overlap."""
    E = _engine()
    from hmmufotu_amd import synth
    from oracle import oracle_py as O
    db = _long_db()
    H = _oracle(db, 0)
    rng = np.random.default_rng(5)
    ins = synth.simulate_reads(db, 8, 100000, rng, amplicon_start=60, amplicon_cols=600, jitter=20) + \
        synth.simulate_reads(db, 8, 100000, rng, amplicon_start=60, amplicon_cols=1200, jitter=20)
    fw, rv, vf, vr = [], [], [], []
    for k, r in enumerate(ins):
        n = len(r.seq)
        nf, nm = (250, 300) if k % 2 == 0 else (300, 250)
        assert n >= 300
        f = synth.SimRead(r.seq[:nf], r.cols[:nf], r.node, r.rc, r.cs_start, r.cs_end)
        m = synth.SimRead(r.seq[n - nm:], r.cols[n - nm:], r.node, r.rc, r.cs_start, r.cs_end)        # mate after revcom
        assert (len(f.seq), len(m.seq)) == (nf, nm)
        fw.append(f.seq); rv.append(m.seq); vf.append(synth.read_vpaths(db.hmm, f)); vr.append(synth.read_vpaths(db.hmm, m))
    assert sum(len(r.seq) < 550 for r in ins) == 8
    D = E.Database.from_synth(db)
    B = None
    try:
        B = E.Batch(D, len(fw))
        B.set_knob("trace", 1)
        B.set_reads(fw, np.stack(vf), rv, np.stack(vr))
        capfd.readouterr()
        B.align(E.default_opts())
        t = _trace(capfd.readouterr().err)
        assert (t["n"], t["longest"], t["fill"], t["full"]) == (32, 300, "k_viterbi_wave<8>", 0), t
        out = B.alignments(want_align=True)
        for i in range(len(fw)):
            a = H.align(fw[i], vf[i]); b = H.align(rv[i], vr[i])
            assert a["ok"] and b["ok"] and not a["usedFull"] and not b["usedFull"], i
            ia = [a[k] for k in ("seqStart", "seqEnd", "hmmStart", "hmmEnd", "csStart", "csEnd")]
            ib = [b[k] for k in ("seqStart", "seqEnd", "hmmStart", "hmmEnd", "csStart", "csEnd")]
            ok, im, cm, am = O.merge(db.cs_len, ia, a["cost"], a["align"].encode("latin1"), ib, b["cost"], b["align"].encode("latin1"))
            rec = out["recs"][i]
            assert ok and rec["status"] == 1, i
            assert [rec[k] for k in ("seq_start", "seq_end", "hmm_start", "hmm_end", "cs_start", "cs_end")] == list(im[:6]), i
            assert rec["cost"] == cm and out["align"][i] == am.decode("latin1"), i
        print("align edges: pairs %s" % t)
    finally:
        if B is not None:
            B.close()
        D.close()


# the fills only a knob reaches, at the same edges: knob -> (its value, fill by the batch's longest read)
KNOB_FILLS = {
    "viterbi_mode": (2, {255: "k_viterbi_dec2<256>", 256: "k_viterbi_dec2<256>", 257: "k_viterbi_dec2<512>",
                         511: "k_viterbi_dec2<512>", 512: "k_viterbi_dec2<512>", 513: "k_viterbi_dec"}),
    "viterbi_dec1": (1, {L: "k_viterbi_dec" for L in (255, 256, 257, 511, 512, 513)}),
    "viterbi_values": (1, {L: "k_viterbi_lds" for L in (255, 256, 257, 511, 512, 513)}),
    "viterbi_hbm": (1, {L: "k_viterbi" for L in (255, 256, 257, 511, 512, 513)}),
    "viterbi_force_redo": (1, {255: "k_viterbi_wave<4>", 256: "k_viterbi_wave<4>", 257: "k_viterbi_wave<8>",
                               511: "k_viterbi_wave<8>", 512: "k_viterbi_wave<8>", 513: "k_viterbi_dec"}),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [255, 256, 257, 511, 512, 513])
@pytest.mark.parametrize("knob", list(KNOB_FILLS))
def test_knob_fills(knob, L, mode, capfd):
    """the batches of 255 / 256 / 257 and 511 / 512 / 513 bases again on every fill a knob selects: the same answers as the default fill"""
    E = _engine()
    db = _long_db()
    value, fills = KNOB_FILLS[knob]
    seqs, vps, want, _ = _single(E, L, mode, capfd)
    got, err = _check_alignments(E, db, _oracle(db, mode), seqs, vps, opts=E.default_opts(align_mode=mode), knobs={knob: value, "trace": 1}, capfd=capfd)
    t = _trace(err)
    assert (t["n"], t["longest"], t["fill"]) == (len(seqs), L, fills[L]), t
    assert t["lds"] == _expected_lds(fills[L], L, _halo(db, vps)) and t["full"] == 0, t
    if knob == "viterbi_force_redo":
        assert t["values"] == len(seqs), t
    if knob in ("viterbi_values", "viterbi_hbm"):
        assert t["values"] == 0, t                     # these fills file every value themselves: nothing to redo
    assert got == want
    print("align edges: knob %s L=%d mode=%d %s" % (knob, L, mode, t))
