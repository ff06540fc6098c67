"""The seed scans run, of every quad of 128 scan positions that a tile of sixteen reads lists, only the 32-site words in which a read
of the tile has a base (k_tile_lists: a word mask per listed quad, and the planes of those words word by word).  Reads are given as
codes (hu_batch_set_aligned), so their columns are exact and every case below decides the mask of its tile; the expected (d, N) of
every (read, node) come from numpy alone, over the region's columns of the database's sequences and the read's codes."""
import copy

import numpy as np
import pytest

from conftest import get_db

pytestmark = pytest.mark.gpu

MAX_INS = 24          # HU_MAX_INS: more bases than this on non-profile positions and they stay in the read's planes


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


def make_case():
    """database: 1,099 nodes (five blocks of 256, the last one partial), K = 330 profile columns (three quads, the last one partly
    filled) + 270 others; 8 % of the leaves without their first or last 10 - 36 columns.  37 reads in three tiles (16 + 16 + 5)."""
    db0 = get_db(550, 600, "JC69", dg_k=0, seed=23, n_match=330)
    db = copy.copy(db0)
    rng = np.random.default_rng(5)
    seq = db0.seq.copy()
    leaves = np.flatnonzero(db.is_leaf)
    for i in rng.choice(leaves, size=len(leaves) * 8 // 100, replace=False):
        cut = int(rng.integers(10, 37))
        if rng.random() < 0.5: seq[i, :cut] = -2
        else: seq[i, db.cs_len - cut:] = -2
    db.seq = seq
    K, L = db.hmm.K, db.cs_len
    assert K == 330 and db.n_nodes == 1099
    prof = np.asarray(db.hmm.p2cs[1:K + 1], np.int64) - 1
    rest = np.setdiff1d(np.arange(L), prof)
    pos_col = np.concatenate([prof, rest])          # scan position -> column: the profile columns first (HuDbDev::posCol)
    QM = (K + 127) // 128
    codes, start, end, what = [], [], [], []

    def read(positions, name, extra_cols=()):
        cols = np.unique(np.concatenate([pos_col[np.asarray(positions, np.int64)], np.asarray(extra_cols, np.int64)])).astype(np.int64)
        src = seq[rng.choice(leaves)]
        cd = np.full(L, -2, np.int8)
        cd[cols] = np.where(src[cols] >= 0, src[cols], rng.integers(0, 4, len(cols)))
        flip = cols[rng.random(len(cols)) < 0.1]
        cd[flip] = (cd[flip] + 1 + rng.integers(0, 3, len(flip))) % 4
        codes.append(cd); start.append(int(cols.min())); end.append(int(cols.max())); what.append(name)

    def inserts(lo_pos, hi_pos, count):
        """`count` non-profile columns between two profile positions, all of them at list positions (>= QM * 128)"""
        c = rest[(rest > pos_col[lo_pos]) & (rest < pos_col[hi_pos]) & (np.arange(len(rest)) + K >= QM * 128)]
        assert len(c) >= count
        return rng.choice(c, size=count, replace=False)

    # tile 0: starts at positions below 128
    read(range(40, 61), "one word")                                   # word 1 of quad 0
    read([31, 32], "positions 31 and 32")                             # words 0 and 1
    read([127, 128], "positions 127 and 128")                         # word 3 of quad 0, word 0 of quad 1
    read(range(100, 301), "three quads")
    for i in range(12):
        a = int(rng.integers(0, 100)); read(range(a, a + int(rng.integers(60, 120))), "ordinary")
    # tile 1: words 0 and 2 of quad 1 and nothing in its words 1 and 3
    for i in range(16):
        w0 = list(range(128 + i % 7, 160 - i % 5)); w2 = list(range(192 + i % 6, 224 - i % 3))
        read(w0 if i % 3 == 0 else w2 if i % 3 == 1 else w0 + w2, "words 0 and 2")
    # tile 2: starts beyond position 224; the read without a region sorts last and shares the tile
    read(range(270, 321), "last profile quad")
    read(range(230, 301), "listed inserts", inserts(230, 300, 6))
    read(range(240, 311), "inserts in the planes", inserts(240, 310, MAX_INS + 6))
    read(range(226, 330), "ordinary")
    read(range(50, 90), "empty region"); start[-1], end[-1] = 300, 200
    assert len(codes) == 37
    codes = np.stack(codes); start = np.asarray(start, np.int32); end = np.asarray(end, np.int32)
    # the tiling the cases rely on: sixteen reads per tile in order of region start, reads without a region last
    order = np.argsort(np.where(end >= start, start.astype(np.int64), 1 << 40), kind="stable")
    assert (order[:16] < 16).all() and ((order[16:32] >= 16) & (order[16:32] < 32)).all() and order[-1] == 36
    # expected (d, N) of every (read, node)
    want = []
    for cd, s, e in zip(codes, start, end):
        cols = np.flatnonzero((cd >= 0) & (np.arange(L) >= s) & (np.arange(L) <= e))
        ok = seq[:, cols] >= 0
        want.append((((seq[:, cols] != cd[cols][None, :]) & ok).sum(1), ok.sum(1)))
    n_bases = np.array([len(np.flatnonzero((cd >= 0) & (np.arange(L) >= s) & (np.arange(L) <= e))) for cd, s, e in zip(codes, start, end)])
    assert any((N < nb).any() and (N == nb).any() for (_, N), nb in zip(want, n_bases))      # the gaps of the leaves show in N
    return db, codes, start, end, what, want


@pytest.fixture(scope="module")
def case():
    return make_case()


RUNS = [("reference order, 16-bit pairs", dict(seed_order=1), {}),
        ("reference order, 32-bit pairs", dict(seed_order=1), dict(pairs32=1)),
        ("(dist, node id) order, pair matrix", dict(seed_order=0), dict(scan_pairs=1)),
        ("(dist, node id) order, distance-only scan", dict(seed_order=0, max_nseed=2), {})]


@pytest.mark.parametrize("run", range(len(RUNS)), ids=[r[0] for r in RUNS])
def test_scan_words(case, run):
    E = _engine()
    db, codes, start, end, what, want = case
    _, okw, knobs = RUNS[run]
    opts = E.default_opts(**okw)
    D = E.Database.from_synth(db)
    B = E.Batch(D, len(codes))
    for k, v in knobs.items():
        B.set_knob(k, v)
    B.set_aligned(codes, start, end)
    B.get_seed(opts)
    for r in range(len(codes)):
        d, N = B.pdist(r)          # after the distance-only scan: from the planes, and the scan's row is checked against them inside
        assert np.array_equal(d, want[r][0]) and np.array_equal(N, want[r][1]), (r, what[r])
    if okw["seed_order"] == 1:
        cnt, ids, sd, sN = B.seeds()
        B.set_knob("refsort_host", 1); B.get_seed(opts)
        hcnt, hids, hd, hN = B.seeds()
        assert np.array_equal(cnt, hcnt)
        live = np.arange(ids.shape[1])[None, :] < cnt[:, None]
        assert np.array_equal(ids[live], hids[live]) and np.array_equal(sd[live], hd[live]) and np.array_equal(sN[live], hN[live])
    B.close(); D.close()
