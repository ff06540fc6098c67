"""The tail of the pair scan (k_seed_pdist2 behind its quad loop): the tile's listed inserts walked slot by slot into the lane's own
counters, slot reads and pivots held in lanes, one pack per pair and the level-0 stopper masks of a tile's sixteen slots leaving in one
store per wave.  Reads are given as codes (hu_batch_set_aligned), so every case below decides its tile, its slot and its list; the
expected (d, N) of every (read, node) come from numpy alone, over the region's columns of the database's sequences and the read's codes.

The tree has 5,198 places: more than the device sort holds in LDS with either pair width, so level 0 is a streaming level and the
scan's `L0 = true` instances write the masks the sort starts from.  A wrong mask word, lane or row shows as a difference between the
sort on those masks and the two sorts that do not read them."""
import copy
import re

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
    """database: 5,199 nodes (21 blocks of 256, the last one partial), K = 200 profile columns (two quads) + 100 others, of which the
    last 44 sit at list positions (>= 256); about half of the leaves get a base at each of those, 8 % of the leaves lose their first or
    last 10 - 36 columns.  33 reads in three tiles (16 + 16 + 1); tile 1 lists more than 128 inserts."""
    db0 = get_db(2600, 300, "JC69", dg_k=0, seed=11, n_match=200)
    db = copy.copy(db0)
    rng = np.random.default_rng(8)
    seq = db0.seq.copy()
    K, L = db.hmm.K, db.cs_len
    assert K == 200 and L == 300 and db.n_nodes == 5199
    prof = np.asarray(db.hmm.p2cs[1:K + 1], np.int64) - 1
    rest = np.setdiff1d(np.arange(L), prof)
    QM = (K + 127) // 128
    planes_rest, list_cols = rest[:QM * 128 - K], rest[QM * 128 - K:]        # non-profile columns inside the last profile quad / at list positions
    assert len(list_cols) == 44 and list_cols.min() > 150
    leaves = np.flatnonzero(db.is_leaf)
    for c in list_cols:          # leaves at an insert column: a base for about half of them, a gap for the others (inner nodes all have a base)
        some = leaves[rng.random(len(leaves)) < 0.5]
        seq[some, c] = rng.integers(0, 4, len(some))
    cut_front = []
    for i in rng.choice(leaves, size=len(leaves) * 8 // 100, replace=False):
        cut = int(rng.integers(10, 37))
        if rng.random() < 0.5: seq[i, :cut] = -2; cut_front.append(i)
        else: seq[i, L - cut:] = -2
    db.seq = seq
    codes, start, end, what, n_ins = [], [], [], [], []

    def read(s, e, name, ins=(), ins_code=None, extra=()):
        """bases on the profile columns of [s, e], on the columns `extra` and on the list columns `ins` (codes `ins_code`, or random)"""
        cols = np.unique(np.concatenate([prof[(prof >= s) & (prof <= e)], np.asarray(extra, np.int64), np.asarray(ins, np.int64)])).astype(np.int64)
        assert cols.min() == s and cols.max() <= e
        src = seq[rng.choice(leaves)]
        cd = np.full(L, -2, np.int8)
        cd[cols] = np.where(src[cols] >= 0, src[cols], rng.integers(0, 4, len(cols)))
        flip = cols[rng.random(len(cols)) < 0.1]
        cd[flip] = (cd[flip] + 1 + rng.integers(0, 3, len(flip))) % 4
        if ins_code is not None:
            cd[np.asarray(ins, np.int64)] = ins_code
        codes.append(cd); start.append(int(cols.min())); end.append(int(cols.max())); what.append(name); n_ins.append(len(ins))

    def pick(count):
        return np.sort(rng.choice(list_cols, size=count, replace=False))

    def last(count, e):
        """the last `count` list columns up to column e"""
        return [int(c) for c in list_cols[list_cols <= e][len(list_cols[list_cols <= e]) - count:]]

    p = [int(c) for c in prof]          # region starts are profile columns, all different: the slot of every read is decided
    # tile 0
    read(0, 299, "wide: more than 255 bases, three inserts (slot 0)", pick(3), extra=planes_rest)
    read(p[1], 230, "one insert", last(1, 225))
    read(p[2], p[5], "no column in common with the leaves cut at the front")
    read(p[3], 299, "two inserts", pick(2))
    read(p[4], 260, "no insert, between two reads with some")
    read(p[5], 299, "exactly HU_MAX_INS inserts", pick(MAX_INS))
    read(p[6], 299, "HU_MAX_INS + 6 inserts: they stay in the planes", pick(MAX_INS + 6))
    shared = int(list_cols[10])
    read(p[7], 280, "shared insert column, code 0", [shared], ins_code=0)
    read(p[8], 280, "shared insert column, code 3", [shared, int(list_cols[12])], ins_code=3)
    for i in range(9, 15):
        read(p[i], 200 + 6 * i, "ordinary", last(i % 3, 200 + 6 * i))
    read(p[15], 299, "one insert (slot 15)", pick(1))
    # tile 1
    read(p[30], 180, "no insert (slot 0)")
    for i in range(31, 45):
        e = 150 + 10 * (i - 31)
        if 36 <= i <= 42:          # seven full lists in slots 6 - 12: the tile's list passes 64 entries inside slot 8's run and 128 inside slot 11's
            read(p[i], 299, "exactly HU_MAX_INS inserts, in a tile that lists more than 128", pick(MAX_INS))
        else:
            read(p[i], e, "ordinary", last((i - 31) % 4 if e >= 230 else 0, e))
    read(p[45], 299, "two inserts (slot 15)", pick(2))
    # tile 2: one read, fifteen empty slots
    read(p[90], 299, "alone in its tile, one insert", pick(1))
    assert len(codes) == 33
    codes = np.stack(codes); start = np.asarray(start, np.int32); end = np.asarray(end, np.int32)
    order = np.argsort(start, kind="stable")
    assert (np.diff(start[order]) > 0).all() and (order == np.arange(33)).all()          # read r sits in slot r % 16 of tile r // 16
    slot_ins = np.asarray(n_ins)          # inserts on slot 0 and slot 15 of a tile, on the read that is alone in its tile, and on a read between two without any
    assert slot_ins[0] and slot_ins[15] and slot_ins[31] and slot_ins[32] and not slot_ins[16]
    assert slot_ins[3] and not slot_ins[4] and slot_ins[5]
    assert {0, 1, 2, MAX_INS, MAX_INS + 6} <= set(n_ins)
    # entries a tile lists (a read beyond HU_MAX_INS lists none): the scan holds 64 of them in its lanes at a time.  Tile 0 stays below 64; in tile 1
    # entries 63 | 64 and 127 | 128 fall inside one slot's run, and slots with entries follow the second reload
    listed = np.where(slot_ins <= MAX_INS, slot_ins, 0)
    ends1 = np.cumsum(listed[16:32])
    assert 0 < listed[:16].sum() < 64 and listed[32:].sum() == 1 and ends1[-1] > 128 + MAX_INS
    assert any(a < 63 and b > 64 for a, b in zip(ends1[:-1], ends1[1:])) and any(a < 127 and b > 128 for a, b in zip(ends1[:-1], ends1[1:]))
    assert codes[7, shared] == 0 and codes[8, shared] == 3
    # the narrow version of the batch: the wide read without the non-profile columns of the planes (but its first column, so its slot stays)
    narrow = codes.copy()
    narrow[0, planes_rest[1:]] = -2
    assert (codes[0] >= 0).sum() > 255 and ((narrow >= 0).sum(1) <= 255).all() and (codes[1:] >= 0).sum(1).max() <= 255

    def expect(cds):
        want = []
        for cd, s, e in zip(cds, start, end):
            cols = np.flatnonzero((cd >= 0) & (np.arange(L) >= s) & (np.arange(L) <= e))
            ok = seq[:, cols] >= 0
            want.append((((seq[:, cols] != cd[cols][None, :]) & ok).sum(1), ok.sum(1)))
        return want
    want, want_narrow = expect(codes), expect(narrow)
    # what the cases promise
    for r in range(33):          # at every listed insert some leaves have the read's base, some another, some a gap
        if 0 < n_ins[r] <= MAX_INS:
            for c in np.flatnonzero((codes[r] >= 0) & np.isin(np.arange(L), list_cols)):
                col = seq[leaves, c]
                assert (col == codes[r, c]).any() and ((col >= 0) & (col != codes[r, c])).any() and (col < 0).any(), (r, c)
    zero_reads = [r for r in range(33) if (want[r][1] == 0).any()]
    assert zero_reads == [2] and (want[2][1][cut_front] == 0).all() and len(cut_front) > 0
    assert any((N < N.max()).any() for _, N in want)          # the gaps of the leaves show in N
    return db, codes, narrow, start, end, what, want, want_narrow


@pytest.fixture(scope="module")
def case():
    return make_case()


RUNS = [("reference order, 16-bit pairs", dict(seed_order=1), {}),
        ("reference order, 32-bit pairs", dict(seed_order=1), dict(pairs32=1)),
        ("(dist, node id) order, pair matrix", dict(seed_order=0), dict(scan_pairs=1)),
        ("(dist, node id) order, distance-only scan", dict(seed_order=0, max_nseed=2), {})]
MODES = [("device sort on the scan's masks", {}), ("device sort counting level 0 itself", dict(ref_nofuse=1)), ("host restatement", dict(refsort_host=1))]


@pytest.mark.parametrize("run", range(len(RUNS)), ids=[r[0] for r in RUNS])
def test_scan_tail(case, run, capfd):
    """B.pdist of every read against numpy; in the reference's order the seeds of the device sort on the scan's masks, of the device sort that
    counts level 0 itself and of the host restatement are the same, the first one's log names the scan's masks, and both device sorts leave
    the read with a compared-site count of zero to the host path"""
    E = _engine()
    db, codes, narrow, start, end, what, want, want_narrow = case
    _, okw, knobs = RUNS[run]
    if "pairs32" not in knobs:          # the wide read is for the 32-bit run only: one read beyond 255 bases and the batch takes 32-bit pairs
        codes, want = narrow, want_narrow
    opts = E.default_opts(**okw)
    D = E.Database.from_synth(db)
    lists, stats = [], []
    for mi, (mode, mk) in enumerate(MODES if okw["seed_order"] == 1 else MODES[:1]):
        B = E.Batch(D, len(codes))
        for k, v in dict(knobs, trace=1, **mk).items():
            B.set_knob(k, v)
        B.set_aligned(codes, start, end)
        capfd.readouterr()
        B.get_seed(opts)
        err = capfd.readouterr().err
        if mi == 0:
            for r in range(len(codes)):
                d, N = B.pdist(r)          # after the distance-only scan: from the planes, and the scan's row is checked against them inside
                assert np.array_equal(d, want[r][0]) and np.array_equal(N, want[r][1]), (r, what[r])
        if okw["seed_order"] == 1:
            if "refsort_host" in mk:
                assert "k_seed_refsort" not in err
            else:
                m = re.search(r"k_seed_refsort: 33 reads.* %s pairs.* (\d+) reads left to the host" % ("32-bit" if "pairs32" in knobs else "16-bit"), err)
                assert m, err
                assert ("level 0 from the scan" in err) == (mi == 0), err
                stats.append((B.refsort_stats(), int(m.group(1))))
            cnt, ids, sd, sN = B.seeds()
            lists.append((cnt.copy(), ids.copy(), sd.copy(), sN.copy()))
        B.close()
    if lists:
        # the one read without a column in common with some leaf, and no other, goes to the host path, whichever device sort found it (the host
        # restatement keeps no such count: it is held to the same seeds)
        assert stats[0] == stats[1] and stats[0][0][0] == stats[0][1] == 1 and stats[0][0][1] is False, stats
        cnt = lists[0][0]
        live = np.arange(lists[0][1].shape[1])[None, :] < cnt[:, None]
        assert (cnt > 0).all()
        for (mode, _), (c, i, d, n) in zip(MODES[1:], lists[1:]):
            assert np.array_equal(cnt, c), mode
            assert np.array_equal(lists[0][1][live], i[live]) and np.array_equal(lists[0][2][live], d[live]) and np.array_equal(lists[0][3][live], n[live]), mode
    D.close()
