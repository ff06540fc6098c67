"""k_estimate_prod does a slot's uniform arithmetic once per workgroup: one wave (blockIdx.x % NW, the builder) evaluates ratio, the six
exponentials, wnr, the 5 x 4 table and the closing log, the others take the exponentials and the table from LDS behind a barrier.  Which
wave executes an operation changed, no operation did: every (read, seed) slot's ratio, wnr and loglik is, byte for byte, what the commit
before the change gave (tests/golden/estimate_uniform_parent.npz, written there by tests/golden/estimate_uniform_parent_gen.py), and
agrees with the CPU oracle as tests/test_gpu_parity.py asks (ratio and the unweighted wnr exactly, the rest within its 1e-6).

The regions are handed over aligned (hu_batch_set_aligned) on the synthetic tree of tests/test_loads_batched.py.  A launch takes its
kernel from the widest region in it, so the reads go in one batch per width class, each run unweighted and weighted:

  class     instance     widths in the batch
  <= 512    <2, 4>       512, 257 = 256 + 1, 65, 40, 40 (the exact copy), none
  <= 1,024  <4, 4>       1,024, 769 = 256 x 3 + 1, 65, 40, 40, none
  <= 1,536  <6, 4, 4>    1,536, 1,281 = 256 x 5 + 1, 65, 40, 40, none
  <= 2,048  <8, 4>       2,048, 1,793 = 256 x 7 + 1, 65, 40, 40, none
  <= 3,072  <6, 8, 2>    3,072, 2,561 = 512 x 5 + 1, 65, 40, 40, none

40 columns: only wave 0 holds a site, the other waves contribute the neutral product and still meet every barrier.  65 columns: wave 1
holds one site.  The exact copy is a read of 40 bases copied without substitutions from an inner node, in conserved columns: every node
it is seeded on has the same 40 bases (distance 0), no inferred state differs, the unweighted wnr is exactly 0 and the table build takes
its wnr == 0 branch.  The last read has an empty region and so no
seed: its workgroups, like those of the slots beyond a read's 16 seeds (HU_MAX_SEEDS is 64), return ahead of every barrier.  Every
launch holds at least 2 NW slots with a seed, so each wave index is the builder at least once.  A batch of 256 narrow reads with two wide
ones takes the width-split second pass."""
import os

import numpy as np
import pytest

from conftest import get_db, oracle_objects

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimate_uniform_parent.npz")
MAX_NSEED = 16
GAP = -2
# class maximum -> (instance, waves per workgroup, (columns, bases) of its reads)
CLASSES = {
    512: ("k_estimate_prod<2,4>", 4, [(512, 200), (257, 120), (65, 50), (40, 40)]),
    1024: ("k_estimate_prod<4,4>", 4, [(1024, 256), (769, 250), (65, 50), (40, 40)]),
    1536: ("k_estimate_prod<6,4,4>", 4, [(1536, 256), (1281, 200), (65, 50), (40, 40)]),
    2048: ("k_estimate_prod<8,4>", 4, [(2048, 450), (1793, 400), (65, 50), (40, 30)]),
    3072: ("k_estimate_prod<6,8,2>", 8, [(3072, 500), (2561, 480), (65, 50), (40, 30)]),
}
EXACT_START, EXACT_COLS = 20, 40
N_WSPLIT, WIDE_AT = 256, (17, 211)
I_EXACT, I_NONE = 4, 5                             # positions of the exact copy and of the read without a region in a class batch


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


def make_db():
    return get_db(200, 3300, "GTR", dg_k=4, seed=7)


def make_read(db, rng, cols, bases):
    """as tests/test_loads_batched.py: a read copied from a random leaf with 3 % substitutions, `bases` base sites in `cols` columns"""
    leaves = np.flatnonzero(db.is_leaf)
    u = int(leaves[rng.integers(len(leaves))])
    start = int(rng.integers(20, db.cs_len - cols - 20))
    end = start + cols - 1
    at = np.arange(start, end + 1) if cols == bases else \
        np.concatenate([[start, end], start + 1 + rng.choice(cols - 2, size=bases - 2, replace=False)])
    b = np.where(db.seq[u, at] >= 0, db.seq[u, at], db.seq[db.parent[u], at]).astype(np.int8)
    mut = rng.random(len(at)) < 0.03
    b[mut] = (b[mut] + rng.integers(1, 4, size=int(mut.sum()))) % 4
    codes = np.full(db.cs_len, GAP, np.int8)
    codes[at] = b
    return codes, start, end


def make_exact(db):
    """the exact copy: columns EXACT_START .. EXACT_START + 39 of the first inner node below the root (an inner node's sequence has no
    gaps).  The columns are conserved: most nodes of the tree carry the same 40 bases, so the read is an exact copy of every one of its seeds"""
    u = int(np.flatnonzero(~db.is_leaf & (db.parent >= 0))[0])
    codes = np.full(db.cs_len, GAP, np.int8)
    codes[EXACT_START:EXACT_START + EXACT_COLS] = db.seq[u, EXACT_START:EXACT_START + EXACT_COLS]
    assert (codes[EXACT_START:EXACT_START + EXACT_COLS] >= 0).all()
    return u, codes, EXACT_START, EXACT_START + EXACT_COLS - 1


def make_cases(db):
    """{class maximum: (codes [n][cs_len], start [n], end [n])} and the width-split batch under the key 0"""
    rng = np.random.default_rng(2025)
    _, xc, xs, xe = make_exact(db)
    cases = {}
    for M, (_, _, spec) in CLASSES.items():
        rd = [make_read(db, rng, c, b) for c, b in spec] + [(xc, xs, xe), (np.full(db.cs_len, GAP, np.int8), 0, -1)]
        cases[M] = (np.stack([r[0] for r in rd]), np.array([r[1] for r in rd], np.int32), np.array([r[2] for r in rd], np.int32))
    cd, st, en = (x.copy() for x in cases[512])
    pick = np.arange(N_WSPLIT) % len(st)                       # the narrow class over and over, two reads of 1,536 and 1,281 columns among them
    cd, st, en = cd[pick], st[pick], en[pick]
    for k, w in zip(WIDE_AT, (0, 1)):
        cd[k], st[k], en[k] = cases[1536][0][w], cases[1536][1][w], cases[1536][2][w]
    cases[0] = (cd, st, en)
    return cases


def _results(B):
    cnt, ids, d, N = B.seeds()
    used = np.arange(MAX_NSEED)[None, :] < cnt[:, None]
    out = dict(seed_cnt=cnt.copy())
    for name, a in zip(("seed_id", "seed_d", "seed_N"), (ids, d, N)):
        out[name] = np.where(used, a[:, :MAX_NSEED], 0)
    for name, a in zip(("est_ratio", "est_wnr", "est_loglik"), B.estimates()):
        out[name] = np.where(used, a[:, :MAX_NSEED], 0.0)       # slots without a seed are never written
    return out


def run_cases(E, db, cases, log=None):
    """every launch of the test: {"c<class>.w<weighted>.<field>": array}.  log(case, weighted): called after a run (the test reads the trace there)"""
    D = E.Database.from_synth(db)
    res = {}
    for M, (cd, st, en) in cases.items():
        B = E.Batch(D, len(st))
        B.set_knob("trace", 1)
        B.set_aligned(cd, st, en)
        for w in (0, 1):
            opts = E.default_opts(max_nseed=MAX_NSEED, weighted=w)
            B.get_seed(opts)
            B.estimate_seq(opts)
            for k, v in _results(B).items():
                res["c%d.w%d.%s" % (M, w, k)] = v
            if log:
                log(M, w)
        B.close()
    D.close()
    return res


_STATE = {}


def _state(capfd=None):
    """the runs on the device, once per session"""
    if not _STATE:
        E = _engine()
        db = make_db()
        cases = make_cases(db)
        trace = {}
        res = run_cases(E, db, cases, log=(lambda M, w: trace.__setitem__((M, w), capfd.readouterr().err)) if capfd else None)
        _STATE.update(E=E, db=db, cases=cases, res=res, trace=trace)
    return _STATE


def test_every_class_took_its_kernel_and_its_slots(capfd):
    s = _state(capfd)
    res = s["res"]
    for M, (inst, nw, _) in CLASSES.items():
        cd, st, en = s["cases"][M]
        w = en - st + 1
        assert sorted(w) == sorted([0, 40, 40, 65, M, w[1]]) and w[1] % (64 * nw) == 1, w
        for wt in (0, 1):
            assert inst + "\n" in s["trace"][(M, wt)], s["trace"][(M, wt)][-400:]
            cnt = res["c%d.w%d.seed_cnt" % (M, wt)]
            assert cnt[I_NONE] == 0 and (cnt[:I_NONE] > 0).all() and (cnt <= MAX_NSEED).all() and cnt.sum() >= 2 * nw, cnt
            assert (res["c%d.w%d.seed_d" % (M, wt)][I_EXACT, :cnt[I_EXACT]] == 0).all()         # an exact copy of the nodes it is seeded on
    for wt in (0, 1):
        assert "width split: 2 of 256 reads beyond 512 columns (widest 1536)" in s["trace"][(0, wt)], s["trace"][(0, wt)][-600:]


def test_same_bits_as_the_parent_commit(capfd):
    s = _state(capfd)
    res = s["res"]
    with np.load(GOLDEN) as g:
        assert sorted(g.files) == sorted(res), (sorted(set(g.files) ^ set(res)))
        bad = [k for k in g.files if g[k].dtype != res[k].dtype or g[k].shape != res[k].shape or g[k].tobytes() != res[k].tobytes()]
        for M in CLASSES:                                      # the exact copy on its seeds: no inferred state differs, wnr == 0
            k = int(g["c%d.w0.seed_cnt" % M][I_EXACT])
            assert k > 0 and (g["c%d.w0.est_wnr" % M][I_EXACT, :k] == 0.0).all() and (g["c%d.w0.seed_d" % M][I_EXACT, :k] == 0).all(), M
    assert not bad, bad


def test_against_the_oracle(capfd):
    """every slot with a seed against estimateSeq of the CPU oracle on the same (read, node, distance): ratio and the unweighted wnr
    exactly, the weighted wnr and loglik within the 1e-6 of tests/test_gpu_parity.py"""
    import test_gpu_parity as P
    s = _state(capfd)
    db, res = s["db"], s["res"]
    _, _, T = oracle_objects(db)
    memo = {}
    worst = dict(wnr=0.0, loglik=0.0)
    slots = 0
    for M, (cd, st, en) in s["cases"].items():
        for wt in (0, 1):
            r = {k: res["c%d.w%d.%s" % (M, wt, k)] for k in ("seed_cnt", "seed_id", "seed_d", "seed_N", "est_ratio", "est_wnr", "est_loglik")}
            for i in range(len(st)):
                for c in range(int(r["seed_cnt"][i])):
                    node, d, N = int(r["seed_id"][i, c]), int(r["seed_d"][i, c]), int(r["seed_N"][i, c])
                    key = (cd[i].tobytes(), int(st[i]), int(en[i]), node, wt)
                    if key not in memo:
                        memo[key] = T.estimate(cd[i], int(st[i]), int(en[i]), node, float(np.float64(d) / np.float64(N)), weighted=bool(wt))
                        slots += 1
                    o = memo[key]
                    where = (M, wt, i, c)
                    assert r["est_ratio"][i, c] == o["ratio"], where
                    if wt == 0:
                        assert r["est_wnr"][i, c] == o["wnr"], where
                    else:
                        worst["wnr"] = max(worst["wnr"], float(P._rel(r["est_wnr"][i, c], o["wnr"])))
                    worst["loglik"] = max(worst["loglik"], float(P._rel(r["est_loglik"][i, c], o["loglik"])))
    print("estimate uniform: %d distinct slots against the oracle, worst relative difference" % slots, worst)
    assert worst["wnr"] < P.REL and worst["loglik"] < P.REL, worst
