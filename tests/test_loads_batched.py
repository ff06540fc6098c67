"""The load phases of k_estimate_prod and k_place_blk (one round trip for a workgroup's message loads) change no arithmetic:
every instance that a region width selects gives, bit for bit, what the commit before the change gave, and agrees with the CPU
oracle as tests/test_gpu_parity.py asks.

The regions are handed over aligned (hu_batch_set_aligned) on a synthetic tree of 200 leaves with 3,300 consensus columns.  A launch
takes its kernel from the WIDEST region in it, so the reads go in one batch per width class — the class maximum, THREADS k + 1
columns for the estimate's and the placement's workgroup size, and 40 columns — and every batch runs the instance of its class on
all of its widths:

  class     estimate instance              placement instance (place_nosplit = 1)
  <= 512    <2, 4>      256 threads        <4, 2, ...>           128 threads
  <= 1,024  <4, 4>      256                <8, 2, ..., 3, 6>     128, gap/base split slots  (<8, 2, ...> in column order)
  <= 1,536  <6, 4, 4>   256                <12, 2, ..., 1, 10>   128, gap/base split slots  (<12, 2, ..., 1> in column order)
  <= 2,048  <8, 4>      256                <8, 4, ...>           256
  <= 3,072  <6, 8, 2>   512                <12, 4, ..., 1>       256

The widest read of the two split classes has exactly 256 bases and 768 / 1,280 gap sites: its base sites fill the base slots and its
gap sites the gap slots.  Reads of 40 columns with 40 bases have no gap site.  A batch of 256 reads, two of them wide, takes the
width-split second pass (the lists of the wide reads' slots and candidates in place of the sorted order).

tests/golden/loads_batched_parent.npz was written by tests/golden/loads_batched_parent_gen.py on the commit before the change; the
comparison with it is byte for byte."""
import os

import numpy as np
import pytest

from conftest import get_db, oracle_objects

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loads_batched_parent.npz")
MAX_NSEED = 16
GAP = -2
# class maximum -> (columns, bases) of its reads.  256 k + 1 / 512 k + 1: one site past k full rounds of the estimate's workgroup;
# 128 k + 1 / 256 k + 1: the same for the placement's
CLASSES = {
    512: [(512, 200), (257, 120), (385, 150), (40, 40)],
    1024: [(1024, 256), (769, 250), (897, 256), (40, 40)],
    1536: [(1536, 256), (1281, 200), (40, 40)],                # 1,281 = 256 x 5 + 1 = 128 x 10 + 1
    2048: [(2048, 450), (1793, 400), (40, 30)],                # 1,793 = 256 x 7 + 1
    3072: [(3072, 500), (2561, 480), (2817, 490), (40, 30)],   # 2,561 = 512 x 5 + 1, 2,817 = 256 x 11 + 1
}
SPLIT_CLASSES = (1024, 1536)
N_WSPLIT, WIDE_AT = 256, (17, 211)


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


def make_db():
    return get_db(200, 3300, "GTR", dg_k=4, seed=7)


def make_read(db, rng, cols, bases):
    """codes [cs_len], start, end of a read copied from a random leaf (its parent's inferred base where the leaf has a gap) with 3 %
    substitutions: `bases` base sites, the two ends among them, in a region of `cols` columns"""
    leaves = np.flatnonzero(db.is_leaf)
    u = int(leaves[rng.integers(len(leaves))])
    start = int(rng.integers(20, db.cs_len - cols - 20))
    end = start + cols - 1
    at = np.array([start, end]) if cols == bases or bases < 3 else \
        np.concatenate([[start, end], start + 1 + rng.choice(cols - 2, size=bases - 2, replace=False)])
    if cols == bases:
        at = np.arange(start, end + 1)
    b = np.where(db.seq[u, at] >= 0, db.seq[u, at], db.seq[db.parent[u], at]).astype(np.int8)
    mut = rng.random(len(at)) < 0.03
    b[mut] = (b[mut] + rng.integers(1, 4, size=int(mut.sum()))) % 4
    codes = np.full(db.cs_len, GAP, np.int8)
    codes[at] = b
    return codes, start, end


def make_cases(db):
    """{class maximum: (codes [n][cs_len], start [n], end [n])} and the width-split batch under the key 0"""
    rng = np.random.default_rng(2024)
    cases = {}
    for M, spec in CLASSES.items():
        rd = [make_read(db, rng, c, b) for c, b in spec]
        cases[M] = (np.stack([r[0] for r in rd]), np.array([r[1] for r in rd], np.int32), np.array([r[2] for r in rd], np.int32))
    cd, st, en = (x.copy() for x in cases[512])
    pick = np.arange(N_WSPLIT) % len(st)                       # the narrow class over and over, two reads of 1,536 and 1,281 columns among them
    cd, st, en = cd[pick], st[pick], en[pick]
    for k, w in zip(WIDE_AT, (0, 1)):
        cd[k], st[k], en[k] = cases[1536][0][w], cases[1536][1][w], cases[1536][2][w]
    cases[0] = (cd, st, en)
    return cases


def _results(B):
    cnt = B.seeds()[0]
    used = np.arange(MAX_NSEED)[None, :] < cnt[:, None]
    out = {}
    for name, a in zip(("est_ratio", "est_wnr", "est_loglik"), B.estimates()):
        out[name] = np.where(used, a[:, :MAX_NSEED], 0.0)       # slots without a seed are never written
    out["seed_cnt"] = cnt.copy()
    for k, v in B.candidates().items():
        out["cand_" + k] = v.copy()                             # iters: the outer iterations and the EM steps, packed
    return out


def run_cases(E, db, cases, log=None):
    """every launch of the test: {"<case>.<field>": array}.  log(case): called after a case's runs (the test reads the trace there)"""
    D = E.Database.from_synth(db)
    opts = E.default_opts(max_nseed=MAX_NSEED)
    res = {}
    for M, (cd, st, en) in cases.items():
        B = E.Batch(D, len(st))
        B.set_knob("trace", 1)
        B.set_aligned(cd, st, en)
        B.assign(opts)
        runs = {"c%d" % M: _results(B)}
        if M in SPLIT_CLASSES:
            B.set_knob("place_nosplit", 1)
            B.assign(opts)
            runs["c%d_nosplit" % M] = _results(B)
        B.close()
        for name, r in runs.items():
            for k, v in r.items():
                res[name + "." + k] = v
        if log:
            log(M)
    D.close()
    return res


_STATE = {}


def _state(capfd=None):
    """the runs on the device and the oracle's answer per distinct read, once per session"""
    if not _STATE:
        E = _engine()
        db = make_db()
        cases = make_cases(db)
        trace = {}
        res = run_cases(E, db, cases, log=(lambda M: trace.__setitem__(M, capfd.readouterr().err)) if capfd else None)
        _STATE.update(E=E, db=db, cases=cases, res=res, trace=trace)
    return _STATE


def test_every_class_took_its_kernel(capfd):
    s = _state(capfd)
    for M in SPLIT_CLASSES:
        err = s["trace"][M]
        assert "%d sites per thread, gap/base split slots" % (8 if M == 1024 else 12) in err and "column order" in err, err   # both forms ran
        cd, st, en = s["cases"][M]
        nb = (cd[0, st[0]:en[0] + 1] >= 0).sum()
        assert nb == 256 and en[0] - st[0] + 1 - nb == (768 if M == 1024 else 1280)          # base slots and gap slots exactly full
    assert "width split: 2 of 256 reads beyond 512 columns (widest 1536)" in s["trace"][0], s["trace"][0][-600:]
    for M, (cd, st, en) in s["cases"].items():
        if M:
            w = en - st + 1
            assert w.max() == M and w.min() == 40 and (s["res"]["c%d.seed_cnt" % M] > 0).all() and (np.diff(s["res"]["c%d.cand_offs" % M]) > 0).all()
    cd, st, en = s["cases"][512]
    assert (cd[3, st[3]:en[3] + 1] >= 0).all()                                                  # a read without a gap site


def test_same_bits_as_the_parent_commit(capfd):
    res = _state(capfd)["res"]
    with np.load(GOLDEN) as g:
        assert sorted(g.files) == sorted(res), (sorted(set(g.files) ^ set(res)))
        bad = [k for k in g.files if g[k].dtype != res[k].dtype or g[k].shape != res[k].shape or g[k].tobytes() != res[k].tobytes()]
    assert not bad, bad


def test_against_the_oracle(capfd):
    """as tests/test_gpu_parity.py: the same candidates in the same order (check_order_and_best), the same iteration counts, estimates
    and placed lengths within its 1e-6"""
    import test_gpu_parity as P
    from oracle import oracle_py as O
    s = _state(capfd)
    db, res = s["db"], s["res"]
    _, _, T = oracle_objects(db)
    oo = O.default_opts(maxNSeed=MAX_NSEED)
    memo = {}
    stats = dict(reads=0, near_tie_swaps=0, best_differs_by_tie=0)
    worst = 0.0
    for name in sorted({k.split(".")[0] for k in res}):
        M = int(name[1:].split("_")[0])
        cd, st, en = s["cases"][M]
        r = {k.split(".")[1]: v for k, v in res.items() if k.split(".")[0] == name}
        for i in range(len(st)):
            key = (cd[i].tobytes(), int(st[i]), int(en[i]))
            if key not in memo:
                memo[key] = T.assign(cd[i], int(st[i]), int(en[i]), oo)
            ref = memo[key]
            lo, hi = int(r["cand_offs"][i]), int(r["cand_offs"][i + 1])
            assert hi - lo == ref["n"] and r["seed_cnt"][i] == len(ref["seed_ids"]), (name, i)
            gpu_filt = [int(x) for x in r["cand_c_node"][lo:hi]]
            pos = [int(x) for x in ref["filt_order"]].index(int(ref["nodes"][0][0]))
            P.check_order_and_best(ref, gpu_filt, dict(c_node=gpu_filt[pos]), stats, db.parent)
            oc = {int(n_[0]): (v[0], v[1], int(n_[3])) for n_, v in zip(ref["nodes"], ref["vals"])}
            for c in range(lo, hi):
                r0, w0, it = oc[int(r["cand_c_node"][c])]
                worst = max(worst, abs(r["cand_ratio"][c] - r0) / max(abs(r0), 1e-3), abs(r["cand_wnr"][c] - w0) / max(abs(w0), 1e-3))
                assert (int(r["cand_iters"][c]) & 0xff) == it, (name, i, c)
            oe = {int(n_): e for n_, e in zip(ref["seed_ids"], ref["est"])}
            for c in range(lo, hi):
                assert P._rel(r["cand_est_loglik"][c], oe[int(r["cand_c_node"][c])][2]) < P.REL, (name, i, c)
    print("loads batched: oracle parity", stats, "worst relative difference of a placed length", worst)
    assert worst < P.REL, worst
