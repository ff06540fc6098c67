"""The floating-point kernels against an independent 50-digit derivation of the same formulas (tests/golden/hiprec.npz, see
tests/golden/make_hiprec_golden.py), one stage per test: k_model_pr, k_tree_up / down, k_tree_loglik, k_estimate_prod, k_filter,
k_place_blk, k_root_loglik, k_finish, and the streaming estimate / place kernels.

Integer results (seed counts, the ratio's quotient, the unweighted wnr, outer and EM iteration counts, the filter set, the taxon node) are
exact.  A continuous quantity is held to ten times the worst distance measured on an MI355X (libm and the compiler's choice of fused
multiply-adds may move last bits between ROCm versions; a wrong formula moves far more), and never to less than the project asks against
the oracle: 1e-12 for P(t) and logliks, REL for lengths, 1e-9 max(1, |x|) for messages, the conditioned q bound with 1e-6.

Worst distance from the 50-digit values, measured on an MI355X (ROCm 7, the six databases of the archive, every variant below), and the
bound each test asserts (ten times the worst, capped by the project's own figure):

  stage (kernel)                                   quantity                                      worst     bound    project's
  P(t) (k_model_pr)                                absolute                                      8.9e-16   8.9e-15  1e-12
  messages (k_tree_up / k_tree_down)               relative to max(|x|, 1)                       1.8e-12   1.8e-11  1e-9
  root loglik per column and sum (k_tree_loglik)   relative                                      3.5e-14   3.5e-13  1e-12
  estimated loglik (k_estimate_prod, streaming)    relative                                      2.1e-14   2.1e-13  1e-12
  weighted wnr (k_estimate_prod)                   relative to max(|x|, 1e-3)                    2.9e-14   2.9e-13  REL
  placed ratio, wnr (k_place_blk<4, 2, 3, 0, 2>,   relative to max(|x|, 1e-3)                    4.5e-11   4.5e-10  REL
    <12, 2, 1, 0, 2> under place_var = 6, and        (4.5e-14 absolute: the ratios are ~3e-4)
    the streaming place kernel)
  placed height                                    relative to max(|x|, 1e-3)                    1.7e-12   1.7e-11  REL
  intended root loglik (k_root_loglik)             relative                                      4.8e-15   4.8e-14  1e-12
  the reference's constant loglik                  relative                                      1.5e-16   1e-12    1e-12
  q-values (k_finish)                              eps of |dq| <= (10 / ln 10) eps / (1 - p)     1.2e-12   1.2e-11  1e-6
                                                     + 1e-12 q
  seed counts, ratio, unweighted wnr, iteration counts, filter set, taxon node                    exact

Regions of at most 190 columns select the four-sites-per-thread instance of k_place_blk with v in registers and k_estimate_prod<2, 4>.
Every other instance of the two dispatch chains runs on the wide set (tests/golden/hiprec_wide.npz: GTR+4 and JC69 on 8 leaves x 3,300
columns, twelve reads of 512 to 3,073 columns, each in a batch of its own; WIDE_INSTANCES / WIDE_KNOB_FORMS below name the instance per
read, which the tests assert from the trace lines).  Its bounds do not come from the kernels: per quantity
min(project's, max(the narrow bound above, 10 x the oracle's worst distance over the wide set)), the oracle measured on the CPU first.

  quantity (wide set)                              oracle    narrow bound  bound     kernels' worst (MI355X, over every instance)
  estimated loglik, relative                       6.2e-14   2.1e-13       6.2e-13   7.4e-16
  weighted wnr, relative to max(|x|, 1e-3)         5.4e-14   2.9e-13       5.4e-13   3.2e-15
  placed ratio, wnr, relative to max(|x|, 1e-3)    7.6e-12   4.5e-10       4.5e-10   1.8e-11
  placed height, relative to max(|x|, 1e-3)        7.5e-13   1.7e-11       1.7e-11   5.3e-12
  intended root loglik, relative                   5.7e-14   4.8e-14       5.7e-13   1.1e-15
  the reference's constant loglik, relative        1.6e-16   1e-12         1e-12     1.6e-16
  q-values, eps of the conditioned bound           2.1e-10   1.2e-11       2.1e-9    6.4e-12

  per instance (wide set)                          reads (columns)                     est. loglik   weighted wnr
  k_estimate_prod<2,4>                             512                                 7.4e-16       3.2e-15
  k_estimate_prod<4,4>                             513, 1,024                          7.4e-16       7.9e-16
  k_estimate_prod<6,4,4>                           1,025, 1,400, 1,536                 6.7e-16       5.8e-16
  k_estimate_prod<8,4>                             1,537, 2,048                        7.3e-16       8.0e-16
  k_estimate_prod<6,8,2>                           2,049, 3,072                        7.3e-16       7.6e-16
  k_estimate_prod<12,4> (est_var = 4)              2,049, 3,072                        7.3e-16
  k_estimate_blk<2 .. 12,256> (est_var = 2)        512, 1,024, 1,536, 2,048, 3,072     7.4e-16
  k_estimate (streaming)                           3,073                               7.3e-16       1.0e-15
                                                                                       ratio, wnr    height     root loglik
  k_place_blk<4,2,3,0,2>                           512                                 2.4e-12       7.9e-13    7.5e-16
  k_place_blk<8,2,3,0,3,false,3,6> (v in LDS)      513, 1,024 (256 bases)              5.6e-12       1.0e-12    7.4e-16
  k_place_blk<8,2,3,0,2,false,0,6> (place_var 6)   513, 1,024 (256 bases)              5.6e-12       1.0e-12
  k_place_blk<8,2,3,0,2>                           1,024 (257 bases; place_nosplit)    5.6e-12       1.2e-12    5.5e-16
  k_place_blk<12,2,3,0,2,false,1,10>               1,025, 1,536                        1.8e-11       6.5e-13    8.6e-16
  k_place_blk<12,2,3,0,2,false,1>                  1,400 (257 bases; place_nosplit)    1.3e-11       4.7e-12    1.1e-15
  k_place_blk<12,2,1,0,2> (place_var 6)            1,024 and 1,400 (257 bases)         1.3e-11       4.7e-12
  k_place_blk<12,2,3,0,2> (place_var 7)            513, 1,536                          4.8e-12       1.0e-12
  k_place_blk<8,4,3,0,1>                           1,537, 2,048                        9.2e-12       5.3e-12    7.3e-16
  k_place_blk<12,4,3,0,2,false,1>                  2,049, 3,072                        5.3e-12       1.1e-12    7.3e-16
  k_place_blk<12,4,3,0,1> (place_var 9)            2,049, 3,072                        5.3e-12       1.1e-12
  k_place (streaming)                              3,073                               6.7e-12       6.9e-13    4.9e-16

With the Newton step of the reciprocal shared by four sites (EMV = 3) removed, every EMV = 3 instance is 7.9e-7 to 5.7e-6 off in ratio / wnr
and fails here, while tests/test_gpu_parity.py::test_wide_region_kernels (REL against the oracle) still passes; with the spt2 <= 8
threshold moved by one, the 1,024-column reads fail on the instance assertion alone.
The oracle against the same values (tests/test_hiprec_oracle.py): P(t) 1.0e-15, messages 9.1e-13 (synth's numpy messages 4.2e-12),
logliks 5.0e-15, placed lengths 5.3e-14 absolute.
A knife-edge candidate (hiprec_cases.Case.knife: 10 of the 1,260, all on JC69's two-column read) is compared neither in its counts nor
in its unweighted wnr, and in its lengths to REL; everything else of it is compared as for any other candidate.

The deep set (tests/golden/hiprec_deep.npz, test_deep_*): GTR+4 and JC69 on 1,024 leaves x 96 columns with branches long enough that 19 / 64
of the 64 match columns have a root message below the -510 at which tree_conv, TreeAcc::finish and k_tree_loglik rescale (the lowest -766 /
-963; the all-gap columns -1,197 / -1,420), so that the packing exponents and the carried exponent of k_estimate_prod / k_place_blk / the
streaming kernels are in the thousands.  Six reads per database, each with a candidate list of its own (at most 48 nodes, given through
Batch.get_seed_given; the (d, N) of the given seeds are asserted), the instance asserted from the trace lines.  Bounds by the wide set's
rule from the CPU's distances (ORACLE_DEEP), fixed before a kernel ran; messages by hiprec_cases.level_shape (level: the largest component,
relative to max(|x|, 1); shape: the other components relative to it, absolute -- the linear value's relative error), for which there is no
project figure: 10 x the larger of the oracle's and synth's distance.

  quantity (deep set)                              oracle (synth)      narrow bound  bound     kernels' worst (MI355X, every variant)
  message level (k_tree_up / k_tree_down)          2.2e-14 (1.3e-13)                 1.4e-12   3.0e-14
  message shape                                    4.7e-12 (9.3e-12)                 9.4e-11   4.1e-12
  root loglik per column and sum (k_tree_loglik)   2.8e-14 (2.4e-14)   3.5e-13       3.5e-13   2.3e-14
  estimated loglik, relative                       4.9e-15             2.1e-13       2.1e-13   4.7e-15
  weighted wnr, relative to max(|x|, 1e-3)         2.0e-14             2.9e-13       2.9e-13   1.6e-14
  placed ratio, wnr, relative to max(|x|, 1e-3)    1.3e-11             4.5e-10       4.5e-10   1.3e-11
  placed height, relative to max(|x|, 1e-3)        7.8e-13             1.7e-11       1.7e-11   1.4e-12
  intended root loglik, relative                   4.9e-15             4.8e-14       4.9e-14   4.7e-15
  the reference's constant loglik, relative        1.6e-16             1e-12         1e-12     1.6e-16
  q-values, eps of the conditioned bound           8.0e-12             1.2e-11       8.1e-11   5.6e-12
  counts, ratio, unweighted wnr, iteration counts, filter sets, taxon nodes                    exact (7 knife-edge candidates of 344)

Found by test_deep_estimate_place_q[JC690]: k_place_blk<4,2,3,0,2> returned NaN for ratio, wnr and height of one candidate (the
one-column read against a leaf of another base).  em_branch_blk forms p as p0 times a rounded reciprocal, which can exceed 1 by an ulp
once q is below 2^-53; q = 1 - p was then negative and -log q NaN, where the reference's quotient never rounds above 1, reads q = 0 and
takes the cap.  p is now clamped to 1 (no other output changes: the case gave NaN before).
With tree_conv's scale forced to 0 test_deep_tree_messages_and_loglik fails on both databases, with TreeAcc::finish's on GTR+4 alone, and
every other test of this file passes on both builds.

The deepwide set (tests/golden/hiprec_deepwide.npz, test_deepwide_*): the wide instances at depth, the regime of every production read.
GTR+4 (mean branch length 0.3) and JC69 (0.15) on 1,029 leaves x 3,300 columns, 1,200 of them match columns: 301 / 1,200 of the match
columns have a root message below -510 (the lowest -841 / -986), the sparse columns reach -1,208 / -1,427, so the packing exponents are
about -2,000 per site and the carried sum of a read about -1e6 to -6e6, with deep and shallow columns side by side among one thread's sites
on GTR+4.  Seven reads per database (DEEPWIDE_READS: the rows of WIDE_INSTANCES above the 4-site class that differ in their pair of
instances), each in a batch of its own against a database uploaded once, with twelve candidates given through Batch.get_seed_given (the
read's leaf and three ancestors with their siblings, the children of the root, two leaves of the other root subtree; the (d, N) of the
given seeds are asserted).  The instance is asserted from the trace lines against the row of WIDE_INSTANCES / WIDE_KNOB_FORMS with the
read's shape, and every test first asserts from the rebuilt database's own root message that its read holds bases on at least 16 match
columns below -510.  Bounds by the wide and deep rule from the CPU's distances (ORACLE_DEEPWIDE), fixed before a kernel ran on this set.

  quantity (deepwide set)                          oracle    narrow bound  bound     kernels' worst (MI355X, over every instance)
  estimated loglik, relative                       2.1e-14   2.1e-13       2.1e-13   1.4e-15
  weighted wnr, relative to max(|x|, 1e-3)         4.6e-14   2.9e-13       4.6e-13   4.1e-15
  placed ratio, wnr, relative to max(|x|, 1e-3)    5.8e-12   4.5e-10       4.5e-10   2.5e-12
  placed height, relative to max(|x|, 1e-3)        5.7e-13   1.7e-11       1.7e-11   7.3e-13
  intended root loglik, relative                   1.9e-14   4.8e-14       1.9e-13   1.5e-15
  the reference's constant loglik, relative        1.6e-16   1e-12         1e-12     1.6e-16
  q-values, eps of the conditioned bound           2.4e-11   1.2e-11       2.4e-10   1.3e-12
  counts, ratio, unweighted wnr, iteration counts, filter sets, taxon nodes                    exact (no knife-edge candidate among 168)

  per instance (deepwide set, both databases)      reads (columns)                     est. loglik   weighted wnr
  k_estimate_prod<4,4>                             1,024 (256 and 257 bases)           1.2e-15       3.8e-15
  k_estimate_prod<6,4,4>                           1,400, 1,536                        1.4e-15       4.1e-15
  k_estimate_prod<8,4>                             2,048                               1.3e-15       2.5e-15
  k_estimate_prod<6,8,2>                           3,072                               1.4e-15       2.8e-15
  k_estimate_prod<12,4> (est_var = 4)              3,072                               1.4e-15
  k_estimate_blk<4 .. 12,256> (est_var = 2)        1,024, 1,536, 2,048, 3,072          1.4e-15
  k_estimate (streaming)                           3,073; 1,024 under streaming_sep    1.3e-15       2.4e-15
                                                                                       ratio, wnr    height     root loglik
  k_place_blk<8,2,3,0,3,false,3,6> (v in LDS)      1,024 (256 bases)                   2.5e-12       7.3e-13    1.2e-15
  k_place_blk<8,2,3,0,2,false,0,6> (place_var 6)   1,024 (256 bases)                   2.5e-12       7.3e-13
  k_place_blk<8,2,3,0,2>                           1,024 (257 bases; place_nosplit)    2.5e-12       7.3e-13    1.2e-15
  k_place_blk<12,2,3,0,2,false,1,10>               1,536                               1.0e-12       2.4e-13    1.4e-15
  k_place_blk<12,2,3,0,2,false,1>                  1,400 (257 bases; place_nosplit)    1.1e-12       2.4e-13    1.2e-15
  k_place_blk<12,2,1,0,2> (place_var 6)            1,024 and 1,400 (257 bases)         1.1e-12       4.6e-13
  k_place_blk<12,2,3,0,2> (place_var 7)            1,536                               1.0e-12       2.4e-13
  k_place_blk<8,4,3,0,1>                           2,048                               1.5e-12       7.5e-14    1.5e-15
  k_place_blk<12,4,3,0,2,false,1>                  3,072                               1.2e-12       6.6e-13    1.4e-15
  k_place_blk<12,4,3,0,1> (place_var 9)            3,072                               1.2e-12       6.6e-13
  k_place (streaming)                              3,073; 1,024 under streaming_sep    1.9e-12       2.9e-13    1.3e-15

All 80 tests passed on their first run: no kernel bug was found at depth and width.  What the set can and cannot see, on three scratch
builds run against the wide, deep and deepwide tests:
  (a) `ksum` of k_estimate_prod accumulated in an int16_t: every test passes, the deepwide ones included.  A site's two exponents add up
      to about its root message over ln 2, at most -2,059 here, and a thread holds at most twelve sites: -24,700, inside 16 bits.  The
      per-thread sum could leave 16 bits only on a tree of about 1,400 leaves or more; this set does not reach that.
  (b) the guard of em_branch_blk for p > 1 removed: the four deep tests of JC69's one-column read fail with NaN, as when the bug was found;
      no deepwide (or wide) instance returns NaN.  p exceeds 1 only once q is below 2^-53, which takes a read that contradicts the
      candidate at every base site; a read of 256 or more base sites never does.  The guard stands after the EM loop of the one
      em_branch_blk template that every instance is built from, so the deep set's two instances stand for the others there.
  (c) the wave's exponent sum of k_estimate_prod truncated to 16 bits before the waves are added: all 38 deepwide tests that compare an
      estimated loglik of a k_estimate_prod instance fail (every shipped instance and every knob form, both databases; k_estimate_blk and
      the streaming kernel, which carry the exponent their own way, pass), the deep set fails on k_estimate_prod<2,4>, and all 126 wide
      tests pass: a wave's sum is about -1e6 here and about -1e4 on the wide set.
So the set holds the carried exponent of every wide instance to the exact values from the wave level upwards, and the placement
instances to the exact lengths on rescaled messages; it does not reach a thread's own 32-bit sum, nor the p > 1 corner.
"""
import re

import numpy as np
import pytest

from hiprec_cases import CASES, DEEP_CASES, DEEP_LL, DEEPWIDE_CASES, DEEPWIDE_READS, WIDE_CASES, WIDE_READS, Case, level_shape, q_ok, ratio_half

pytestmark = pytest.mark.gpu

REL = 1e-6
# what the project already asserts against the oracle: no bound below is looser
FLOOR = dict(model_pr=1e-12, msg=1e-9, loglik=1e-12, length=REL, q_eps=1e-6)
# ten times the worst distance measured on the device (see the table above)
TEN_X = dict(model_pr=8.9e-15, msg=1.8e-11, tree_ll=3.5e-13, est_ll=2.1e-13, est_wnr_w=2.9e-13, length=4.5e-10, height=1.7e-11,
             root_ll=4.8e-14, q_eps=1.2e-11)
FLOOR_OF = dict(model_pr="model_pr", msg="msg", tree_ll="loglik", est_ll="loglik", est_wnr_w="length", length="length", height="length",
                root_ll="loglik", q_eps="q_eps")


# the wide set: the oracle's worst distance from the 50-digit values over both databases and all twelve reads, measured on the CPU
# (tests/test_hiprec_oracle.py, the HIPREC oracle_wide_* lines; est_ll is the larger of the unweighted and the weighted loglik, q_eps the eps
# that the conditioned q bound needs) -- plain double arithmetic on the same formulas: ten times it is what their conditioning at these
# widths allows a correct double implementation
ORACLE_WIDE = dict(est_ll=6.2e-14, est_wnr_w=5.4e-14, length=7.6e-12, height=7.5e-13, root_ll=5.7e-14, q_eps=2.1e-10)


def bound(key):
    return min(FLOOR[FLOOR_OF[key]], TEN_X[key])


def bound_wide(key):
    """min(project floor, max(the narrow bound, 10 x the oracle's worst distance over the wide set)): fixed before any kernel ran"""
    return min(FLOOR[FLOOR_OF[key]], max(TEN_X[key], 10.0 * ORACLE_WIDE[key]))


def worse(worst, key, x):
    """worst[key] = max(worst[key], x) for a distance that is a number: a NaN, or an infinity against a finite exact value, fails here
    (Python's max(0.0, nan) is 0.0)"""
    x = float(x)
    assert np.isfinite(x), (key, x)
    worst[key] = max(worst[key], x)


def report(test, name, **worst):
    """every figure before it is asserted"""
    print("HIPREC %s %s %s" % (test, name, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


def _rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return np.abs(a - b) / np.maximum(1e-300, np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("name", CASES)
def test_model_pr(name):
    E = _engine()
    c = Case(name)
    D = E.Database.from_synth(c.db)
    P = D.model_pr(c.times().ravel()).reshape(c.P.shape)
    D.close()
    worst = np.abs(P - c.P).max()
    report("model_pr", name, model_pr=worst)
    assert np.isfinite(worst) and worst <= bound("model_pr")


@pytest.mark.parametrize("name", CASES)
def test_tree_messages_and_loglik(name):
    E = _engine()
    import torch
    c = Case(name)
    db = c.db
    n, L = db.seq.shape
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k else None)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up = torch.full((n, L, 4), 7.0, dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    seq, h = E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    per, tot = E.tree_loglik(n, L, 0, md, up.data_ptr())
    gu, gd = up.cpu().numpy()[:, c.msg_cols], down.cpu().numpy()[1:, c.msg_cols]
    assert np.array_equal(seq, db.seq)
    worst = dict(height=np.abs(h - c.height).max(), tree_ll=max(_rel(per, c.root_ll).max(), float(_rel(tot, c.root_ll_sum))))
    for key, got, want in (("up", gu, c.up), ("down", gd, c.down[1:])):
        inf = np.isneginf(want)
        assert np.array_equal(np.isneginf(got), inf), key
        worst[key] = (np.abs(got[~inf] - want[~inf]) / np.maximum(np.abs(want[~inf]), 1.0)).max()
    report("tree", name, **worst)
    assert all(np.isfinite(v) for v in worst.values()), worst
    assert worst["up"] <= bound("msg") and worst["down"] <= bound("msg")
    assert worst["tree_ll"] <= bound("tree_ll")
    assert worst["height"] < 1e-14


def _run(c, knobs=None, stop_after=None, D=None, **opts_kw):
    """the read stages on the archive's reads: every non-root node a seed, every seed placed unless max_error says otherwise.
    D: a database uploaded already, which stays open"""
    E = _engine()
    own = D is None
    if own:
        D = E.Database.from_synth(c.db)
    B = E.Batch(D, c.n_reads)
    for k, v in (knobs or {}).items():
        B.set_knob(k, v)
    B.set_aligned(c.codes, c.start, c.end)
    opts = E.default_opts(**dict(dict(max_error=1e9), **opts_kw))
    if c.deep:                                      # the read's own candidate list, given: the seeds come back in its order
        B.get_seed_given(c.n_cand, c.cand)
        cnt, ids, sd, sN = B.seeds()
        n_cand = c.cand.shape[1]
        real = c.cand >= 0
        assert np.array_equal(cnt, c.n_cand) and np.array_equal(ids[:, :n_cand][real], c.cand[real])
        pos = np.broadcast_to(np.arange(n_cand), (c.n_reads, n_cand))
        assert np.array_equal(sd[:, :n_cand][real], c.dN[:, :, 0][real]) and np.array_equal(sN[:, :n_cand][real], c.dN[:, :, 1][real])
    else:
        B.get_seed(opts)
        cnt, ids, sd, sN = B.seeds()
        n_cand = len(c.seeds)
        assert (cnt == n_cand).all()
        pos = np.argsort(ids[:, :n_cand], axis=1)                # position of node k + 1 in the read's seed list
        assert np.array_equal(np.take_along_axis(ids[:, :n_cand], pos, 1), np.broadcast_to(c.seeds, (c.n_reads, n_cand)))
        assert np.array_equal(np.take_along_axis(sd[:, :n_cand], pos, 1), c.dN[:, :, 0]) and np.array_equal(np.take_along_axis(sN[:, :n_cand], pos, 1), c.dN[:, :, 1])
    B.estimate_seq(opts)
    out = dict(est=[np.take_along_axis(a[:, :n_cand], pos, 1) for a in B.estimates()])
    if stop_after != "estimate":
        B.filter_placements(opts); B.place_seq(opts); B.calc_q_values(opts)
        out["cand"] = B.candidates()
        out["offs"], out["places"] = B.candidate_places()
    B.close()
    if own:
        D.close()
    return out


def _check_estimates(c, name, est, weighted, test, bound=bound):
    er, ew, el = est
    worst = dict(est_ll=0.0, est_wnr_w=0.0)
    for ri in range(c.n_reads):
        for k in range(len(c.cands(ri))):
            assert er[ri, k] == c.ratio_double(ri, k), (ri, k)   # the same integer quotients
            if weighted:
                worse(worst, "est_wnr_w", abs(ew[ri, k] - c.est_wnr_w[ri, k]) / max(abs(c.est_wnr_w[ri, k]), 1e-3))
            elif not c.knife[ri, k]:
                assert ew[ri, k] == c.wnr_unweighted(ri, k), (ri, k)
            want = (c.est_ll_w if weighted else c.est_ll)[ri, k]
            assert np.isfinite(want) and np.isfinite(el[ri, k]), (ri, k, el[ri, k], want)
            worse(worst, "est_ll", _rel(el[ri, k], want))
    report(test, name, **worst)
    assert worst["est_ll"] <= bound("est_ll") and worst["est_wnr_w"] <= bound("est_wnr_w"), worst


def _check_places(c, name, out, test, prior=0, fix=0, bound=bound):
    cand, offs, places = out["cand"], out["offs"], out["places"]
    worst = dict(length=0.0, height=0.0, root_ll=0.0, const_ll=0.0, q_eps=0.0)
    for ri in range(c.n_reads):
        lo, hi = int(offs[ri]), int(offs[ri + 1])
        assert hi - lo == len(c.cands(ri)) and np.array_equal(cand["offs"], offs)
        qs = c.q_exact(ri, prior, fix) if ri in c.q_reads else None
        for x in range(lo, hi):
            g = places[x]
            u = int(g["c_node"]); k = c.slot(ri, u)
            assert int(cand["c_node"][x]) == u == int(c.cands(ri)[k]) and int(g["p_node"]) == int(c.parent[u])
            ratio, wnr = c.pl_ratio[ri, k], c.pl_wnr[ri, k]
            height = c.placed_height(ri, k)
            errs = (abs(g["ratio"] - ratio) / max(abs(ratio), 1e-3), abs(g["wnr"] - wnr) / max(abs(wnr), 1e-3),
                    abs(g["height"] - height) / max(abs(height), 1e-3))
            assert np.isfinite(errs).all(), (ri, u, g["ratio"], g["wnr"], g["height"])
            if c.knife[ri, k]:                                   # counts not compared, lengths to REL; everything else as for any candidate
                assert max(errs) <= REL, (ri, u, errs)
            else:
                it = int(cand["iters"][x])
                assert (it & 0xff, it >> 8) == (int(c.pl_outer[ri, k]), int(c.pl_em[ri, k])), (ri, u, g["ratio"], g["wnr"], ratio, wnr)
                worse(worst, "length", max(errs[:2]))
                worse(worst, "height", errs[2])
            if fix:
                assert g["loglik"] == g["root_loglik"] and np.isfinite(g["root_loglik"])
                worse(worst, "root_ll", _rel(g["root_loglik"], c.pl_root_ll[ri, k]))
            else:
                assert np.isfinite(g["loglik"])
                worse(worst, "const_ll", _rel(g["loglik"], c.pl_const_ll[ri]))
            if abs(ratio - 0.5) > 1e-6:
                assert int(g["a_node"]) == int(c.pl_a_node[ri, k])
            if qs is not None:
                for q, qe, omp in ((g["q_place"], qs[0][k], qs[2][k]),) + (() if ratio_half(c, ri) else ((g["q_taxon"], qs[1][k], qs[3][k]),)):
                    assert np.isfinite(q) and q_ok(q, qe, omp, bound("q_eps")), (ri, u, q, qe, omp)
                    if omp >= 1e-6:
                        worse(worst, "q_eps", (abs(q - qe) - 1e-12 * qe) * omp * np.log(10.0) / 10.0)
    report(test, name, **worst)
    assert worst["length"] <= bound("length") and worst["height"] <= bound("height"), worst
    assert worst["root_ll"] <= bound("root_ll") and worst["const_ll"] <= FLOOR["loglik"], worst


@pytest.mark.parametrize("name", CASES)
def test_estimate_place_q(name):
    """k_estimate_prod, k_place_blk and k_finish as shipped: unweighted estimate, the reference's constant loglik, prior UNIFORM"""
    c = Case(name)
    out = _run(c)
    _check_estimates(c, name, out["est"], False, "estimate")
    _check_places(c, name, out, "place")


@pytest.mark.parametrize("name", CASES)
def test_estimate_weighted(name):
    c = Case(name)
    _check_estimates(c, name, _run(c, stop_after="estimate", weighted=1)["est"], True, "estimate_weighted")


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prior,fix", [(1, 0), (0, 1), (1, 1)])
def test_prior_and_fixed_root_loglik(name, prior, fix):
    """k_root_loglik and the prior term of k_finish"""
    c = Case(name)
    _check_places(c, name, _run(c, prior=prior, fix_root_loglik=fix), "place_prior%d_fix%d" % (prior, fix), prior, fix)


@pytest.mark.parametrize("name", CASES)
def test_filter_set_at_the_default_max_error(name):
    c = Case(name)
    out = _run(c, max_error=c.max_error)
    for ri in range(c.n_reads):
        got = sorted(int(x) for x in out["cand"]["c_node"][int(out["offs"][ri]):int(out["offs"][ri + 1])])
        assert got == sorted(int(u) for u, keep in zip(c.seeds, c.filter_in[ri]) if keep), ri


@pytest.mark.parametrize("name", CASES)
def test_place_var6_instance(name):
    """place_var = 6 on regions of at most 190 columns runs k_place_blk<12, 2, 1, 0, 2>: twelve sites per thread and one Newton-refined
    reciprocal per site (EMV = 1), where the shipped instance for these widths, k_place_blk<4, 2, 3, 0, 2>, has four sites per thread and
    one reciprocal per four sites (EMV = 3).  Both keep the v message in registers; the instance that keeps it in LDS takes regions of
    513 to 1,024 columns and is held to the same values by the wide set below (test_wide_estimate_place_q)"""
    c = Case(name)
    _check_places(c, name, _run(c, knobs=dict(place_var=6)), "place_var6")


@pytest.mark.parametrize("name", CASES)
def test_streaming_kernels(name):
    """the one-wave streaming estimate / place kernels share nothing with the register-resident ones but the formulas"""
    c = Case(name)
    out = _run(c, knobs=dict(streaming_sep=1), fix_root_loglik=1)
    _check_estimates(c, name, out["est"], False, "estimate_streaming")
    _check_places(c, name, out, "place_streaming", 0, 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# The wide set (tests/golden/hiprec_wide.npz): one read per width class of the dispatch in hu_estimate_batch / hu_place_batch, each in a
# batch of its own, so that the widest region and the gap / base site maxima that choose the instance are that read's.  The instance is
# read from the two trace lines and asserted against the table below: a moved threshold fails until the table is edited on purpose.
#
#   read (columns, base sites)   estimate                  placement (default knobs)                       site order
WIDE_INSTANCES = [
    ((512, 120),  "k_estimate_prod<2,4>",   "k_place_blk<4,2,3,0,2>",             "column order"),           # top of the 4-site class
    ((513, 100),  "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,3,false,3,6>",   "gap/base split slots"),   # v in LDS, last slots almost empty
    ((1024, 256), "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,3,false,3,6>",   "gap/base split slots"),   # 768 gap + 256 base sites: both lists full
    ((1024, 257), "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,2>",             "column order"),           # one base too many
    ((1025, 150), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,3,0,2,false,1,10>", "gap/base split slots"),
    ((1536, 256), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,3,0,2,false,1,10>", "gap/base split slots"),   # 1,280 + 256: both lists full
    ((1400, 257), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,3,0,2,false,1>",    "column order"),
    ((1537, 200), "k_estimate_prod<8,4>",   "k_place_blk<8,4,3,0,1>",             "column order"),           # first width of the four-wave forms
    ((2048, 300), "k_estimate_prod<8,4>",   "k_place_blk<8,4,3,0,1>",             "column order"),
    ((2049, 250), "k_estimate_prod<6,8,2>", "k_place_blk<12,4,3,0,2,false,1>",    "column order"),
    ((3072, 500), "k_estimate_prod<6,8,2>", "k_place_blk<12,4,3,0,2,false,1>",    "column order"),
    ((3073, 300), "k_estimate",             "k_place",                            "column order"),           # streaming kernels by width
]
assert [w[0] for w in WIDE_INSTANCES] == WIDE_READS
READ_OF = {shape: ri for ri, shape in enumerate(WIDE_READS)}
# the forms that only a knob reaches: (read, knobs, estimate, placement, site order)
WIDE_KNOB_FORMS = [
    ((513, 100),  dict(place_var=6), "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,2,false,0,6>", "gap/base split slots"),   # v in registers
    ((1024, 256), dict(place_var=6), "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,2,false,0,6>", "gap/base split slots"),
    ((1024, 257), dict(place_var=6), "k_estimate_prod<4,4>",   "k_place_blk<12,2,1,0,2>",          "column order"),
    ((1400, 257), dict(place_var=6), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,1,0,2>",          "column order"),
    ((513, 100),  dict(place_var=7), "k_estimate_prod<4,4>",   "k_place_blk<12,2,3,0,2>",          "column order"),
    ((1536, 256), dict(place_var=7), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,3,0,2>",          "column order"),
    ((2049, 250), dict(place_var=9, est_var=4), "k_estimate_prod<12,4>", "k_place_blk<12,4,3,0,1>", "column order"),
    ((3072, 500), dict(place_var=9, est_var=4), "k_estimate_prod<12,4>", "k_place_blk<12,4,3,0,1>", "column order"),
    ((1024, 256), dict(place_nosplit=1), "k_estimate_prod<4,4>",   "k_place_blk<8,2,3,0,2>",          "column order"),
    ((1536, 256), dict(place_nosplit=1), "k_estimate_prod<6,4,4>", "k_place_blk<12,2,3,0,2,false,1>", "column order"),
    ((512, 120),  dict(est_var=2), "k_estimate_blk<2,256>",  "k_place_blk<4,2,3,0,2>",             "column order"),
    ((1024, 256), dict(est_var=2), "k_estimate_blk<4,256>",  "k_place_blk<8,2,3,0,3,false,3,6>",   "gap/base split slots"),
    ((1536, 256), dict(est_var=2), "k_estimate_blk<6,256>",  "k_place_blk<12,2,3,0,2,false,1,10>", "gap/base split slots"),
    ((2048, 300), dict(est_var=2), "k_estimate_blk<8,256>",  "k_place_blk<8,4,3,0,1>",             "column order"),
    ((3072, 500), dict(est_var=2), "k_estimate_blk<12,256>", "k_place_blk<12,4,3,0,2,false,1>",    "column order"),
]
_shape_id = lambda v: "%dx%d" % v if isinstance(v, tuple) else None


@pytest.fixture(scope="module")
def wide():
    """(case, uploaded database) of a wide case, shared by the tests of this module: the upload of 15 nodes x 3,300 columns costs more
    than a batch of one read"""
    held = {}

    def get(name):
        if name not in held:
            c = Case(name, "wide")
            held[name] = (c, _engine().Database.from_synth(c.db))
        return held[name]
    yield get
    for _, D in held.values():
        D.close()


def _instances(err, width):
    """(estimate kernel, placement kernel, site order) from the trace of one batch: one line of each stage, both naming the read's width"""
    est = re.findall(r"^\[hu\] estimate: max region (\d+), (\S+)$", err, re.M)
    pl = re.findall(r"^\[hu\] place: \d+ candidates, max region (\d+), (?:\d+ sites per thread|sites streamed per sweep), "
                    r"(gap/base split slots|column order), [^,]+, (\S+)$", err, re.M)
    assert len(est) == 1 and len(pl) <= 1, err
    assert int(est[0][0]) == width and all(int(p[0]) == width for p in pl), err
    return (est[0][1],) + ((pl[0][2], pl[0][1]) if pl else (None, None))


def _wide_run(wide, capfd, name, shape, knobs=None, **kw):
    c, D = wide(name)
    one = c.one_read(READ_OF[shape])
    capfd.readouterr()
    out = _run(one, knobs=dict(knobs or {}, trace=1), D=D, **kw)
    return one, out, _instances(capfd.readouterr().err, shape[0])


@pytest.mark.parametrize("name", WIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", WIDE_INSTANCES, ids=_shape_id)
def test_wide_estimate_place_q(wide, capfd, name, shape, est_k, place_k, order):
    """default knobs: the unweighted estimate, the placement with the constant loglik, q-values where the archive holds them"""
    one, out, ran = _wide_run(wide, capfd, name, shape)
    tag = "%s:%dx%d" % ((name,) + shape)
    print("HIPREC wide_instance %s %s %s (%s)" % ((tag,) + ran))
    _check_estimates(one, "%s:%s" % (tag, ran[0]), out["est"], False, "wide_estimate", bound_wide)
    _check_places(one, "%s:%s" % (tag, ran[1]), out, "wide_place", bound=bound_wide)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", WIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", WIDE_INSTANCES, ids=_shape_id)
def test_wide_estimate_weighted(wide, capfd, name, shape, est_k, place_k, order):
    """weighted = 1: every k_estimate_prod instance has a weighted path of its own"""
    one, out, ran = _wide_run(wide, capfd, name, shape, stop_after="estimate", weighted=1)
    _check_estimates(one, "%s:%dx%d:%s" % (name, shape[0], shape[1], ran[0]), out["est"], True, "wide_estimate_weighted", bound_wide)
    assert ran[0] == est_k


@pytest.mark.parametrize("name", WIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", WIDE_INSTANCES, ids=_shape_id)
def test_wide_fixed_root_loglik(wide, capfd, name, shape, est_k, place_k, order):
    """fix_root_loglik = 1: k_root_loglik over regions of up to 3,073 columns"""
    one, out, ran = _wide_run(wide, capfd, name, shape, fix_root_loglik=1)
    _check_places(one, "%s:%dx%d:%s" % (name, shape[0], shape[1], ran[1]), out, "wide_place_fix1", 0, 1, bound_wide)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", WIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", WIDE_INSTANCES, ids=_shape_id)
def test_wide_filter_set_at_the_default_max_error(wide, capfd, name, shape, est_k, place_k, order):
    one, out, ran = _wide_run(wide, capfd, name, shape, max_error=wide(name)[0].max_error)
    got = sorted(int(x) for x in out["cand"]["c_node"][int(out["offs"][0]):int(out["offs"][1])])
    assert got == sorted(int(u) for u, keep in zip(one.seeds, one.filter_in[0]) if keep)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", WIDE_CASES)
@pytest.mark.parametrize("shape,knobs,est_k,place_k,order", WIDE_KNOB_FORMS,
                         ids=["%dx%d-%s" % (w[0] + ("-".join("%s%d" % kv for kv in sorted(w[1].items())),)) for w in WIDE_KNOB_FORMS])
def test_wide_knob_forms(wide, capfd, name, shape, knobs, est_k, place_k, order):
    """the instances that only a comparison knob reaches: pinned like the shipped ones"""
    one, out, ran = _wide_run(wide, capfd, name, shape, knobs=knobs)
    tag = "%s:%dx%d" % ((name,) + shape)
    print("HIPREC wide_instance %s %s %s (%s)" % ((tag,) + ran))
    _check_estimates(one, "%s:%s" % (tag, ran[0]), out["est"], False, "wide_knob_estimate", bound_wide)
    _check_places(one, "%s:%s" % (tag, ran[1]), out, "wide_knob_place", bound=bound_wide)
    assert ran == (est_k, place_k, order)


# ------------------------------------------------------------------------------------------------------------------------------------
# The deep set (tests/golden/hiprec_deep.npz): GTR+4 (mean branch length 0.3) and JC69 (0.15) on 1,024 leaves x 96 columns.  19 / 64 of the
# 64 match columns have a root message below the -510 at which tree_conv, TreeAcc::finish, k_tree_loglik and the packing of messages
# (k = rint(max M / ln 2), the carried exponent of k_estimate_prod / k_place_blk / the streaming kernels) rescale; the all-gap columns
# reach -1,197 / -1,420.  Six reads per database, each with a candidate list of its own (at most 48 nodes, given through
# Batch.get_seed_given), the 50-digit messages of those nodes at three columns.
#
# the oracle's (and, for the messages and the tree loglik, also synth's numpy messages') worst distance from the 50-digit values over both
# databases, measured on the CPU before any kernel ran (tests/test_hiprec_oracle.py, the HIPREC oracle_deep_* lines): what plain double
# arithmetic on the same formulas loses at this depth
ORACLE_DEEP = dict(est_ll=4.9e-15, est_wnr_w=2.0e-14, length=1.4e-11, height=7.9e-13, root_ll=4.9e-15, q_eps=8.1e-12, tree_ll=2.9e-14,
                   msg_level=1.4e-13, msg_shape=9.4e-12)


def bound_deep(key):
    """the wide set's rule: min(project floor, max(the narrow bound, 10 x the CPU's worst distance over the deep set)); the two depth-aware
    message measures (hiprec_cases.level_shape) have no project floor: 10 x the larger of the oracle's and synth's distance"""
    if key in ("msg_level", "msg_shape"):
        return 10.0 * ORACLE_DEEP[key]
    return min(FLOOR[FLOOR_OF[key]], max(TEN_X[key], 10.0 * ORACLE_DEEP[key]))


DEEP_WIDTH = 96


@pytest.fixture(scope="module")
def deep():
    """(case, uploaded database) of a deep case, shared by the tests of this module"""
    held = {}

    def get(name):
        if name not in held:
            c = Case(name, "deep")
            held[name] = (c, _engine().Database.from_synth(c.db))
        return held[name]
    yield get
    for _, D in held.values():
        D.close()


def _deep_run(deep, capfd, name, knobs=None, **kw):
    c, D = deep(name)
    capfd.readouterr()
    out = _run(c, knobs=dict(knobs or {}, trace=1), D=D, **kw)
    return c, out, _instances(capfd.readouterr().err, DEEP_WIDTH)


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_tree_messages_and_loglik(name):
    """k_tree_up / k_tree_down (tree_conv and TreeAcc::finish with scale != 0) and k_tree_loglik on 2,047 nodes"""
    E = _engine()
    import torch
    c = Case(name, "deep")
    db = c.db
    n, L = db.seq.shape
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k else None)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    up = torch.full((n, L, 4), 7.0, dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    seq, h = E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    per, tot = E.tree_loglik(n, L, 0, md, up.data_ptr())
    at = np.ix_(c.msg_nodes, c.msg_cols)
    gu, gd = up.cpu().numpy()[at], down.cpu().numpy()[at]
    assert np.array_equal(seq, db.seq)
    assert (c.up.max(-1) < DEEP_LL).any() and (c.down.max(-1) < DEEP_LL).any() and (c.root_ll < DEEP_LL).sum() >= 16
    worst = dict(height=np.abs(h - c.height).max(), tree_ll=max(_rel(per, c.root_ll).max(), float(_rel(tot, c.root_ll_sum))))
    for key, got, want in (("up", gu, c.up), ("down", gd, c.down)):
        worst[key + "_level"], worst[key + "_shape"] = level_shape(got, want)
        inf = np.isneginf(want)
        worst[key] = (np.abs(got[~inf] - want[~inf]) / np.maximum(np.abs(want[~inf]), 1.0)).max()
    report("deep_tree", name, **worst)
    assert all(np.isfinite(v) for v in worst.values()), worst
    assert max(worst["up_level"], worst["down_level"]) <= bound_deep("msg_level"), worst
    assert max(worst["up_shape"], worst["down_shape"]) <= bound_deep("msg_shape"), worst
    assert worst["up"] <= bound("msg") and worst["down"] <= bound("msg")
    assert worst["tree_ll"] <= bound_deep("tree_ll")
    assert worst["height"] < 1e-14


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_estimate_place_q(deep, capfd, name):
    """k_estimate_prod<2,4>, k_place_blk<4,2,3,0,2> and k_finish as shipped on messages whose exponents are carried"""
    c, out, ran = _deep_run(deep, capfd, name)
    _check_estimates(c, name, out["est"], False, "deep_estimate", bound_deep)
    _check_places(c, name, out, "deep_place", bound=bound_deep)
    assert ran == ("k_estimate_prod<2,4>", "k_place_blk<4,2,3,0,2>", "column order")


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_estimate_weighted(deep, capfd, name):
    c, out, ran = _deep_run(deep, capfd, name, stop_after="estimate", weighted=1)
    _check_estimates(c, name, out["est"], True, "deep_estimate_weighted", bound_deep)
    assert ran[0] == "k_estimate_prod<2,4>"


@pytest.mark.parametrize("name", DEEP_CASES)
@pytest.mark.parametrize("prior,fix", [(1, 0), (0, 1), (1, 1)])
def test_deep_prior_and_fixed_root_loglik(deep, capfd, name, prior, fix):
    """k_root_loglik and the prior term of k_finish: q-values from logliks of -1e4 to -1e5"""
    c, out, ran = _deep_run(deep, capfd, name, prior=prior, fix_root_loglik=fix)
    _check_places(c, name, out, "deep_place_prior%d_fix%d" % (prior, fix), prior, fix, bound_deep)
    assert ran == ("k_estimate_prod<2,4>", "k_place_blk<4,2,3,0,2>", "column order")


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_filter_set_at_the_default_max_error(deep, capfd, name):
    c, out, ran = _deep_run(deep, capfd, name, max_error=deep(name)[0].max_error)
    for ri in range(c.n_reads):
        got = sorted(int(x) for x in out["cand"]["c_node"][int(out["offs"][ri]):int(out["offs"][ri + 1])])
        assert got == sorted(int(u) for u, keep in zip(c.cands(ri), c.filter_in[ri]) if keep), ri
    assert ran == ("k_estimate_prod<2,4>", "k_place_blk<4,2,3,0,2>", "column order")


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_place_var6_instance(deep, capfd, name):
    """place_var = 6: k_place_blk<12,2,1,0,2>, one reciprocal per site"""
    c, out, ran = _deep_run(deep, capfd, name, knobs=dict(place_var=6))
    _check_places(c, name, out, "deep_place_var6", bound=bound_deep)
    assert ran == ("k_estimate_prod<2,4>", "k_place_blk<12,2,1,0,2>", "column order")


@pytest.mark.parametrize("name", DEEP_CASES)
def test_deep_streaming_kernels(deep, capfd, name):
    """the one-wave streaming estimate / place kernels carry the exponent their own way"""
    c, out, ran = _deep_run(deep, capfd, name, knobs=dict(streaming_sep=1), fix_root_loglik=1)
    _check_estimates(c, name, out["est"], False, "deep_estimate_streaming", bound_deep)
    _check_places(c, name, out, "deep_place_streaming", 0, 1, bound_deep)
    assert ran == ("k_estimate", "k_place", "column order")


# ------------------------------------------------------------------------------------------------------------------------------------
# The deepwide set (tests/golden/hiprec_deepwide.npz): the deep set's models and branch lengths on 1,029 leaves x 3,300 columns, 1,200 of them
# match columns, and seven of the wide set's read shapes (DEEPWIDE_READS: one per pair of shipped instances above the 4-site class), each
# with twelve candidates given through Batch.get_seed_given and each in a batch of its own.  Every instance therefore runs on messages whose
# packing exponents are in the thousands, deep and shallow columns side by side among one thread's sites (GTR+4) or deep everywhere (JC69).
# The instance a read must select is the row of WIDE_INSTANCES / WIDE_KNOB_FORMS with its shape: looked up, not copied.
#
# the oracle's worst distance from the 50-digit values over both databases, measured on the CPU before any kernel ran on this set
# (tests/test_hiprec_oracle.py, the HIPREC oracle_deepwide_* lines)
ORACLE_DEEPWIDE = dict(est_ll=2.1e-14, est_wnr_w=4.6e-14, length=5.8e-12, height=5.7e-13, root_ll=1.9e-14, q_eps=2.4e-11)
INSTANCE_OF = {w[0]: w[1:] for w in WIDE_INSTANCES}
DEEPWIDE_INSTANCES = [(shape,) + INSTANCE_OF[shape] for shape in DEEPWIDE_READS]
DEEPWIDE_KNOB_FORMS = [w for w in WIDE_KNOB_FORMS if w[0] in DEEPWIDE_READS]
DEEPWIDE_Q_SHAPES = [(1024, 256), (3072, 500)]                  # the reads whose q complements the archive holds


def bound_deepwide(key):
    """the wide and deep rule: min(project floor, max(the narrow bound, 10 x the CPU's worst distance over the deepwide set))"""
    return min(FLOOR[FLOOR_OF[key]], max(TEN_X[key], 10.0 * ORACLE_DEEPWIDE[key]))


@pytest.fixture(scope="module")
def deepwide():
    """(case, uploaded database, the deep match columns) of a deepwide case, shared by the tests of this module: the upload of 2,057 nodes x
    3,300 columns is the only part that takes seconds.  The columns are found from the rebuilt database's own root message, as the
    generator's deep_setup forms it."""
    held = {}

    def get(name):
        if name not in held:
            c = Case(name, "deepwide")
            db = c.db
            match = (db.seq[db.is_leaf] < 0).mean(0) < 0.5
            root = np.asarray(db.up[0]); mx = root.max(1)
            ll = mx + np.log((np.asarray(db.model.pi)[None, :] * np.exp(root - mx[:, None])).sum(1))
            held[name] = (c, _engine().Database.from_synth(db), match & (ll < DEEP_LL))
        return held[name]
    yield get
    for _, D, _ in held.values():
        D.close()


def _deepwide_run(deepwide, capfd, name, shape, knobs=None, **kw):
    c, D, deep_cols = deepwide(name)
    ri = DEEPWIDE_READS.index(shape)
    # a quietly shallower database fails here: the read holds bases on at least 16 match columns whose root message is rescaled
    assert int((deep_cols & (c.codes[ri] >= 0)).sum()) >= 16
    one = c.one_read(ri)
    assert (ri in c.q_reads) == (shape in DEEPWIDE_Q_SHAPES)
    capfd.readouterr()
    out = _run(one, knobs=dict(knobs or {}, trace=1), D=D, **kw)
    return one, out, _instances(capfd.readouterr().err, shape[0])


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", DEEPWIDE_INSTANCES, ids=_shape_id)
def test_deepwide_estimate_place_q(deepwide, capfd, name, shape, est_k, place_k, order):
    """default knobs: the unweighted estimate, the placement with the constant loglik, q-values where the archive holds them; the (d, N)
    of the given seeds are asserted in _run"""
    one, out, ran = _deepwide_run(deepwide, capfd, name, shape)
    tag = "%s:%dx%d" % ((name,) + shape)
    print("HIPREC deepwide_instance %s %s %s (%s)" % ((tag,) + ran))
    _check_estimates(one, "%s:%s" % (tag, ran[0]), out["est"], False, "deepwide_estimate", bound_deepwide)
    _check_places(one, "%s:%s" % (tag, ran[1]), out, "deepwide_place", bound=bound_deepwide)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", DEEPWIDE_INSTANCES, ids=_shape_id)
def test_deepwide_estimate_weighted(deepwide, capfd, name, shape, est_k, place_k, order):
    one, out, ran = _deepwide_run(deepwide, capfd, name, shape, stop_after="estimate", weighted=1)
    _check_estimates(one, "%s:%dx%d:%s" % (name, shape[0], shape[1], ran[0]), out["est"], True, "deepwide_estimate_weighted", bound_deepwide)
    assert ran[0] == est_k


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", DEEPWIDE_INSTANCES, ids=_shape_id)
def test_deepwide_fixed_root_loglik(deepwide, capfd, name, shape, est_k, place_k, order):
    """fix_root_loglik = 1: k_root_loglik over regions of up to 3,073 rescaled columns; the two q reads with prior HEIGHT as well"""
    for prior in (0, 1) if shape in DEEPWIDE_Q_SHAPES else (0,):
        one, out, ran = _deepwide_run(deepwide, capfd, name, shape, prior=prior, fix_root_loglik=1)
        _check_places(one, "%s:%dx%d:%s" % (name, shape[0], shape[1], ran[1]), out, "deepwide_place_prior%d_fix1" % prior, prior, 1, bound_deepwide)
        assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
@pytest.mark.parametrize("shape,est_k,place_k,order", DEEPWIDE_INSTANCES, ids=_shape_id)
def test_deepwide_filter_set_at_the_default_max_error(deepwide, capfd, name, shape, est_k, place_k, order):
    one, out, ran = _deepwide_run(deepwide, capfd, name, shape, max_error=deepwide(name)[0].max_error)
    got = sorted(int(x) for x in out["cand"]["c_node"][int(out["offs"][0]):int(out["offs"][1])])
    assert got == sorted(int(u) for u, keep in zip(one.cands(0), one.filter_in[0]) if keep)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
@pytest.mark.parametrize("shape,knobs,est_k,place_k,order", DEEPWIDE_KNOB_FORMS,
                         ids=["%dx%d-%s" % (w[0] + ("-".join("%s%d" % kv for kv in sorted(w[1].items())),)) for w in DEEPWIDE_KNOB_FORMS])
def test_deepwide_knob_forms(deepwide, capfd, name, shape, knobs, est_k, place_k, order):
    """the instances that only a comparison knob reaches, on rescaled messages"""
    one, out, ran = _deepwide_run(deepwide, capfd, name, shape, knobs=knobs)
    tag = "%s:%dx%d" % ((name,) + shape)
    print("HIPREC deepwide_instance %s %s %s (%s)" % ((tag,) + ran))
    _check_estimates(one, "%s:%s" % (tag, ran[0]), out["est"], False, "deepwide_knob_estimate", bound_deepwide)
    _check_places(one, "%s:%s" % (tag, ran[1]), out, "deepwide_knob_place", bound=bound_deepwide)
    assert ran == (est_k, place_k, order)


@pytest.mark.parametrize("name", DEEPWIDE_CASES)
def test_deepwide_streaming_kernels(deepwide, capfd, name):
    """streaming_sep = 1 on the (1024, 256) read: the one-wave kernels carry the exponent their own way over 1,024 columns"""
    one, out, ran = _deepwide_run(deepwide, capfd, name, (1024, 256), knobs=dict(streaming_sep=1), fix_root_loglik=1)
    _check_estimates(one, "%s:1024x256:%s" % (name, ran[0]), out["est"], False, "deepwide_estimate_streaming", bound_deepwide)
    _check_places(one, "%s:1024x256:%s" % (name, ran[1]), out, "deepwide_place_streaming", 0, 1, bound_deepwide)
    assert ran == ("k_estimate", "k_place", "column order")
