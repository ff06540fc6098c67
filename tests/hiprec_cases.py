"""Shared by tests/test_hiprec_oracle.py and tests/test_hiprec_gpu.py: tests/golden/hiprec.npz, hiprec_wide.npz, hiprec_deep.npz and
hiprec_deepwide.npz (the floating-point stages in 50-digit arithmetic, written by tests/golden/make_hiprec_golden.py --set narrow / wide /
deep / deepwide) and the rules both files read them by.  The narrow archive holds six models on regions of 1 to 190 columns; the wide one two models on twelve reads of 512 to
3,073 columns, one per width class of the estimate / placement dispatch (WIDE_READS); the deep one two models on 1,024 leaves x 96 columns
with branches long enough that messages lie below the -510 at which the log-space implementations rescale, six reads each with a
candidate list of its own (at most 48 nodes), the messages of those nodes only, and digests in place of the tree and the rows; the
deepwide one the same two models and branch lengths on 1,029 leaves x 3,300 columns (1,200 of them match columns) with seven of the wide
set's read shapes (DEEPWIDE_READS: one per pair of shipped instances above the 4-site class) and twelve candidates per read, stored as
the deep one is (Case.deep) with the root log-likelihood at its three message columns only."""
import hashlib
import os

import numpy as np

from conftest import get_db

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = dict(narrow=os.path.join(GOLDEN, "hiprec.npz"), wide=os.path.join(GOLDEN, "hiprec_wide.npz"), deep=os.path.join(GOLDEN, "hiprec_deep.npz"),
            deepwide=os.path.join(GOLDEN, "hiprec_deepwide.npz"))
CASES = ["GTR4", "TN933", "HKY854", "F810", "K802", "JC690"]
WIDE_CASES = ["GTR4", "JC690"]
DEEP_CASES = ["GTR4", "JC690"]
DEEPWIDE_CASES = ["GTR4", "JC690"]
DEEP_LL = -510.0                                                 # a message whose largest component is below it is rescaled
# (columns, base sites) of read ri of every wide case: what the tests parametrize over (the archive's read_shapes must be this)
WIDE_READS = [(512, 120), (513, 100), (1024, 256), (1024, 257), (1025, 150), (1536, 256), (1400, 257), (1537, 200), (2048, 300),
              (2049, 250), (3072, 500), (3073, 300)]
# (columns, base sites) of read ri of every deepwide case: rows of WIDE_READS
DEEPWIDE_READS = [(1024, 256), (1024, 257), (1536, 256), (1400, 257), (2048, 300), (3072, 500), (3073, 300)]
assert all(r in WIDE_READS for r in DEEPWIDE_READS)
KNIFE_MARGIN, KNIFE_GAP = 1e-6, 1e-9
VARIANTS = {(0, 0): 0, (1, 0): 1, (0, 1): 2, (1, 1): 3}        # (prior, fix_root_loglik) -> index into omp
MAX_Q = 250.0

_ARCS = dict(narrow={}, wide={}, deep={}, deepwide={})
# per-candidate arrays [reads][candidates]
PER_CAND = ("dN", "est_d", "est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll", "pl_outer", "pl_em",
            "pl_a_node", "margin", "state_gap", "margin_cond", "filter_in", "knife")


class Case:
    """one database of the archive: its arrays as attributes, and the synthetic database they were computed on"""

    def __init__(self, name, archive="narrow"):
        _ARC = _ARCS[archive]
        if not _ARC:
            with np.load(GOLD[archive]) as z:
                _ARC.update({k: z[k] for k in z.files})
        self.name, self.archive = name, archive
        self.deep = archive in ("deep", "deepwide")              # digests for the tree and the rows, a candidate list per read
        for k, v in _ARC.items():
            if k.startswith(name + "_"):
                setattr(self, k[len(name) + 1:], v)
        self.ts, self.max_error, self.q_reads = _ARC.get("ts"), float(_ARC["max_error"].ravel()[0]), [int(x) for x in _ARC["q_reads"]]
        self.root_ll_sum = float(self.root_ll_sum.ravel()[0])
        n_leaves, cs_len, n_match = (int(x) for x in _ARC["db_args"])
        model, dg_k = name[:-1], int(name[-1])
        kw = dict(n_match=n_match) if n_match >= 0 else {}
        if self.deep:
            kw["mean_blen"] = float(_ARC["mean_blen"][(DEEP_CASES if archive == "deep" else DEEPWIDE_CASES).index(name)])
        self.db = get_db(n_leaves, cs_len, model, dg_k=dg_k, seed=97, **kw)
        if archive in ("wide", "deepwide"):                      # one read per entry of WIDE_READS / DEEPWIDE_READS, its base sites counted
            shapes = [(int(e - s + 1), int((cd[s:e + 1] >= 0).sum())) for cd, s, e in zip(self.codes, self.start, self.end)]
            assert shapes == (WIDE_READS if archive == "wide" else DEEPWIDE_READS) == [tuple(int(x) for x in r) for r in _ARC["read_shapes"]]
        # the same case: tree, rows and rates are the ones the 50-digit run was given
        if self.deep:                                            # by digest: 2,047 nodes x 96 columns do not fit the size cap of a golden file
            for k, dt in (("parent", np.int32), ("blen", np.float64), ("seq", np.int8)):
                a = np.ascontiguousarray(np.asarray(getattr(self.db, k), dt))
                assert hashlib.sha256(a.tobytes()).digest() == getattr(self, k + "_sha256").tobytes(), k
                setattr(self, k, a)
        assert np.array_equal(self.db.parent, self.parent) and np.array_equal(self.db.blen, self.blen) and np.array_equal(self.db.seq, self.seq)
        self.rates = np.concatenate([[1.0], self.db.dg_r]) if dg_k else np.ones(1)
        self.n_reads = len(self.start)
        # f. knife-edge candidates: the counts and the unweighted wnr are not compared, the lengths only to REL
        # (margin_cond < 1: an EM quantity closer to 1e-5 than a relative error of 1e-14 in p moves it through q = 1 - p — an EM that does
        # not converge halves q until 1 - p has no digits left, and the pass count from there on is the arithmetic's, not the formula's)
        self.knife = (self.margin < KNIFE_MARGIN) | (self.state_gap < KNIFE_GAP) | (self.margin_cond < 1)
        if self.deep:                                            # a candidate list per read: `cand` [reads][W], -1 past the end of a list
            self.knife &= self.cand >= 0
            self._slot = [{int(u): k for k, u in enumerate(row[:n])} for row, n in zip(self.cand, self.n_cand)]

    def cands(self, ri):
        """the candidate nodes of read ri in the order of the per-candidate arrays: every non-root node, or the read's own list (deep)"""
        return self.cand[ri, :int(self.n_cand[ri])] if self.deep else self.seeds

    def slot(self, ri, u):
        """the index of node u in the per-candidate arrays of read ri"""
        return self._slot[ri][int(u)] if self.deep else int(u) - 1

    def one_read(self, ri):
        """the same case with read ri alone (a batch of one read: the kernel instance then depends on that read only)"""
        import copy
        c = copy.copy(self)
        for k in ("codes", "start", "end", "pl_const_ll", "filter_margin") + PER_CAND + (("cand", "n_cand", "_slot") if self.deep else ()):
            setattr(c, k, getattr(self, k)[ri:ri + 1])
        c.n_reads = 1
        c.q_reads = [0] if ri in self.q_reads else []
        if ri in self.q_reads:
            c.omp = self.omp[self.q_reads.index(ri):][:1]
        return c

    def times(self):
        """the branch lengths of P: [len(ts)][1 + dg_k]"""
        return self.ts[:, None] * self.rates[None, :]

    def dist(self, ri, k):
        """cDist of candidate k of read ri as getSeed computes it: d / N in double (NaN for no compared site)"""
        d, N = int(self.dN[ri, k, 0]), int(self.dN[ri, k, 1])
        return float("nan") if N == 0 else float(d) / N

    def ratio_double(self, ri, k):
        """estimateSeq's ratio from the stored counts with the reference's own three double operations (src/PhyloTreeUnrooted.cpp:853-858)"""
        dc, Nc, dp, Np = (int(x) for x in self.dN[ri, k])
        with np.errstate(all="ignore"):
            c = np.float64(dc) / np.float64(Nc); p = np.float64(dp) / np.float64(Np)
            r = c / (c + p)
        return 0.5 if np.isnan(r) else float(r)

    def wnr_unweighted(self, ri, k):
        return float(self.est_d[ri, k]) / float(self.end[ri] - self.start[ri] + 1)

    def placed_height(self, ri, k):
        u = int(self.cands(ri)[k])
        return float(self.height[u] + self.pl_ratio[ri, k] * self.blen[u])

    def q_exact(self, ri, prior, fix):
        """(q_place, q_taxon, 1 - p_place, 1 - p_taxon) [n_cand] of read ri (one of q_reads) from the exact complements"""
        omp = self.omp[self.q_reads.index(ri), :len(self.cands(ri)), VARIANTS[(prior, fix)], :]
        with np.errstate(divide="ignore"):
            q = np.minimum(MAX_Q, -10.0 * np.log10(omp))
        return q[:, 0], q[:, 1], omp[:, 0], omp[:, 1]


def q_ok(q, q_exact, omp, eps):
    """the conditioned q bound: |dq| <= (10 / ln 10) eps / (1 - p) + 1e-12 q; where p > 1 - 1e-6 only that both sides give q >= 59.9"""
    if omp < 1e-6:
        return q >= 59.9 and q_exact >= 59.9
    return abs(q - q_exact) <= (10.0 / np.log(10.0)) * eps / omp + 1e-12 * q_exact


def ratio_half(case, ri):
    """a placed ratio within 1e-6 of 0.5 switches the taxon node: the taxon sums of that read are not comparable"""
    return bool((np.abs(case.pl_ratio[ri] - 0.5) < 1e-6).any())


def level_shape(got, want):
    """the depth-aware distance of log-space messages [..., 4] from the exact ones: (level, shape) with level = |max_i got_i - max_i want_i|
    relative to max(|max_i want_i|, 1) and shape = max over the finite components of |(got_i - max got) - (want_i - max want)|, absolute.
    |dM| / max(|M|, 1) alone allows 1.6e-8 in the linear value at |M| = 900; the shape is the linear value's relative error.  The -inf
    pattern must be equal."""
    got = np.asarray(got, float); want = np.asarray(want, float)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf) and np.isfinite(got[~inf]).all()
    gm, wm = got.max(-1), want.max(-1)
    level = (np.abs(gm - wm) / np.maximum(np.abs(wm), 1.0)).max()
    d = np.abs((got - gm[..., None]) - (want - wm[..., None]))
    return float(level), float(d[~inf].max())
