"""Regenerates tests/golden/hiprec.npz, hiprec_wide.npz, hiprec_deep.npz and hiprec_deepwide.npz: the floating-point stages of the per-read
task in 50-digit arithmetic.

    python tests/golden/make_hiprec_golden.py [--set narrow|wide|deep|deepwide] [--out PATH] [--workers N]

A second derivation, independent of oracle/ and of the engine: it is written from the reference's source (cited as file:line below)
and the mathematics, imports neither, and works in LINEAR space with mpmath (mp.dps = 50) where both of them work in log space with
the reference's -510 scaling rule (src/PhyloTreeUnrooted.h:1495-1510) — at 50 digits with an unbounded exponent that rule is a no-op.
hmmufotu_amd.synth supplies DATA only: the tree (parent, blen), the leaf rows, the model parameters and the discrete-Gamma rates.
Every float64 input is taken as the exact number it is; every stored value is the float64 rounding of the 50-digit result.

Contents, per database CASE (key prefix "<model><dg_k>_"):
  a. P(t) = expm(Q t) of the model's rate matrix Q at t in TS, each also multiplied by the database's dGamma rates.
  c. the messages of every directed edge at MSG_COLS columns — the fewest, a median number and the most leaf gaps; all 200 would not
     fit the size cap of a golden file (no file there is larger than 170 KB, this one is to stay below) —, the root
     log-likelihood of EVERY column and its serial sum.
  d. seven aligned reads (make_reads: codes, start, end) and the seed list (every non-root node).
  e. per read and non-root node: estimateSeq unweighted / weighted, placeSeq (joint EM from the unweighted estimate), the F4 constant,
     the intended root loglik; filterPlacements membership at maxError = 20; for the reads of Q_READS the exact complements 1 - p of
     calcQValues' posteriors (q = min(250, -10 log10(1 - p)) is left to the reader: float64(1 - p) keeps every digit where p -> 1)
     for prior UNIFORM / HEIGHT with and without the fixed root loglik.
  f. decision margins: per candidate the smallest relative distance of a convergence quantity from BRANCH_EPS, the same distance
     of the EM quantities in units of what double precision leaves of them (class Margin), and the smallest gap between the two best
     inferred-state components; per read the smallest distance of a filter gap from 20.
The run fails if more than 5 % of a database's candidates are knife-edge (margin < 1e-6, conditioned margin < 1 or state gap < 1e-9)
or a filter gap lies within 1e-6 of 20: change READ_SEED then, not the caps.

--set wide (hiprec_wide.npz) is the same mathematics on the widths the product runs: two databases of 8 leaves x 3,300 columns (GTR with 4
rate categories, JC69 without dGamma) and twelve reads each (WIDE_READS: a leaf's row with 3 % substitutions, `bases` base sites in a
region of `cols` columns, every other site a gap), one per width class of the estimate / placement dispatch; per candidate the same values
as above, q complements for three reads.  To stay under the size cap it holds the messages and the per-column root log-likelihood at the
MSG_COLS columns only (and the serial sum over all columns), and no P(t) block.  It costs about 65 CPU-minutes (9 minutes with 8 workers).  The conditions above hold for it with its own read seed.

--set deep (hiprec_deep.npz) is the same mathematics where the two log-space implementations rescale: messages below -510
(src/PhyloTreeUnrooted.h:1495-1510), which no message of the other two sets comes near.  Two databases of 1,024 leaves x 96 columns, 64 of
them match columns: GTR with 4 rate categories at a mean branch length of 0.3 (19 match columns with a root message below -510, the lowest
-766; 45 above it, the highest -44), and JC69 without dGamma at 0.15 (all 64 below, the lowest -963).  The 32 all-gap columns lie lower
still (-1,197 / -1,420).  Asserted from the 50-digit messages themselves (change the database arguments if one fails, not the
conditions): at least 16 match columns with a root message below -510; no message whose finite components are 200 nats or more apart (the
largest spread is 19.3, so no component underflows under the reference's rule and the exact value is what that rule is meant to compute);
every inner row of the data the argmax of the exact message.
  Reads (make_deep_reads), six per database, all within the 96 columns: the whole width (a leaf with 3 % substitutions; on GTR+4 it holds
  bases on at least 5 deep and 5 other match columns, asserted: 18 and 45), 80 columns equal to a leaf, 65 columns all gaps but the two
  ends, 90 columns 30 % diverged, one deep match column, and two neighbouring columns of which one is a deep match column and the other is
  not deep (JC69 has no such column: there both are deep match columns).  The columns of the two short reads are chosen with synth's float64
  root message and asserted against the 50-digit one.
  Candidates (cand_nodes), at most 48 per read and from the tree alone: every ancestor of the read's leaf up to a child of the root, their
  siblings (so both children of the root), and four leaves of the other root subtree.  Asserted per read: the list holds a leaf, a branch
  with only `down` below -510 at a column of the read, and -- for the four reads wider than two columns -- a branch with `up` and `down`
  both below -510 at one column (up + down of a column is about its root message, so this happens at all-gap columns only, which the
  two short reads do not hold).
  Stored: per read and candidate what the other archives hold (`cand` [reads][W] names the nodes, -1 past the end of a list), the q
  complements for two reads, the messages of the candidate nodes alone (msg_nodes) at the MSG_COLS columns with the lowest, a median and
  the highest root message, the root log-likelihood of all 96 columns and its serial sum, the heights; SHA-256 digests of parent / blen /
  seq in place of the arrays (2,047 x 96 rows do not fit the size cap), which tests/hiprec_cases.py compares with the database it rebuilds.
  `up` is swept over all 2,047 nodes, `down` over the candidates and their ancestors, by column chunks in parallel.
  On a deep tree a one-column read that differs from a candidate sends q = 1 - p of the 2-node EM below 1e-50 within the 100 passes (em2
  then takes the same number without the cancellation), and a one-hot message against another base at length 0 makes the length infinite
  in exact arithmetic too (the reference runs its passes out on log 0 and takes the cap: stored as the cap, knife-edge).  With the read
  seed in use (2681) 0 of 180 (GTR+4) and 7 of 164 (JC69, 4.3 %) candidates are knife-edge.  Measured cost: 155 CPU-seconds, 27 s of wall
  time with 8 workers (21 s of them the message sweeps).

--set deepwide (hiprec_deepwide.npz) is the deep set at the wide set's width: what every production read is.  GTR with 4 rate categories at
a mean branch length of 0.3 and JC69 without dGamma at 0.15, on 1,029 leaves x 3,300 columns of which 1,200 are match columns.  Two
database arguments differ from the deep and the wide set's, both because a condition below cannot hold otherwise.  With 1,024 leaves the
children of the root hold 735 and 289 leaves, and among a read's twelve candidates no branch then has `up` and `down` both below -510 (up +
down of a column is about its root message, -1,204 / -1,420 at the lowest: the subtree must hold 42 to 58 % of the leaves); with 1,029
leaves they hold 534 and 495.  With the default 601 match columns a read of 256 base sites holds bases on about 47 of them, and under
GTR+4 a column is deep by its rate category, one in four at any branch length: about 11 deep columns per read, never 16 for all seven.
  Asserted from the 50-digit values (change READ_SEED or the database arguments if one fails, not the conditions): 301 (GTR+4) and 1,200
  (JC69) match columns with a root message below -510 (the lowest -841 / -986, the highest of a match column -41 / -777; the lowest of any
  column -1,208 / -1,427); the largest spread between the finite components of a message 17.7 nats (below 200); every inner row the argmax of
  the exact message.
  Reads (DEEPWIDE_READS), seven per database, made exactly as make_wide_reads makes them: (columns, base sites) = (1024, 256), (1024, 257),
  (1536, 256), (1400, 257), (2048, 300), (3072, 500), (3073, 300), one per pair of shipped estimate / placement instances above the 4-site
  class.  Asserted per read: bases on at least 16 match columns with a root message below -510 and, on GTR+4, on at least 16 above it
  (GTR+4: 21 to 40 deep and 59 to 136 other; JC69: 82 to 175 deep).
  Candidates (cand_nodes(short=True)), twelve per read and from the tree alone, a prefix and a suffix of the deep set's list: the read's
  leaf, its sibling and the next three ancestors each with its sibling; the two children of the root; the two lowest-numbered leaves of the
  other root subtree (fewer under a shallow leaf, never fewer than 8).  Asserted per read, as for the deep set: a leaf, a branch with only
  `down` below -510 at a column of the read, a branch with `up` and `down` both below -510 at one column.
  Stored as the deep archive is: digests of parent / blen / seq, `cand` / `n_cand`, every per-candidate value, the q complements for the
  (1024, 256) and the (3072, 500) read, both messages of the 62 candidate nodes at the MSG_COLS columns with the lowest, a median and the
  highest root message, the root log-likelihood at those three columns and its serial sum over all 3,300, the heights, `read_shapes`.
  The sweeps run by column chunks of at least 64 columns (16 chunks per database with 8 workers).  A subtree whose leaves are all gaps at a
  column sends the same message at every such column, so that message is formed once per node and chunk and shared (the same operations on
  the same numbers: the deep archive is reproduced byte for byte); at a sparse column of 1,029 leaves only the ancestors of the one or two
  leaves with a base are left.  With the read seed in use (2711) none of the 2 x 84 candidates is knife-edge.  Measured cost: 21.4
  CPU-minutes, 3 minutes 12 s of wall time with 8 workers.

The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
from __future__ import annotations

import argparse
import hashlib
import io
import multiprocessing
import os
import sys
import zipfile

import numpy as np
from mpmath import mp, mpf, matrix, expm, eigsy

mp.dps = 50

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [("GTR", 4), ("TN93", 3), ("HKY85", 4), ("F81", 0), ("K80", 2), ("JC69", 0)]
DB_ARGS = dict(n_leaves=16, cs_len=200, n_match=120)           # synth.make_db(16, 200, model, dg_k, n_match=120), default seed
TS = [0.0, 1e-5, 1e-3, 0.05, 1.0, 10.0]
MSG_COLS = 3                                                     # message columns stored per database (chosen in db_state)
READ_SEED = 2029
Q_READS = (2, 4, 5, 6)                                           # reads whose q-value posteriors are stored (the size cap again)
GAP = -2
BRANCH_EPS = mpf(1e-5)                                           # src/PhyloTreeUnrooted.cpp:71 (the double 1e-5)
MAX_ITER = 100                                                   # src/PhyloTreeUnrooted.h:1381
MAX_ERROR = 20.0
KNIFE_MARGIN, KNIFE_GAP, KNIFE_CAP, FILTER_MARGIN = 1e-6, 1e-9, 0.05, 1e-6
# the case sets: db_state, make_reads and assemble take one of them
NARROW = dict(name="narrow", out="hiprec.npz", cases=CASES, db_args=DB_ARGS, read_seed=READ_SEED, q_reads=Q_READS)
# --set wide: regions of 512 to 3,073 columns, one read per width class of the estimate / placement dispatch
WIDE_READS = [(512, 120), (513, 100), (1024, 256), (1024, 257), (1025, 150), (1536, 256), (1400, 257), (1537, 200), (2048, 300),
              (2049, 250), (3072, 500), (3073, 300)]                # (columns, base sites) of each read
WIDE = dict(name="wide", out="hiprec_wide.npz", cases=[("GTR", 4), ("JC69", 0)], db_args=dict(n_leaves=8, cs_len=3300, n_match=None),
            read_seed=2031, q_reads=(2, 5, 10))                     # q-values for (1024, 256), (1536, 256) and (3072, 500)
# --set deep: 1,024 leaves x 96 columns with long branches, so that messages lie below the -510 at which both log-space implementations rescale
DEEP = dict(name="deep", out="hiprec_deep.npz", cases=[("GTR", 4), ("JC69", 0)], db_args=dict(n_leaves=1024, cs_len=96, n_match=64),
            mean_blen=(0.3, 0.15), read_seed=2681, q_reads=(0, 3))  # q-values for the whole-width and the 30 % diverged read
DEEP_LL = -510                                                   # src/PhyloTreeUnrooted.h:1495-1510: messages below it are rescaled there
DEEP_MIN_COLS, DEEP_MAX_SPREAD, DEEP_MAX_CAND = 16, 200, 48
# --set deepwide: the deep set's tree at the wide set's width, one read per pair of shipped instances above the 4-site class
DEEPWIDE_READS = [(1024, 256), (1024, 257), (1536, 256), (1400, 257), (2048, 300), (3072, 500), (3073, 300)]
DEEPWIDE = dict(name="deepwide", out="hiprec_deepwide.npz", cases=[("GTR", 4), ("JC69", 0)],
                db_args=dict(n_leaves=1029, cs_len=3300, n_match=1200), mean_blen=(0.3, 0.15), read_seed=2711, q_reads=(0, 5),
                read_shapes=DEEPWIDE_READS)                         # q-values for (1024, 256) and (3072, 500)
DEEPWIDE_MIN_CAND, DEEPWIDE_CHUNK = 8, 64
SETS = dict(narrow=NARROW, wide=WIDE, deep=DEEP, deepwide=DEEPWIDE)
A, C, G, T = 0, 1, 2, 3


def case_name(model, dg_k):
    return "%s%d" % (model, dg_k)


# ----------------------------------------------------------------------------- a. models
def build_Q(name, pi, par):
    """rate matrix of each model from its definition; pi / par as floats (exact)"""
    pi = [mpf(float(x)) for x in pi]
    par = [mpf(float(x)) for x in par]
    Q = [[mpf(0)] * 4 for _ in range(4)]
    if name == "GTR":
        # src/GTR.cpp:124-131: Q.col(j) = R.col(j) * pi(j); diagonal = -rowsum; Q = scale(Q) with the DEFAULT pi = Ones()
        # (src/DNASubModel.h:154, src/DNASubModel.cpp:123-126): beta = sum_i Q_ii, Q / -beta
        for i in range(4):
            for j in range(4):
                if i != j:
                    Q[i][j] = par[4 * i + j] * pi[j]
    elif name in ("TN93", "HKY85"):
        # src/TN93.h:99-110,113-154 / src/HKY85.h:111-153: exchange rate beta between any two bases, times kr on A<->G and ky on C<->T
        # (HKY85: kr = ky = kappa); beta is the stored parameter
        if name == "TN93":
            kr, ky, beta = par[0], par[1], par[2]
        else:
            kr = ky = par[0]; beta = par[1]
        for i in range(4):
            for j in range(4):
                if i != j:
                    k = kr if {i, j} == {A, G} else ky if {i, j} == {C, T} else mpf(1)
                    Q[i][j] = beta * k * pi[j]
    elif name == "F81":
        for i in range(4):                                       # src/F81.h:110-118
            for j in range(4):
                if i != j:
                    Q[i][j] = par[0] * pi[j]
    elif name == "K80":
        kappa = par[0]; beta = 1 / (2 * kappa)                   # src/K80.h:98-100,113-118; transversions beta, transitions kappa beta
        for i in range(4):
            for j in range(4):
                if i != j:
                    Q[i][j] = kappa * beta if {i, j} in ({A, G}, {C, T}) else beta
    elif name == "JC69":
        for i in range(4):                                       # src/JC69.h:97-101
            for j in range(4):
                if i != j:
                    Q[i][j] = mpf(1) / 3
    else:
        raise ValueError(name)
    for i in range(4):
        Q[i][i] = -sum(Q[i][j] for j in range(4) if j != i)
    if name == "GTR":
        s = -sum(Q[i][i] for i in range(4))
        Q = [[x / s for x in row] for row in Q]
    return Q


class ModelP:
    """P(t) of a reversible model.  The tables of the archive come from mpmath.expm(Q t); the thousands of P(t) inside the
    branch-length loops come from the spectral form of the same Q, which __init__ holds to expm at every t of TS."""

    def __init__(self, name, pi, par):
        self.pi = [mpf(0.25)] * 4 if name in ("K80", "JC69") else [mpf(float(x)) for x in pi]
        self.Q = build_Q(name, self.pi, par)
        sq = [mp.sqrt(p) for p in self.pi]
        S = matrix(4, 4)
        for i in range(4):
            for j in range(4):
                S[i, j] = (sq[i] * self.Q[i][j] / sq[j] + sq[j] * self.Q[j][i] / sq[i]) / 2      # detailed balance: symmetric
        lam, V = eigsy(S)
        self.lam = [lam[k] for k in range(4)]
        self.L = [[V[i, k] / sq[i] for k in range(4)] for i in range(4)]
        self.R = [[V[j, k] * sq[j] for j in range(4)] for k in range(4)]
        for t in TS:
            for i, row in enumerate(self.expm(mpf(t))):
                assert abs(sum(row) - 1) < mpf(10) ** -40
                for j, x in enumerate(row):
                    assert abs(x - self.P(mpf(t))[i][j]) < mpf(10) ** -40, (name, t)

    def expm(self, t):
        M = expm(matrix(self.Q) * t)
        return [[M[i, j] for j in range(4)] for i in range(4)]

    def P(self, t):
        if t == 0:                                               # exactly I (src/GTR.h:116-121; the closed forms of the others give it too)
            return [[mpf(int(i == j)) for j in range(4)] for i in range(4)]
        e = [mp.exp(l * t) for l in self.lam]
        return [[sum(self.L[i][k] * e[k] * self.R[k][j] for k in range(4)) for j in range(4)] for i in range(4)]


# ----------------------------------------------------------------------------- c. messages (linear space)
def conv(P, m):
    """sum_k P(i -> k) m_k: what dot_product_scaled(Matrix4d, Vector4d) is the logarithm of (src/PhyloTreeUnrooted.h:1495-1503)"""
    return [P[i][0] * m[0] + P[i][1] * m[1] + P[i][2] * m[2] + P[i][3] * m[3] for i in range(4)]


def join(contribs, dg):
    """message of an inner node from incoming (P of every rate category, message) pairs (src/PhyloTreeUnrooted.cpp:320-346): the product
    over the children per category, and with dGamma the plain average over the categories at THIS node (row_mean_exp_scaled,
    src/PhyloTreeUnrooted.h:1521-1529)"""
    K = len(contribs[0][0])
    acc = [mpf(0)] * 4
    for k in range(K):
        prod = [mpf(1)] * 4
        for Pk, m in contribs:
            c = conv(Pk[k], m)
            prod = [prod[i] * c[i] for i in range(4)]
        acc = [acc[i] + prod[i] for i in range(4)]
    return [a / K for a in acc] if dg else acc


def leaf_vec(code, pi):
    """getLeafLoglik (src/PhyloTreeUnrooted.h:1431-1437): the base's unit vector, pi for a gap"""
    return [mpf(1) if i == code else mpf(0) for i in range(4)] if code >= 0 else list(pi)


TIE = mpf(10) ** -40                                             # components closer than this (relative) are equal in exact arithmetic


def argmax4(v):
    """Eigen's maxCoeff(&idx): the first maximum (of components that tie in exact arithmetic, the first)"""
    thr = max(v) * (1 - TIE)
    for i in range(4):
        if v[i] >= thr:
            return i


def flog(x):
    return float("-inf") if x == 0 else float(mp.log(x))


class DbState:
    pass


def db_state(ci, only_read=None, cfg=NARROW):
    """only_read: messages (and what is computed from them) for the columns of that read alone — one_candidate on a wide database"""
    from hmmufotu_amd import synth
    name, dg_k = cfg["cases"][ci]
    db = synth.make_db(cfg["db_args"]["n_leaves"], cfg["db_args"]["cs_len"], name, dg_k, n_match=cfg["db_args"]["n_match"])
    s = DbState()
    s.ci, s.name, s.dg_k = ci, name, dg_k
    s.n, s.L = db.n_nodes, db.cs_len
    s.parent = [int(x) for x in db.parent]
    s.blen = [mpf(float(x)) for x in db.blen]
    s.is_leaf = [bool(x) for x in db.is_leaf]
    s.anno = [int(x) for x in db.anno_id]
    s.rates = [mpf(float(x)) for x in db.dg_r] if dg_k > 0 else [mpf(1)]
    s.model = ModelP(name, db.model.pi, db.model.par)
    pi = s.model.pi
    n, L = s.n, s.L
    s.seq = np.array(db.seq, np.int8)
    s.read_seed = cfg["read_seed"]
    s.reads = make_reads(s) if cfg["name"] == "narrow" else make_wide_reads(s)
    at = range(L) if only_read is None else range(s.reads[only_read][1], s.reads[only_read][2] + 1)
    row = lambda f: [f(j) if j in at else None for j in range(L)]
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[s.parent[i]].append(i)
    Pn = [None] + [[s.model.P(s.blen[i] * r) for r in s.rates] for i in range(1, n)]
    dg = dg_k > 0
    up = [None] * n; down = [None] * n
    for u in range(n - 1, -1, -1):                               # parents are numbered before their children
        if s.is_leaf[u]:
            up[u] = row(lambda j: leaf_vec(int(db.seq[u, j]), pi))
        else:
            up[u] = row(lambda j: join([(Pn[c], up[c][j]) for c in kids[u]], dg))
    for u in range(1, n):
        p = s.parent[u]
        down[u] = row(lambda j: join(([(Pn[p], down[p][j])] if p != 0 else []) + [(Pn[c], up[c][j]) for c in kids[p] if c != u], dg))
    s.up, s.down = up, down
    # ancestral rows: per-site argmax of the node -> parent message (src/PhyloTreeUnrooted.cpp:1085-1093); the data's must be these
    seq = s.seq
    for u in range(n):
        if not s.is_leaf[u]:
            for j in at:                                         # components equal in exact arithmetic (K80 / JC69): any of them
                assert up[u][j][int(db.seq[u, j])] >= max(up[u][j]) * (1 - TIE), "inner row %d of the database is not the argmax of the 50-digit message" % u
    # heights: the smallest distance to a descendant leaf (src/PhyloTreeUnrooted.cpp:274-287)
    h = [None] * n
    for u in range(n - 1, -1, -1):
        h[u] = mpf(0) if s.is_leaf[u] else min(h[c] + s.blen[c] for c in kids[u])
    s.height = h
    # treeLoglik of a column: log(pi . root message) (src/PhyloTreeUnrooted.cpp:707-719)
    s.root_ll = row(lambda j: mp.log(sum(pi[i] * up[0][j][i] for i in range(4))))
    s.root_ll_sum = sum(s.root_ll) if only_read is None else None
    ngap = (seq[np.array(s.is_leaf)] < 0).sum(0)
    s.msg_cols = sorted({int(np.argmin(ngap)), int(np.argmax(ngap)), int(np.argsort(ngap, kind="stable")[L // 2])})
    assert len(s.msg_cols) == MSG_COLS
    return s


# ----------------------------------------------------------------------------- d. reads
def make_reads(s):
    """(codes [L], start, end) x 7: regions of 1, 2, 64 (no gap site), 65 (all gaps but the two ends), 128 (equal to a leaf over its
    region: d = 0), 129 (30 % diverged from every leaf) and 190 columns (a leaf with 3 % substitutions and its gaps).  Both end columns
    of every read hold a base, as an aligned read's do."""
    rng = np.random.default_rng(s.read_seed + s.ci)
    leaves = np.flatnonzero(s.is_leaf)
    L = s.L

    def from_leaf(cols, mut, gaps):
        u = int(leaves[rng.integers(len(leaves))])
        start = int(rng.integers(2, L - cols - 1)); end = start + cols - 1
        at = np.arange(start, end + 1)
        anc = s.seq[s.parent[u], at]
        b = np.where(s.seq[u, at] >= 0, s.seq[u, at], anc).astype(np.int8)
        m = rng.random(cols) < mut
        b[m] = (b[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        if gaps == "leaf":
            g = s.seq[u, at] < 0
            g[0] = g[-1] = False
            b[g] = GAP
        elif gaps == "all":
            b[1:-1] = GAP
        codes = np.full(L, GAP, np.int8)
        codes[at] = b
        return codes, start, end, u

    reads = [from_leaf(1, 0.03, None), from_leaf(2, 0.03, None), from_leaf(64, 0.03, None), from_leaf(65, 0.03, "all")]
    while True:                                                  # equal to a leaf wherever both hold a base
        cd, st, en, u = from_leaf(128, 0.0, "leaf")
        if ((cd[st:en + 1] >= 0) & (s.seq[u, st:en + 1] >= 0)).sum() >= 40:
            both = (cd >= 0) & (s.seq[u] >= 0)
            assert (cd[both] == s.seq[u][both]).all()
            reads.append((cd, st, en, u))
            break
    while True:                                                  # 30 % diverged: no leaf closer than 0.25 over the compared sites
        cd, st, en, u = from_leaf(129, 0.30, "leaf")
        far = True
        for l in leaves:
            both = (cd[st:en + 1] >= 0) & (s.seq[l, st:en + 1] >= 0)
            if both.sum() and (cd[st:en + 1][both] != s.seq[l, st:en + 1][both]).mean() < 0.25:
                far = False
        if far:
            reads.append((cd, st, en, u))
            break
    reads.append(from_leaf(190, 0.03, "leaf"))
    return [(r[0], r[1], r[2]) for r in reads]


def make_wide_reads(s, shapes=WIDE_READS, src=None):
    """(codes [L], start, end) per entry of `shapes` (src: a list that takes each read's leaf), made as tests/test_loads_batched.py makes its reads: a random leaf's row (its
    parent's inferred base where the leaf has a gap) with 3 % substitutions, `bases` base sites, the two ends among them, in a region of
    `cols` columns; every other site a gap"""
    rng = np.random.default_rng(s.read_seed + s.ci)
    leaves = np.flatnonzero(s.is_leaf)
    reads = []
    for cols, bases in shapes:
        u = int(leaves[rng.integers(len(leaves))])
        if src is not None:
            src.append(u)
        start = int(rng.integers(20, s.L - cols - 20)); end = start + cols - 1
        at = np.concatenate([[start, end], start + 1 + rng.choice(cols - 2, size=bases - 2, replace=False)])
        b = np.where(s.seq[u, at] >= 0, s.seq[u, at], s.seq[s.parent[u], at]).astype(np.int8)
        mut = rng.random(len(at)) < 0.03
        b[mut] = (b[mut] + rng.integers(1, 4, size=int(mut.sum()))) % 4
        codes = np.full(s.L, GAP, np.int8)
        codes[at] = b
        reads.append((codes, start, end))
    return reads


# ----------------------------------------------------------------------------- the deep set
_SETUPS = {}


def deep_setup(ci, cfg=DEEP):
    """the data of a deep (or deepwide) case, its reads and their candidate lists; no message yet.  Built once per process and set (a pool
    forked after the first call inherits it); every caller gets a shallow copy to hang its messages on."""
    import copy
    if (cfg["name"], ci) not in _SETUPS:
        _SETUPS[(cfg["name"], ci)] = _deep_setup(ci, cfg)
    return copy.copy(_SETUPS[(cfg["name"], ci)])


def _deep_setup(ci, cfg):
    """The columns of the deep set's two short reads are CHOSEN with synth's float64 root message (data, like the rows); that they are deep
    or not is asserted from the 50-digit values in deep_state."""
    from hmmufotu_amd import synth
    name, dg_k = cfg["cases"][ci]
    da = cfg["db_args"]
    db = synth.make_db(da["n_leaves"], da["cs_len"], name, dg_k, n_match=da["n_match"], mean_blen=cfg["mean_blen"][ci])
    s = DbState()
    s.ci, s.name, s.dg_k = ci, name, dg_k
    s.n, s.L = db.n_nodes, db.cs_len
    s.parent = [int(x) for x in db.parent]
    s.blen = [mpf(float(x)) for x in db.blen]
    s.is_leaf = [bool(x) for x in db.is_leaf]
    s.anno = [int(x) for x in db.anno_id]
    s.rates = [mpf(float(x)) for x in db.dg_r] if dg_k > 0 else [mpf(1)]
    s.model = ModelP(name, db.model.pi, db.model.par)
    s.seq = np.array(db.seq, np.int8)
    s.read_seed = cfg["read_seed"]
    s.digests = {k: hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()
                 for k, a in (("parent", np.asarray(db.parent, np.int32)), ("blen", np.asarray(db.blen, np.float64)), ("seq", s.seq))}
    s.kids = [[] for _ in range(s.n)]
    for i in range(1, s.n):
        s.kids[s.parent[i]].append(i)
    s.match = (s.seq[np.array(s.is_leaf)] < 0).mean(0) < 0.5    # the columns make_db drew as match columns: few leaf gaps
    root = np.asarray(db.up[0]); mx = root.max(1)
    s.ll_synth = mx + np.log((np.asarray(db.model.pi)[None, :] * np.exp(root - mx[:, None])).sum(1))
    if "read_shapes" in cfg:                                     # deepwide: the wide set's reads, twelve candidates each
        s.src = []
        s.reads = make_wide_reads(s, cfg["read_shapes"], s.src)
        s.cands = [cand_nodes(s, u, short=True) for u in s.src]
    else:
        s.reads, s.src = make_deep_reads(s)
        s.cands = [cand_nodes(s, u) for u in s.src]
    s.msg_nodes = sorted(set(u for c in s.cands for u in c))
    need = set()                                                 # down of a node takes its parent's: the candidates and their ancestors
    for u in s.msg_nodes:
        while u != 0 and u not in need:
            need.add(u); u = s.parent[u]
    s.need_down = sorted(need)
    h = [None] * s.n                                             # src/PhyloTreeUnrooted.cpp:274-287
    for u in range(s.n - 1, -1, -1):
        h[u] = mpf(0) if s.is_leaf[u] else min(h[c] + s.blen[c] for c in s.kids[u])
    s.height = h
    return s


def make_deep_reads(s):
    """(codes [L], start, end) x 6 within the 96 columns, made as make_reads makes the narrow ones: the whole width (a leaf with 3 %
    substitutions and its gaps), 80 columns equal to a leaf, 65 columns all gaps but the two ends, 90 columns 30 % diverged, one deep
    match column, and two neighbouring columns of which one is a deep match column and the other is not deep.  Also each read's leaf."""
    rng = np.random.default_rng(s.read_seed + s.ci)
    leaves = np.flatnonzero(s.is_leaf)
    L = s.L

    def from_leaf(cols, mut, gaps, start=None):
        u = int(leaves[rng.integers(len(leaves))])
        if start is None:
            start = int(rng.integers(0, L - cols + 1))
        end = start + cols - 1
        at = np.arange(start, end + 1)
        b = np.where(s.seq[u, at] >= 0, s.seq[u, at], s.seq[s.parent[u], at]).astype(np.int8)
        m = rng.random(cols) < mut
        b[m] = (b[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        if gaps == "leaf":
            g = s.seq[u, at] < 0
            g[0] = g[-1] = False
            b[g] = GAP
        elif gaps == "all":
            b[1:-1] = GAP
        codes = np.full(L, GAP, np.int8)
        codes[at] = b
        return codes, start, end, u

    reads = [from_leaf(L, 0.03, "leaf")]
    while True:                                                  # equal to a leaf wherever both hold a base
        cd, st, en, u = from_leaf(80, 0.0, "leaf")
        both = (cd >= 0) & (s.seq[u] >= 0)
        if both.sum() >= 40:
            assert (cd[both] == s.seq[u][both]).all()
            reads.append((cd, st, en, u))
            break
    reads.append(from_leaf(65, 0.03, "all"))
    while True:                                                  # 30 % diverged: no leaf closer than 0.25 over the compared sites
        cd, st, en, u = from_leaf(90, 0.30, "leaf")
        rows = s.seq[leaves][:, st:en + 1]
        both = (cd[st:en + 1] >= 0)[None, :] & (rows >= 0)
        diff = (both & (rows != cd[st:en + 1][None, :])).sum(1)
        if (diff[both.sum(1) > 0] >= 0.25 * both.sum(1)[both.sum(1) > 0]).all():
            reads.append((cd, st, en, u))
            break
    deep = s.match & (s.ll_synth < DEEP_LL)
    cols = np.flatnonzero(deep)
    reads.append(from_leaf(1, 0.03, None, start=int(cols[rng.integers(len(cols))])))
    # a deep match column next to a column that is not deep: a shallow match column where the database has one, else any other
    # (JC69: every match column is deep and every other column is all gaps, deeper still and without a say in a branch length: there the
    # read takes two deep match columns)
    pairs = [j for j in range(L - 1) if deep[j] != deep[j + 1] and s.ll_synth[j if deep[j + 1] else j + 1] > DEEP_LL]
    pool = pairs or [j for j in range(L - 1) if deep[j] and deep[j + 1]]
    reads.append(from_leaf(2, 0.03, None, start=int(pool[rng.integers(len(pool))])))
    return [(r[0], r[1], r[2]) for r in reads], [r[3] for r in reads]


def cand_nodes(s, leaf, short=False):
    """the candidates of a read from the tree alone: every ancestor of its leaf up to a child of the root (the leaf first), each followed
    by its sibling -- the last pair is the two children of the root --, then the four lowest-numbered leaves of the other root subtree.
    short (deepwide): a prefix and a suffix of that list, twelve nodes -- the leaf, its sibling and the next three ancestors each with its
    sibling; the two children of the root; the first two of the far leaves -- or, under a shallow leaf, what there is of them"""
    out = []
    u = leaf
    while u != 0:
        out.append(u)
        out += [c for c in s.kids[s.parent[u]] if c != u]
        top, u = u, s.parent[u]
    other = [c for c in s.kids[0] if c != top]
    far = []
    for v in range(1, s.n):                                      # preorder numbering: an ancestor has the smaller number
        a = v
        while s.parent[a] != 0:
            a = s.parent[a]
        if s.is_leaf[v] and a in other and v not in out:
            far.append(v)
            if len(far) == 4:
                break
    if short:
        out = out[:8] + [u for u in out[-2:] if u not in out[:8]] + far[:2]
        assert len(out) == len(set(out)) >= DEEPWIDE_MIN_CAND, "fewer than %d candidates: change READ_SEED" % DEEPWIDE_MIN_CAND
        return out
    out += far
    assert len(out) == len(set(out)) <= DEEP_MAX_CAND, "more than %d candidates: change READ_SEED" % DEEP_MAX_CAND
    return out


def deep_sweep(task):
    """the 50-digit messages of one deep case at the columns `cols`: `up` of every node, `down` of the candidates and their ancestors.  Kept:
    both messages of the candidate nodes, the root log-likelihood, and what the conditions of deep_state are asserted from."""
    ci, cols = task[0], task[1]                                  # (case, columns[, set]): the deep set unless the task names another
    s = deep_setup(ci, SETS[task[2]] if len(task) > 2 else DEEP)
    pi, dg = s.model.pi, s.dg_k > 0
    Pn = [None] + [[s.model.P(s.blen[i] * r) for r in s.rates] for i in range(1, s.n)]
    up = [None] * s.n; down = {}
    spread = mpf(0)

    def see(m):
        pos = [x for x in m if x > 0]
        return mp.log(max(pos)) - mp.log(min(pos))
    # A subtree whose leaves are all gaps at a column sends the same message at every such column: formed once per node, by the same
    # operations on the same numbers, and shared.  At a sparse column of 1,000 leaves only the ancestors of the one or two leaves with a
    # base are left to compute.
    below = np.zeros((s.n, len(cols)), bool)                     # [node][k]: every leaf under it is a gap at cols[k]
    gap_up = [None] * s.n; gap_spread = [None] * s.n; gap_arg = {}
    for u in range(s.n - 1, -1, -1):                             # parents are numbered before their children
        if s.is_leaf[u]:
            below[u] = s.seq[u, cols] < 0
            gap_up[u] = leaf_vec(GAP, pi)
            up[u] = {j: gap_up[u] if below[u, k] else leaf_vec(int(s.seq[u, j]), pi) for k, j in enumerate(cols)}
        else:
            below[u] = np.logical_and.reduce([below[c] for c in s.kids[u]])
            gap_up[u] = join([(Pn[c], gap_up[c]) for c in s.kids[u]], dg)
            up[u] = {j: gap_up[u] if below[u, k] else join([(Pn[c], up[c][j]) for c in s.kids[u]], dg) for k, j in enumerate(cols)}
            for k, j in enumerate(cols):                         # components equal in exact arithmetic (JC69): any of them
                code = int(s.seq[u, j])
                if below[u, k] and (u, code) not in gap_arg:
                    gap_arg[(u, code)] = gap_up[u][code] >= max(gap_up[u]) * (1 - TIE)
                ok = gap_arg[(u, code)] if below[u, k] else up[u][j][code] >= max(up[u][j]) * (1 - TIE)
                assert ok, "inner row %d of the database is not the argmax of the 50-digit message" % u
        gap_spread[u] = see(gap_up[u]) if below[u].any() else mpf(0)
        spread = max([spread, gap_spread[u]] + [see(up[u][j]) for k, j in enumerate(cols) if not below[u, k]])
    for u in s.need_down:
        p = s.parent[u]
        down[u] = {j: join(([(Pn[p], down[p][j])] if p != 0 else []) + [(Pn[c], up[c][j]) for c in s.kids[p] if c != u], dg) for j in cols}
        spread = max([spread] + [see(down[u][j]) for j in cols])
    return dict(ci=ci, cols=list(cols), spread=spread, up={u: up[u] for u in s.msg_nodes + [0]}, down={u: down[u] for u in s.msg_nodes},
                root_ll={j: mp.log(sum(pi[i] * up[0][j][i] for i in range(4))) for j in cols})


def deep_state(ci, parts, cfg=DEEP):
    """the state that candidate() reads, from the sweeps of one deep case (all columns, or those of one read), and its conditions"""
    s = deep_setup(ci, cfg)
    wide = "read_shapes" in cfg
    whole = sorted(j for p in parts for j in p["cols"]) == list(range(s.L))
    s.up = [None] * s.n; s.down = [None] * s.n
    s.root_ll = [None] * s.L
    for p in parts:
        for side, dst in ((p["up"], s.up), (p["down"], s.down)):
            for u, by_col in side.items():
                if dst[u] is None:
                    dst[u] = [None] * s.L
                for j, m in by_col.items():
                    dst[u][j] = m
        for j, x in p["root_ll"].items():
            s.root_ll[j] = x
    spread = max(p["spread"] for p in parts)
    assert spread < DEEP_MAX_SPREAD, "a message with components %s nats apart: change the database arguments" % spread
    low = lambda m: mp.log(max(m)) < DEEP_LL
    rd = lambda ri: range(s.reads[ri][1], s.reads[ri][2] + 1)
    for ri, (codes, st, en) in enumerate(s.reads):               # the three kinds of branch the list is to hold, at columns that are here
        at = [j for j in rd(ri) if s.root_ll[j] is not None]
        kinds = dict(both=any(low(s.up[u][j]) and low(s.down[u][j]) for u in s.cands[ri] for j in at),
                     down_only=any(low(s.down[u][j]) and not low(s.up[u][j]) for u in s.cands[ri] for j in at),
                     leaf=any(s.is_leaf[u] for u in s.cands[ri]))
        s.kinds = getattr(s, "kinds", []) + [kinds]
        # up + down of one column is about its root message, -1,420 at the lowest: both are below -510 only at an all-gap column, which
        # the two short reads do not hold
        assert not whole or (kinds["leaf"] and kinds["down_only"] and (kinds["both"] or en - st < 2)), "read %d: %s: change READ_SEED" % (ri, kinds)
    if wide:
        assert [(en - st + 1, int((cd[st:en + 1] >= 0).sum())) for cd, st, en in s.reads] == cfg["read_shapes"]
    else:
        j1 = s.reads[4][1]; j2 = s.reads[5][1]
        is_deep = lambda j: bool(s.match[j] and s.ll_synth[j] < DEEP_LL)
        assert is_deep(j1) and (is_deep(j2) != is_deep(j2 + 1) or (s.ll_synth < DEEP_LL).all())
        for j in (j1, j2, j2 + 1):                               # what the columns were chosen by holds for the 50-digit values
            if s.root_ll[j] is not None:
                assert (s.root_ll[j] < DEEP_LL) == bool(s.ll_synth[j] < DEEP_LL), "column %d: synth's root message and the 50-digit one differ about -510" % j
    if not whole:
        s.root_ll_sum = None
        return s
    s.root_ll_sum = sum(s.root_ll)
    deep_cols = [j for j in range(s.L) if s.match[j] and s.root_ll[j] < DEEP_LL]
    assert len(deep_cols) >= DEEP_MIN_COLS, "%d deep match columns: change the database arguments" % len(deep_cols)
    if wide:
        return deepwide_conditions(s, deep_cols, spread)
    on0 = [j for j in range(s.L) if s.match[j] and s.reads[0][0][j] >= 0]
    n_deep0 = sum(1 for j in on0 if s.root_ll[j] < DEEP_LL)
    if s.dg_k > 0:                                               # deep and shallow columns side by side under one read
        assert n_deep0 >= 5 and len(on0) - n_deep0 >= 5, (n_deep0, len(on0))
    order = sorted(range(s.L), key=lambda j: (s.root_ll[j], j))
    s.msg_cols = sorted({order[0], order[s.L // 2], order[-1]})  # the lowest, a median and the highest root message
    assert len(s.msg_cols) == MSG_COLS
    print("%-7s %d of %d match columns below %d at the root (lowest %.1f; lowest of any column %.1f), largest spread %.1f nats, "
          "the whole-width read on %d deep and %d other match columns, %d message nodes" %
          (case_name(s.name, s.dg_k), len(deep_cols), int(s.match.sum()), DEEP_LL, float(min(s.root_ll[j] for j in deep_cols)),
           float(min(s.root_ll)), float(spread), n_deep0, len(on0) - n_deep0, len(s.msg_nodes)), flush=True)
    return s


def deepwide_conditions(s, deep_cols, spread):
    """what deep_state asserts of a deepwide case beyond the deep set's conditions: every read holds bases on at least DEEP_MIN_COLS match
    columns with a root message below -510 and, with dGamma, on as many above it: deep and shallow columns side by side in one region"""
    counts = []
    for ri, (codes, st, en) in enumerate(s.reads):
        on = [j for j in range(st, en + 1) if s.match[j] and codes[j] >= 0]
        n_deep = sum(1 for j in on if s.root_ll[j] < DEEP_LL)
        assert n_deep >= DEEP_MIN_COLS, "read %d: bases on %d deep match columns: change READ_SEED or the database arguments" % (ri, n_deep)
        if s.dg_k > 0:
            assert len(on) - n_deep >= DEEP_MIN_COLS, "read %d: bases on %d other match columns: change READ_SEED or the database arguments" % (ri, len(on) - n_deep)
        counts.append("%d+%d" % (n_deep, len(on) - n_deep))
    order = sorted(range(s.L), key=lambda j: (s.root_ll[j], j))
    s.msg_cols = sorted({order[0], order[s.L // 2], order[-1]})  # the lowest, a median and the highest root message
    assert len(s.msg_cols) == MSG_COLS
    print("%-7s %d of %d match columns below %d at the root (lowest %.1f, highest of any match column %.1f; lowest of any column %.1f), "
          "largest spread %.1f nats, reads on deep+other match columns %s, candidates per read %s, %d message nodes" %
          (case_name(s.name, s.dg_k), len(deep_cols), int(s.match.sum()), DEEP_LL, float(min(s.root_ll[j] for j in deep_cols)),
           float(max(s.root_ll[j] for j in range(s.L) if s.match[j])), float(min(s.root_ll)), float(spread), " ".join(counts),
           [len(c) for c in s.cands], len(s.msg_nodes)), flush=True)
    return s


# ----------------------------------------------------------------------------- e. one candidate
def pdist_counts(a, b, start, end):
    """SeqUtils::pDist (src/SeqUtils.cpp:37-54): sites where both hold a base, and those of them that differ"""
    both = (a[start:end + 1] >= 0) & (b[start:end + 1] >= 0)
    return int((a[start:end + 1][both] != b[start:end + 1][both]).sum()), int(both.sum())


class Margin:
    """m: the smallest relative distance of a convergence quantity from BRANCH_EPS.  cond: the smallest distance of an EM quantity
    |log q - log q0| from BRANCH_EPS in units of what a relative error of P_ERR in p does to it through q = 1 - p, P_ERR (1/q + 1/q0):
    an EM that does not converge halves q pass after pass until 1 - p has no digits left, and from there on the pass count is the
    arithmetic's (q sticks at 2^-53 and the test reads 0, or q reaches 0 and it reads NaN), not the formula's."""
    P_ERR = mpf("1e-14")                                         # ~100 ulp: a reciprocal refined by one Newton step from 2^-23

    def __init__(self):
        self.m = mpf(1)
        self.cond = mp.inf

    def see(self, x, q=None, q0=None):
        self.m = min(self.m, abs(x - BRANCH_EPS) / BRANCH_EPS)
        if q is not None:
            self.cond = min(self.cond, abs(x - BRANCH_EPS) / (self.P_ERR * (1 / q + 1 / q0)))


def em2(pi, Um, Vm, w0, max_l, mg, deep=False):
    """the 2-node EM of src/PhyloTreeUnrooted.cpp:749-798 on linear messages: A = pi . (U o V), B = (pi . U)(pi . V) per site.  A site is
    skipped there when logA or logB is NaN; with messages that are not all zero neither can be (asserted).  Returns (w, passes)."""
    q0 = mp.exp(-w0); p0 = 1 - q0
    AB = []
    for a, b in zip(Um, Vm):
        Aj = sum(pi[i] * a[i] * b[i] for i in range(4))
        Bj = sum(pi[i] * a[i] for i in range(4)) * sum(pi[i] * b[i] for i in range(4))
        assert Bj > 0
        AB.append((Aj, Bj))
    n = len(AB)
    p, q, steps = p0, q0, 0
    it = 0
    while it < MAX_ITER and 0 <= p <= 1:
        steps += 1
        p = sum(Bj * p0 / (Aj * q0 + Bj * p0) for Aj, Bj in AB) / n
        q = 1 - p
        if q == 0 and deep:                                      # the same number without the cancellation: on a deep tree a one-column read
            q = sum(Aj * q0 / (Aj * q0 + Bj * p0) for Aj, Bj in AB) / n      # that differs from a leaf sends q below 1e-50 within the 100 passes
        if q == 0 and deep:                                      # every A is 0 (a one-hot message against another base at length 0): the length is
            mg.cond = mpf(0)                                     # infinite in exact arithmetic too; the reference runs its passes out on log(0) and
            return max_l, MAX_ITER                               # takes the cap.  Knife-edge: the pass count is not compared
        assert q > 0, "a branch length ran to infinity: choose other reads"
        x = abs(mp.log(q) - mp.log(q0))
        mg.see(x, q, q0)
        if x < BRANCH_EPS:
            break
        p0, q0 = p, q
        it += 1
    w = -mp.log(q)
    return (max_l if w > max_l else w), steps


def candidate(s, ri, u):
    """everything the archive holds for read ri on the branch above node u, as a dict of floats / ints"""
    codes, start, end = s.reads[ri]
    v = s.parent[u]
    pi, M = s.model.pi, s.model
    n = end - start + 1
    cols = range(start, end + 1)
    U = [s.up[u][j] for j in cols]; V = [s.down[u][j] for j in cols]
    N = [leaf_vec(int(codes[j]), pi) for j in cols]
    out = {}
    # ---- estimateSeq (src/PhyloTreeUnrooted.cpp:849-877)
    dc, Nc = pdist_counts(s.seq[u], codes, start, end)
    dp, Np = pdist_counts(s.seq[v], codes, start, end)
    out["dN"] = (dc, Nc, dp, Np)
    if Nc == 0 or Np == 0 or dc * Np + dp * Nc == 0:
        ratio = mpf(1) / 2                                       # cDist / (cDist + pDist) is NaN
    else:
        ratio = (mpf(dc) / Nc) / (mpf(dc) / Nc + mpf(dp) / Np)
    w0 = s.blen[u]
    wur = w0 * ratio; wvr = w0 - wur
    Pu, Pv = M.P(wur), M.P(wvr)                                  # model->Pr(wur): no rate categories here
    R = [[a * b for a, b in zip(conv(Pu, U[j]), conv(Pv, V[j]))] for j in range(n)]
    d = 0; dw = mpf(0); Nw = mpf(0); gap = mp.inf
    for j in range(n):                                           # src/PhyloTreeUnrooted.cpp:1018-1052
        b1, b2 = argmax4(R[j]), argmax4(N[j])
        srt = sorted(R[j], reverse=True)
        if srt[3] < srt[0] * (1 - TIE):                          # four equal components: the first wins on any arithmetic
            gap = min(gap, mp.log(srt[0]) - mp.log(srt[1]) if srt[1] > 0 else mp.inf)
        w = (R[j][b1] / sum(R[j])) * (N[j][b2] / sum(N[j]))
        if b1 != b2:
            d += 1; dw += w
        Nw += w
    out["est_d"] = d
    wnr_u = mpf(d) / n; wnr_w = dw / Nw

    def est_ll(wnr):
        Pn = M.P(wnr)
        tot = mpf(0); neg_inf = False
        for j in range(n):
            x = sum(pi[i] * R[j][i] * c for i, c in enumerate(conv(Pn, N[j])))
            if x == 0:
                neg_inf = True
            else:
                tot += mp.log(x)
        return mpf("-inf") if neg_inf else tot
    ll_u, ll_w = est_ll(wnr_u), est_ll(wnr_w)
    out.update(est_ratio=float(ratio), est_wnr_w=float(wnr_w), est_ll=float(ll_u), est_ll_w=float(ll_w),
               state_gap=float(gap) if gap != mp.inf else np.inf)
    # ---- placeSeq: copySubTree, the new root r on the branch, the joint EM (src/PhyloTreeUnrooted.cpp:879-954, 800-847)
    dg = s.dg_k > 0
    catP = lambda t: [M.P(t * r) for r in s.rates]               # loglikConv(child, j, dG->rate(k)) (src/PhyloTreeUnrooted.cpp:315-318)
    lenUR = w0 * ratio; lenVR = w0 * (1 - ratio); lenNR = wnr_u
    w0j = lenUR + lenVR
    wur0, wnr0 = lenUR, lenNR
    wur = lenUR
    mg = Margin()
    deep = hasattr(s, "cands")
    outer = em = 0
    it = 0
    while it < MAX_ITER and 0 <= wur <= w0j:
        outer += 1
        PU, PV = catP(lenUR), catP(lenVR)
        RN = [join([(PU, U[j]), (PV, V[j])], dg) for j in range(n)]
        wnr, k = em2(pi, RN, N, lenNR, mpf(1), mg, deep); em += k
        lenNR = wnr
        PN = catP(lenNR)
        RU = [join([(PV, V[j]), (PN, N[j])], dg) for j in range(n)]
        wur, k = em2(pi, RU, U, lenUR, w0j, mg, deep); em += k
        lenUR = wur
        lenVR = w0j - wur
        a, b = abs(wur - wur0), abs(wnr - wnr0)
        mg.see(a); mg.see(b)
        if a < BRANCH_EPS and b < BRANCH_EPS:
            break
        wur0, wnr0 = wur, wnr
        it += 1
    pl_ratio = lenUR / w0
    height = s.height[u] + lenUR
    a_node = u if pl_ratio <= mpf(1) / 2 else v                  # max_height = inf (src/PhyloTreeUnrooted.cpp:949-952)
    # the value placeSeq returns: the root message is left at INVALID_LOGLIK = 1 (src/PhyloTreeUnrooted.cpp:918-922), so
    # treeLoglik sums log(sum_i pi_i e^1) over the region
    const_ll = n * mp.log(sum(pi) * mp.e)
    # --fix-root-loglik: loglik(r, j) from the three children at the optimised lengths (src/PhyloTreeUnrooted.cpp:320-346)
    PU, PV, PN = catP(lenUR), catP(w0j - lenUR), catP(lenNR)
    root_ll = sum(mp.log(sum(pi[i] * x for i, x in enumerate(join([(PU, U[j]), (PV, V[j]), (PN, N[j])], dg)))) for j in range(n))
    anno_dist = (w0 * pl_ratio + lenNR) if a_node == u else ((1 - pl_ratio) * w0 + lenNR)       # src/PhyloTreeUnrooted.h:464-467
    log_prior_height = -(anno_dist - lenNR + height)             # src/PhyloTreeUnrooted.cpp:1166-1177
    out.update(pl_ratio=float(pl_ratio), pl_wnr=float(lenNR), pl_outer=outer, pl_em=em, pl_a_node=a_node, pl_root_ll=float(root_ll),
               pl_const_ll=float(const_ll), margin=float(mg.m), margin_cond=float(min(mg.cond, mpf(10) ** 30)))
    out["_q"] = (ll_u, const_ll, root_ll, log_prior_height, s.anno[a_node])
    return out


def q_complements(cands):
    """calcQValues (src/HmmUFOtu_main.cpp:182-216) over one read's candidates: 1 - p of every placement and of its taxon, for
    (prior, fixed root) in (U,0) (H,0) (U,1) (H,1) -> [n][4][2]"""
    out = np.zeros((len(cands), 4, 2))
    for vi, (prior, fix) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        lp = [(c["_q"][2] if fix else c["_q"][1]) + (c["_q"][3] if prior else 0) for c in cands]
        mx = max(lp)
        e = [mp.exp(x - mx) for x in lp]
        tot = sum(e)
        for i, c in enumerate(cands):
            out[i, vi, 0] = float(sum(x for k, x in enumerate(e) if k != i) / tot)
            out[i, vi, 1] = float(sum(x for k, x in enumerate(e) if cands[k]["_q"][4] != c["_q"][4]) / tot)
    return out


# ----------------------------------------------------------------------------- driver
_STATES = {}


def _task(t):
    key, ri, u = t
    try:
        return t, candidate(_STATES[key], ri, u)
    except AssertionError as e:
        raise AssertionError("%s (case %d, read %d, node %d)" % (e, key[1], ri, u))


def assemble(states, results, cfg=NARROW):
    """{key: array} of the whole archive"""
    if cfg["name"] in ("deep", "deepwide"):
        return assemble_deep(states, results, cfg)
    wide = cfg["name"] == "wide"
    da = cfg["db_args"]
    arc = {"ts": np.array(TS), "max_error": np.array(MAX_ERROR), "dps": np.array(mp.dps), "read_seed": np.array(cfg["read_seed"]),
           "q_reads": np.array(cfg["q_reads"], np.int32),
           "db_args": np.array([da["n_leaves"], da["cs_len"], -1 if da["n_match"] is None else da["n_match"]], np.int32),
           "cases": np.array([case_name(*c) for c in cfg["cases"]])}
    if wide:                                                     # P(t) is not repeated; (columns, base sites) of every read instead
        del arc["ts"]
        arc["read_shapes"] = np.array(WIDE_READS, np.int32)
    over = []
    for s in states:
        px = case_name(s.name, s.dg_k) + "_"
        nr, nodes = len(s.reads), list(range(1, s.n))
        mult = [mpf(1)] + (s.rates if s.dg_k > 0 else [])
        if not wide:
            arc[px + "P"] = np.array([[[[float(x) for x in row] for row in s.model.expm(mpf(t) * m)] for m in mult] for t in TS])
        arc[px + "parent"] = np.array(s.parent, np.int32)
        arc[px + "blen"] = np.array([float(x) for x in s.blen])
        arc[px + "seq"] = s.seq
        arc[px + "height"] = np.array([float(x) for x in s.height])
        arc[px + "msg_cols"] = np.array(s.msg_cols, np.int32)
        arc[px + "up"] = np.array([[[flog(x) for x in s.up[u][j]] for j in s.msg_cols] for u in range(s.n)])
        arc[px + "down"] = np.array([[[flog(x) for x in s.down[u][j]] if u else [0.0] * 4 for j in s.msg_cols] for u in range(s.n)])
        arc[px + "root_ll"] = np.array([float(s.root_ll[j]) for j in (s.msg_cols if wide else range(s.L))])      # wide: at msg_cols only
        arc[px + "root_ll_sum"] = np.array(float(s.root_ll_sum))
        arc[px + "codes"] = np.stack([r[0] for r in s.reads])
        arc[px + "start"] = np.array([r[1] for r in s.reads], np.int32)
        arc[px + "end"] = np.array([r[2] for r in s.reads], np.int32)
        arc[px + "seeds"] = np.array(nodes, np.int32)
        cand = [[results[((cfg["name"], s.ci), ri, u)] for u in nodes] for ri in range(nr)]
        f = lambda key, dt=np.float64: np.array([[c[key] for c in row] for row in cand], dt)
        arc[px + "dN"] = f("dN", np.int16)
        arc[px + "est_d"] = f("est_d", np.int16)
        for key in ("est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll"):
            arc[px + key] = f(key)
        arc[px + "pl_const_ll"] = np.array([row[0]["pl_const_ll"] for row in cand])
        arc[px + "pl_outer"] = f("pl_outer", np.uint8)
        arc[px + "pl_em"] = f("pl_em", np.uint16)
        arc[px + "pl_a_node"] = f("pl_a_node", np.uint8)
        arc[px + "margin"] = f("margin", np.float32)
        arc[px + "state_gap"] = f("state_gap", np.float32)
        arc[px + "margin_cond"] = f("margin_cond", np.float32)
        ll = f("est_ll")
        gapf = ll.max(1, keepdims=True) - ll                     # filterPlacements (src/HmmUFOtu_main.cpp:162-173)
        arc[px + "filter_in"] = ~(gapf > MAX_ERROR)
        exact = [[max(c["_q"][0] for c in row) - c["_q"][0] for c in row] for row in cand]
        fm = np.array([min(float(abs(x - mpf(MAX_ERROR))) for x in row) for row in exact])
        arc[px + "filter_margin"] = fm.astype(np.float32)
        assert (arc[px + "filter_in"] == np.array([[not (x > mpf(MAX_ERROR)) for x in row] for row in exact])).all()
        assert fm.min() > FILTER_MARGIN, "a filter gap within %g of %g (%s): change READ_SEED" % (FILTER_MARGIN, MAX_ERROR, px)
        knife = (arc[px + "margin"] < KNIFE_MARGIN) | (arc[px + "state_gap"] < KNIFE_GAP) | (arc[px + "margin_cond"] < 1)
        if knife.mean() > KNIFE_CAP:
            over.append("%s: %d knife-edge candidates of %d" % (px[:-1], knife.sum(), knife.size))
        arc[px + "omp"] = np.stack([q_complements(cand[ri]) for ri in cfg["q_reads"]])
        print("%-7s knife-edge %d/%d, smallest margin %.3g, conditioned %.3g, state gap %.3g, filter margin %.3g" %
              (px[:-1], knife.sum(), knife.size, arc[px + "margin"].min(), arc[px + "margin_cond"].min(), arc[px + "state_gap"].min(), fm.min()), flush=True)
    assert not over, "more than %g of a database's candidates are knife-edge: change READ_SEED (%s)" % (KNIFE_CAP, "; ".join(over))
    return arc


def assemble_deep(states, results, cfg):
    """the deep archive: the per-candidate values of assemble() per read and entry of that read's own candidate list (`cand` [reads][W], -1
    where a list is shorter), the messages of the candidate nodes only, and digests in place of the tree and the rows"""
    da = cfg["db_args"]
    arc = {"max_error": np.array(MAX_ERROR), "dps": np.array(mp.dps), "read_seed": np.array(cfg["read_seed"]),
           "q_reads": np.array(cfg["q_reads"], np.int32), "db_args": np.array([da["n_leaves"], da["cs_len"], da["n_match"]], np.int32),
           "mean_blen": np.array(cfg["mean_blen"]), "cases": np.array([case_name(*c) for c in cfg["cases"]])}
    wide = "read_shapes" in cfg                                  # deepwide: the root log-likelihood at the MSG_COLS columns only
    if wide:
        arc["read_shapes"] = np.array(cfg["read_shapes"], np.int32)
    over = []
    for s in states:
        px = case_name(s.name, s.dg_k) + "_"
        nr = len(s.reads)
        W = max(len(c) for c in s.cands)
        for k, d in s.digests.items():
            arc[px + k + "_sha256"] = np.frombuffer(d, np.uint8)
        arc[px + "height"] = np.array([float(x) for x in s.height])
        arc[px + "msg_cols"] = np.array(s.msg_cols, np.int32)
        arc[px + "msg_nodes"] = np.array(s.msg_nodes, np.int32)
        arc[px + "up"] = np.array([[[flog(x) for x in s.up[u][j]] for j in s.msg_cols] for u in s.msg_nodes])
        arc[px + "down"] = np.array([[[flog(x) for x in s.down[u][j]] for j in s.msg_cols] for u in s.msg_nodes])
        arc[px + "root_ll"] = np.array([float(s.root_ll[j]) for j in (s.msg_cols if wide else range(s.L))])
        arc[px + "root_ll_sum"] = np.array(float(s.root_ll_sum))
        arc[px + "codes"] = np.stack([r[0] for r in s.reads])
        arc[px + "start"] = np.array([r[1] for r in s.reads], np.int32)
        arc[px + "end"] = np.array([r[2] for r in s.reads], np.int32)
        arc[px + "n_cand"] = np.array([len(c) for c in s.cands], np.int32)
        arc[px + "cand"] = np.array([c + [-1] * (W - len(c)) for c in s.cands], np.int32)
        cand = [[results[((cfg["name"], s.ci), ri, u)] for u in s.cands[ri]] for ri in range(nr)]
        pad = lambda row, fill: row + [fill] * (W - len(row))
        f = lambda key, dt=np.float64, fill=0: np.array([pad([c[key] for c in row], fill) for row in cand], dt)
        arc[px + "dN"] = f("dN", np.int16, (0, 0, 0, 0))
        arc[px + "est_d"] = f("est_d", np.int16)
        for key in ("est_ratio", "est_wnr_w", "est_ll", "est_ll_w", "pl_ratio", "pl_wnr", "pl_root_ll"):
            arc[px + key] = f(key)
        arc[px + "pl_const_ll"] = np.array([row[0]["pl_const_ll"] for row in cand])
        arc[px + "pl_outer"] = f("pl_outer", np.uint8)
        arc[px + "pl_em"] = f("pl_em", np.uint16)
        arc[px + "pl_a_node"] = f("pl_a_node", np.int32)
        for key in ("margin", "state_gap", "margin_cond"):
            arc[px + key] = f(key, np.float32, 1.0)
        real = arc[px + "cand"] >= 0
        ll = f("est_ll", fill=-np.inf)
        arc[px + "filter_in"] = real & ~(ll.max(1, keepdims=True) - ll > MAX_ERROR)             # src/HmmUFOtu_main.cpp:162-173
        exact = [[max(c["_q"][0] for c in row) - c["_q"][0] for c in row] for row in cand]
        fm = np.array([min(float(abs(x - mpf(MAX_ERROR))) for x in row) for row in exact])
        arc[px + "filter_margin"] = fm.astype(np.float32)
        for ri, row in enumerate(exact):
            assert [bool(x) for x in arc[px + "filter_in"][ri, :len(row)]] == [not (x > mpf(MAX_ERROR)) for x in row]
        assert fm.min() > FILTER_MARGIN, "a filter gap within %g of %g (%s): change READ_SEED" % (FILTER_MARGIN, MAX_ERROR, px)
        knife = real & ((arc[px + "margin"] < KNIFE_MARGIN) | (arc[px + "state_gap"] < KNIFE_GAP) | (arc[px + "margin_cond"] < 1))
        if knife.sum() > KNIFE_CAP * real.sum():
            over.append("%s: %d knife-edge candidates of %d, per read %s" % (px[:-1], knife.sum(), real.sum(), knife.sum(1).tolist()))
        omp = np.ones((len(cfg["q_reads"]), W, 4, 2))
        for i, ri in enumerate(cfg["q_reads"]):
            omp[i, :len(cand[ri])] = q_complements(cand[ri])
        arc[px + "omp"] = omp
        print("%-7s knife-edge %d/%d, smallest margin %.3g, conditioned %.3g, state gap %.3g, filter margin %.3g" %
              (px[:-1], knife.sum(), real.sum(), arc[px + "margin"][real].min(), arc[px + "margin_cond"][real].min(),
               arc[px + "state_gap"][real].min(), fm.min()), flush=True)
    assert not over, "more than %g of a database's candidates are knife-edge: change READ_SEED (%s)" % (KNIFE_CAP, "; ".join(over))
    return arc


def write_archive(path, arc):
    """an .npz (deflated) with fixed member timestamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arc):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arc[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def one_candidate(case, ri, u, set_name="narrow"):
    """a single candidate regenerated (tests/test_hiprec_oracle.py proves with it that the archive is this file's output); of the wide
    set's databases only the read's own columns are evaluated"""
    cfg = SETS[set_name]
    ci = [case_name(*c) for c in cfg["cases"]].index(case)
    key = (set_name, ci) if set_name == "narrow" else (set_name, ci, ri)
    if key not in _STATES and set_name == "deep":                # the sweep over the whole tree at the read's own columns
        rd = deep_setup(ci, cfg).reads[ri]
        _STATES[key] = deep_state(ci, [deep_sweep((ci, list(range(rd[1], rd[2] + 1))))], cfg)
    if key not in _STATES:
        _STATES[key] = db_state(ci, None if set_name == "narrow" else ri, cfg)
    s = _STATES[key]
    c = candidate(s, ri, u)
    c.pop("_q")
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", choices=sorted(SETS), default="narrow")
    ap.add_argument("--out", default=None)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    cfg = SETS[a.set]
    out = a.out or os.path.join(HERE, cfg["out"])
    workers = max(1, min(16, a.workers))
    ctx = multiprocessing.get_context("fork")
    n = len(cfg["cases"])
    deep = a.set in ("deep", "deepwide")
    if deep:                                                     # the sweeps by column chunks: a column's messages depend on no other's
        L = cfg["db_args"]["cs_len"]
        per = max(1, workers // n)
        if a.set == "deepwide":                                  # chunks of DEEPWIDE_CHUNK columns or more: a worker's P(t) of every branch are amortised
            per = max(1, min(L // DEEPWIDE_CHUNK, 4 * workers // n))
            for ci in range(n):                                  # built here, inherited by the forked workers
                deep_setup(ci, cfg)
        chunks = [(ci, list(range(k, L, per)), a.set) for ci in range(n) for k in range(per)]
        with ctx.Pool(min(workers, len(chunks))) as pool:
            parts = pool.map(deep_sweep, chunks)
        states = [deep_state(ci, [p for p in parts if p["ci"] == ci], cfg) for ci in range(n)]
    else:
        with ctx.Pool(min(workers, n)) as pool:
            states = pool.starmap(db_state, [(ci, None, cfg) for ci in range(n)])
    for s in states:
        _STATES[(a.set, s.ci)] = s
    nodes_of = (lambda s, ri: s.cands[ri]) if deep else (lambda s, ri: range(1, s.n))
    tasks = [((a.set, s.ci), ri, u) for s in states for ri in range(len(s.reads)) for u in nodes_of(s, ri)]
    tasks.sort(key=lambda t: -(states[t[0][1]].reads[t[1]][2] - states[t[0][1]].reads[t[1]][1]) * (1 + max(states[t[0][1]].dg_k, 1)))
    with ctx.Pool(workers) as pool:                              # forked after _STATES is filled: the workers inherit it
        results = dict(pool.imap_unordered(_task, tasks, chunksize=1 if a.set == "deepwide" else 4))
    write_archive(out, assemble(states, results, cfg))
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
