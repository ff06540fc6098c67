"""The cases of tests/test_place_bits_gpu.py and of its generator (tests/make_place_bits_golden.py): small databases and reads that
send a batch to one instance of k_place_blk each, and the run that reads back every candidate's results as raw integers.

The databases and the read shapes are those of the wide set of tests/test_hiprec_gpu.py (8 leaves x 3,300 columns, GTR; reads made as
tests/golden/make_hiprec_golden.py makes them: a leaf's row with 3 % substitutions, `bases` base sites in a region of `cols` columns,
every other site a gap), three reads per batch so that a case has a few dozen candidates."""
import dataclasses
import os
import re

import numpy as np

from conftest import get_db

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "place_bits")
DB_ARGS = dict(n_leaves=8, cs_len=3300, model="GTR", seed=97)
GAP = -2

# instance -> ((columns, base sites) of the reads of the batch, knobs, the kernel the trace must name)
INSTANCES = {
    # the headline instance: 12 sites per thread, gap / base split slots (regions of 1,025 .. 1,536 columns, <= 1,280 gap and 256 base sites)
    "split12": ([(1536, 256), (1400, 200), (1025, 150)], {}, "k_place_blk<12,2,3,0,2,false,1,10>"),
    # four waves per candidate, everything in registers (regions of 2,049 .. 3,072 columns under place_var = 9)
    "wave4": ([(2049, 250), (2300, 300), (2600, 350)], dict(place_var=9, est_var=4), "k_place_blk<12,4,3,0,1>"),
    # the whole v message in LDS (regions of 513 .. 1,024 columns)
    "vlds8": ([(1024, 256), (800, 200), (513, 100)], {}, "k_place_blk<8,2,3,0,3,false,3,6>"),
}
# (case, instance, dGamma categories, special): every instance without dGamma and with four categories; the headline instance also with 8 and
# 16, where the exponentials of a table build fill more lanes (with 16 and two waves, one thread has two); and one set that crosses the
# degenerate EM path and the clamp
CASES = [("%s_k%d" % (inst, k), inst, k, None) for inst in INSTANCES for k in (0, 4)] + \
        [("split12_k%d" % k, "split12", k, None) for k in (8, 16)] + [("split12_k4_edge", "split12", 4, "edge")]
CASE_IDS = [c[0] for c in CASES]
MIN_CANDIDATES = 24


def make_case(name):
    """(db, codes [n][L], start [n], end [n], knobs, kernel, zero-branch node or None)"""
    _, inst, k, special = CASES[CASE_IDS.index(name)]
    shapes, knobs, kernel = INSTANCES[inst]
    db = get_db(DB_ARGS["n_leaves"], DB_ARGS["cs_len"], DB_ARGS["model"], dg_k=k, seed=DB_ARGS["seed"])
    rng = np.random.default_rng(1000 + CASE_IDS.index(name))
    leaves = np.flatnonzero(db.is_leaf)
    codes, start, end = [], [], []
    for ri, (cols, bases) in enumerate(shapes):
        u = int(leaves[rng.integers(len(leaves))])
        s = int(rng.integers(20, db.cs_len - cols - 20)); e = s + cols - 1
        at = np.concatenate([[s, e], s + 1 + rng.choice(cols - 2, size=bases - 2, replace=False)])
        b = np.where(db.seq[u, at] >= 0, db.seq[u, at], db.seq[db.parent[u], at]).astype(np.int8)
        mut = rng.random(len(at)) < 0.03
        b[mut] = (b[mut] + rng.integers(1, 4, size=int(mut.sum()))) % 4
        if special == "edge" and ri == 1:                        # every base a transversion away from the leaf's: no finite n-r branch explains it,
            b = ((b + 2) % 4).astype(np.int8)                    # q falls to 0 in the first EM step and wnr runs into the clamp
        cd = np.full(db.cs_len, GAP, np.int8)
        cd[at] = b
        codes.append(cd); start.append(s); end.append(e)
    zero = None
    if special == "edge":                                        # a branch of length 0: exp(-w_ur) = 1 and p0 = 0 at the start of its u-r EM
        zero = int(leaves[0])
        blen = db.blen.copy(); blen[zero] = 0.0
        db = dataclasses.replace(db, blen=blen)
    return db, np.stack(codes), np.array(start, np.int32), np.array(end, np.int32), knobs, kernel, zero


def run_case(E, name):
    """the read stages as tests/test_hiprec_gpu.py runs them (every seed kept), with the trace on.  Returns the candidates' node, and ratio, wnr
    and iters (outer | EM << 8) as unsigned integers of their own width"""
    db, codes, start, end, knobs, kernel, zero = make_case(name)
    D = E.Database.from_synth(db)
    B = E.Batch(D, len(start))
    for k, v in dict(knobs, trace=1).items():
        B.set_knob(k, v)
    B.set_aligned(codes, start, end)
    opts = E.default_opts(max_error=1e9)
    B.get_seed(opts); B.estimate_seq(opts); B.filter_placements(opts); B.place_seq(opts); B.calc_q_values(opts)
    c = B.candidates()
    B.close(); D.close()
    return dict(offs=c["offs"].astype(np.int64), c_node=c["c_node"].astype(np.int32), ratio=c["ratio"].view(np.uint64).copy(),
                wnr=c["wnr"].view(np.uint64).copy(), iters=c["iters"].view(np.uint32).copy())


def placed_by(err):
    """the kernel names of the trace's placement lines"""
    return re.findall(r"^\[hu\] place: .*, (\S+)$", err, re.M)


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")
