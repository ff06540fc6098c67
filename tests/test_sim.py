"""hmmufotu-amd-sim: the generator, the rejection loop, the record description and the program's refusals
without a device; on the device the kernel against a numpy restatement of src/hmmufotu-sim.cpp:393-409 taken literally
(dot_product_scaled with its MIN_LOGLIK_EXP rule on the raw log messages, the sum of the two, exp(. - max)), the outputs' own
consistency, the refusals of hu_sim_reads, and the program end to end.

How a site is compared.  Both sides draw the same two uniforms from the same integers, so the gap decisions are identical.  A base is
the interval of the normalised cumulative weights that u_base falls into; the kernel's weights differ from the restatement's by
rounding (a few 1e-16 relative: it works in the eigenbasis, in linear space), so a site is DECIDED when u_base is farther than 1e-9
from every boundary of the restatement.  Every decided site must match; at most 2 undecided sites are tolerated per case, and the seed
of a case is chosen, on the host, so that the restatement has none (about 3e-9 per site are expected)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from hmmufotu_amd import engine as E, synth
from conftest import get_db

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-sim")
CLI = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd")
MIN_LOGLIK_EXP = -510.0          # DBL_MIN_EXP / 2 in integer arithmetic, src/PhyloTreeUnrooted.cpp:68
BLOCK = 256                      # HU_SIM_BLOCK: lanes, and columns per tile, of k_sim_reads
M32 = np.uint64(0xffffffff)
KAT = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


# ----------------------------------------------------------------------------- the test's own generator
def np_philox(ctr, key):
    """Philox4x32-10 of counters [..., 4] under one key [2], in uint64 arithmetic"""
    ctr = np.asarray(ctr, np.uint64)
    c = [ctr[..., i] for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]; p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32; k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, -1)


def u01(hi, lo):
    return (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def site_uniforms(seed, g, cols):
    """(u_gap, u_base) of global read g at the columns cols"""
    cols = np.asarray(cols, np.uint64)
    ctr = np.stack([cols, np.full_like(cols, g & 0xffffffff), np.full_like(cols, g >> 32), np.zeros_like(cols)], -1)
    w = np_philox(ctr, [seed & 0xffffffff, seed >> 32])
    return u01(w[:, 0], w[:, 1]), u01(w[:, 2], w[:, 3])


# ----------------------------------------------------------------------------- the restatement
def dot_product_scaled(P, V):
    """src/PhyloTreeUnrooted.h:1495-1503 for every row of V [n][4] (log space)"""
    mx = V.max(1)
    scale = np.where((mx != -np.inf) & (mx < MIN_LOGLIK_EXP), MIN_LOGLIK_EXP - mx, 0.0)[:, None]
    with np.errstate(divide="ignore"):
        return np.log(np.exp(V + scale) @ P.T) - scale


def restate_read(db, gap_frac, c, rc, s, e, seed, g):
    """aligned row of one read and, per site, the distance of u_base to the nearest boundary (inf at a gap)"""
    j = np.arange(s, e + 1)
    ug, ub = site_uniforms(seed, g, j)
    gap = ug <= gap_frac[j]
    v = db.blen[c]
    r = dot_product_scaled(synth.model_P(db.model, v * rc), db.up[c, s:e + 1]) + dot_product_scaled(synth.model_P(db.model, v * (1 - rc)), db.down[c, s:e + 1])
    q = np.exp(r - r.max(1, keepdims=True))
    cum = np.cumsum(q, 1)
    b = cum[:, :3] / cum[:, 3:4]
    base = (ub[:, None] >= b).sum(1)
    margin = np.where(gap, np.inf, np.abs(ub[:, None] - b).min(1))
    row = np.where(gap, ord("-"), np.frombuffer(b"ACGT", np.uint8)[base]).astype(np.uint8).tobytes().decode()
    return row, margin


def restate(db, gap_frac, plan, seed, read0=0):
    out = [restate_read(db, gap_frac, int(plan["node"][r]), float(plan["rc"][r]), int(plan["start"][r]), int(plan["end"][r]), seed, read0 + r)
           for r in range(len(plan["node"]))]
    return [o[0] for o in out], [o[1] for o in out]


def compare(got_rows, want_rows, margins):
    """every decided site equal, the gaps equal everywhere; returns the number of undecided sites"""
    undecided = 0
    for r, (g, w, m) in enumerate(zip(got_rows, want_rows, margins)):
        assert len(g) == len(w), "read %d: %d columns, expected %d" % (r, len(g), len(w))
        ga, wa = np.frombuffer(g.encode(), np.uint8), np.frombuffer(w.encode(), np.uint8)
        assert np.array_equal(ga == ord("-"), wa == ord("-")), "read %d: gap decisions differ" % r
        und = m <= 1e-9
        undecided += int(und.sum())
        bad = (ga != wa) & ~und
        assert not bad.any(), "read %d: decided sites differ at %s" % (r, np.nonzero(bad)[0][:8])
    return undecided


# ----------------------------------------------------------------------------- the cases
def synth_db(which):
    return get_db(40, 600, "GTR", dg_k=4) if which == "synth40" else otus70()


@functools.lru_cache(maxsize=None)
def otus70():
    return synth.make_db_70otus("JC69")


def explicit_plan(db, gap_block):
    """the smallest shapes that can break the kernel (see the issue's list), then random reads up to R = 67 (not a multiple of 64)"""
    L = db.cs_len
    root = int(np.nonzero(db.parent < 0)[0][0])
    kids = np.zeros(db.n_nodes, int); np.add.at(kids, db.parent[db.parent >= 0], 1)
    leaves = [i for i in range(db.n_nodes) if kids[i] == 0 and i != root]
    top = [i for i in range(db.n_nodes) if db.parent[i] == root]
    inner = [i for i in range(db.n_nodes) if kids[i] > 0 and i != root and db.parent[i] != root]
    assert leaves and top and inner and L >= 2 * BLOCK + 8
    g0 = gap_block
    reads = [(leaves[0], 0.0, 0, 0),                                  # one column, start = 0, a leaf, rc = 0
             (inner[0], 0.5, 10, 10 + BLOCK - 2),                     # 255 columns
             (inner[-1], 1.0, 3, 3 + BLOCK - 1),                      # 256 columns, rc = 1
             (top[0], 0.25, 7, 7 + BLOCK),                            # 257 columns, a child of the root
             (leaves[1], 0.0, L - 300, L - 1),                        # end = csLen - 1
             (inner[0], 0.5, g0, g0 + 4),                             # every column has gapFrac = 1: an empty sequence
             (leaves[-1], 1.0, 0, L - 1),                             # every column
             (top[-1], 0.0, 40, 40 + 2 * BLOCK - 1),                  # exactly two tiles
             (leaves[2], 0.5, L - 1, L - 1)]                          # one column, the last
    rng = np.random.default_rng(5)
    nonroot = [i for i in range(db.n_nodes) if i != root]
    while len(reads) < 67:
        s = int(rng.integers(0, L)); e = int(rng.integers(s, min(L, s + 400)))
        reads.append((int(rng.choice(nonroot)), float(rng.random()), s, e))
    a = list(zip(*reads))
    return dict(node=np.array(a[0], np.int32), rc=np.array(a[1]), start=np.array(a[2], np.int32), end=np.array(a[3], np.int32))


_CASES = {}


def case(which):
    """per database, made once: the device database, the gap fractions (a block of five set to 1, one column to 0), the explicit plan,
    a seed for which the restatement has no undecided site, and the restatement"""
    if which not in _CASES:
        need_gpu()
        db = synth_db(which)
        D = E.Database.from_synth(db)
        gf = D.sim_gap_frac().copy()
        g0 = 300
        gf[g0:g0 + 5] = 1.0; gf[g0 + 7] = 0.0
        plan = explicit_plan(db, g0)
        for seed in range(1, 50):
            rows, margins = restate(db, gf, plan, seed)
            if not any((m <= 1e-9).any() for m in margins):
                break
        else:
            raise AssertionError("no seed without an undecided site")
        _CASES[which] = dict(db=db, D=D, gf=gf, plan=plan, seed=seed, rows=rows, margins=margins)
    return _CASES[which]


def sub_plan(plan, a, b):
    return {k: v[a:b] for k, v in plan.items()}


def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


def run(args, cwd, binary=BIN):
    return subprocess.run([binary] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def read_fasta(path):
    recs = []
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    assert len(lines) % 2 == 0                       # one header and ONE sequence line per record
    for h, s in zip(lines[0::2], lines[1::2]):
        assert h[0] == ">"
        rid, desc = h[1:].split(" ", 1)
        recs.append((rid, desc, s))
    return recs


DESC = re.compile(r'branchID=(?P<branchID>\d+->\d+);taxonID=(?P<taxonID>\d+);taxonName=(?P<taxonName>"[^"]*");branchPoint=(?P<branchPoint>[^;]+);'
                  r'csStart=(?P<csStart>\d+);csEnd=(?P<csEnd>\d+);seqLen=(?P<seqLen>\d+);')


def parse_desc(desc):
    """the fields of a record's description; a taxon name holds ';' itself, so the text is not split there"""
    m = DESC.fullmatch(desc)
    assert m, desc
    return m.groupdict()


# ============================================================================= CPU
def test_program_is_built():
    assert os.path.exists(BIN), "hmmufotu-amd-sim missing: run __graft_entry__.build()"


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % w for w in E.sim_philox(ctr, key)) == want
    assert " ".join("%08x" % w for w in np_philox(ctr, key)) == want            # the test's own generator is pinned by the same vectors


def test_philox_of_the_library_and_of_the_test_agree():
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64); key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64)
    want = np_philox(ctr, key)
    for i in range(len(ctr)):
        assert np.array_equal(E.sim_philox(ctr[i], key).astype(np.uint64), want[i])
    u = u01(np.array([0, 0xffffffff], np.uint64), np.array([0, 0xffffffff], np.uint64))
    assert u[0] == 0.0 and u[1] == 1.0 - 2.0 ** -53                              # [0, 1)


def tree_of(which):
    db = get_db(40, 600) if which == "synth40" else otus70()
    return db, (db.parent, db.blen, db.height, db.cs_len)


def check_plan(db, pl, max_dist=np.inf, min_size=0, max_size=0, regions=None):
    c = pl["node"]
    assert (db.parent[c] >= 0).all()                                              # never the root
    assert (db.height[c] + db.blen[c] * pl["rc"] <= max_dist).all()
    assert ((pl["rc"] >= 0) & (pl["rc"] < 1)).all()
    assert ((0 <= pl["start"]) & (pl["start"] <= pl["end"]) & (pl["end"] < db.cs_len)).all()
    if regions is None:
        ln = pl["end"] - pl["start"]                                              # len, of len + 1 columns
        assert (ln >= int(min_size)).all() and (max_size == 0 or (ln <= int(max_size)).all())
    else:
        ok = {(s + 1, e) for s, e in regions if 0 <= s < e < db.cs_len}
        assert set(zip(pl["start"].tolist(), pl["end"].tolist())) == ok             # every accepted region is used, no other


@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_plan_respects_the_reference_rules(which):
    db, t = tree_of(which)
    L = db.cs_len
    pl = E.sim_plan(*t, 2000, 11, mean_size=200, sd_size=60)
    check_plan(db, pl)
    assert len(set((pl["end"] - pl["start"]).tolist())) > 20                      # sizes do vary
    pl = E.sim_plan(*t, 2000, 11, mean_size=200, sd_size=60, min_size=180.5, max_size=230.9)
    check_plan(db, pl, min_size=180.5, max_size=230.9)
    ln = pl["end"] - pl["start"]
    assert ln.min() == 180 and ln.max() == 230                                    # both clamps bite, cut as the reference's int
    d = float(np.median(db.height[db.height > 0]))                                # some nodes are out, the leaves (height 0) are in
    assert (db.height > d).any()
    pl = E.sim_plan(*t, 2000, 11, mean_size=200, max_dist=d)
    check_plan(db, pl, max_dist=d)
    assert len(set(pl["node"].tolist())) > 3
    regions = [(10, 50), (0, L), (5, 5), (100, L - 1), (-1, 20), (70, 60), (L - 2, L - 1)]   # (0, L): ends AT csLen, refused here
    pl = E.sim_plan(*t, 500, 11, regions=regions)
    check_plan(db, pl, regions=regions)


@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_plan_depends_on_seed_and_options_alone(which):
    db, t = tree_of(which)
    a = E.sim_plan(*t, 300, 5, mean_size=150, info=True)
    b = E.sim_plan(*t, 300, 5, mean_size=150)
    c = E.sim_plan(*t, 300, 6, mean_size=150)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    assert not np.array_equal(a["node"], c["node"]) and not np.array_equal(a["rc"], c["rc"])
    assert a["attempt"] >= 300
    # in pieces of unequal size, the attempt number carried along: the same plan
    att, parts = 0, []
    for n in (1, 7, 192, 100):
        p = E.sim_plan(*t, n, 5, mean_size=150, attempt=att, info=True)
        att = p["attempt"]; parts.append(p)
    assert att == a["attempt"]
    assert all(np.array_equal(np.concatenate([p[k] for p in parts]), b[k]) for k in b)


@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_plan_reaches_every_branch(which):
    db, t = tree_of(which)
    pl = E.sim_plan(*t, 100 * db.n_nodes, 3, mean_size=100)
    assert set(pl["node"].tolist()) == {i for i in range(db.n_nodes) if db.parent[i] >= 0}     # a miss: about nodes x e^-100


def test_plan_refusals():
    db, t = tree_of("synth40")
    for kw in (dict(mean_size=0), dict(sd_size=0), dict(min_size=-1), dict(min_size=9, max_size=3), dict(min_size=db.cs_len),
               dict(max_dist=-1.0)):
        with pytest.raises(E.EngineError):
            E.sim_plan(*t, 5, 1, **kw)


def test_description_byte_for_byte():
    d = E.sim_description(5, 2, "k__A;p__B", "k__A", 0.1, 3, 9, 7)
    assert d == 'branchID=5->2;taxonID=5;taxonName="k__A;p__B";branchPoint=0.10000000000000001;csStart=3;csEnd=9;seqLen=7;'
    d = E.sim_description(5, 2, "k__A;p__B", "k__A", 0.5, 0, 0, 1)                # rc <= 0.5: the child
    assert d == 'branchID=5->2;taxonID=5;taxonName="k__A;p__B";branchPoint=0.5;csStart=0;csEnd=0;seqLen=1;'
    d = E.sim_description(5, 2, "k__A;p__B", "k__A", 0.75, 0, 0, 1)               # beyond the middle: the parent
    assert d == 'branchID=5->2;taxonID=2;taxonName="k__A";branchPoint=0.75;csStart=0;csEnd=0;seqLen=1;'
    rc = 0.1 + 0.2                                                                 # 0.30000000000000004: 16 digits give back 0.3, another double
    assert float("%.16g" % rc) != rc and float("%.17g" % rc) == rc
    d = E.sim_description(123456, 77, "", "x", rc, 1499, 1500, 0)
    assert d == 'branchID=123456->77;taxonID=123456;taxonName="";branchPoint=0.30000000000000004;csStart=1499;csEnd=1500;seqLen=0;'
    assert E.sim_description(1, 0, "a", "b", 0.0, 0, 0, 0).split(";")[3] == "branchPoint=0"
    assert E.sim_description(1, 0, "a", "b", 1e-05, 0, 0, 0).split(";")[3] == "branchPoint=1.0000000000000001e-05"


def test_program_refusals(tmp_path):
    db = get_db(40, 600)
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    out = tmp_path / "sim.fa"

    def refused(args, *lines):
        r = run(args, tmp_path)
        got = [x for x in r.stderr.split("\n") if x]
        assert r.returncode == 1 and r.stdout == "" and got[:len(lines)] == list(lines), (r.returncode, r.stderr)
        assert "device" not in r.stderr            # refused before a device is asked for: this test runs without one
        assert not out.exists()

    r = run([pre, out], tmp_path)                                                  # a missing -N: "Error:" and the usage (:140-144)
    assert r.returncode == 1 and r.stderr.startswith("Error:\nUsage:    ") and not out.exists()
    refused([pre, out, "-N", "0"], "-N must be positive")
    refused([pre, out, "-N", "5", "-l", "9", "-u", "3"], "-u|--max-size must be non-negative and non-less than -l|--min-size")
    refused([pre, out, "-N", "5", "-s", "0"], "-s|--sd-size must be positive")
    refused([pre, out, "-N", "5", "--sd-size", "-2"], "-s|--sd-size must be positive")       # the long spelling is read here
    refused([pre, out, "-N", "5", "-m", "0"], "-m|--min-size must be positive")               # the reference's message names --min-size
    refused([pre, out, "-N", "5", "-l", "-1"], "-l|--min-size must be non-negative")
    refused([str(tmp_path / "nodb"), out, "-N", "5"], "Unable to open %s : No such file or directory" % (tmp_path / "nodb.hmm"))
    os.rename(pre + ".ptu", pre + ".away")
    refused([pre, out, "-N", "5"], "Unable to open %s.ptu : No such file or directory" % pre)
    os.rename(pre + ".away", pre + ".ptu")
    refused([pre, out, "-N", "5", "-R", tmp_path / "no.bed"], "Unable to open %s : No such file or directory" % (tmp_path / "no.bed"))
    bad = tmp_path / "nodir" / "sim.fa"
    refused([pre, bad, "-N", "5"], "Unable to write seq to '%s' : No such file or directory" % bad)
    refused([pre, out, bad, "-N", "5"], "Unable to write mate to '%s' : No such file or directory" % bad)   # and the read file made before it is removed


def test_program_without_a_device_leaves_no_output(tmp_path):
    if E.device_count() > 0:
        return                                      # with a device the same call succeeds: test_program_end_to_end
    db = get_db(40, 600)
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    r = run([pre, "sim.fa", "mate.fa", "-N", "5"], tmp_path)
    assert r.returncode == 1 and "gfx950 device(s) visible" in r.stderr
    assert not (tmp_path / "sim.fa").exists() and not (tmp_path / "mate.fa").exists()


# ============================================================================= GPU
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_kernel_against_the_restatement(which):
    c = case(which)
    assert not any((m <= 1e-9).any() for m in c["margins"])                       # the seed was chosen so
    got = c["D"].sim_reads(c["plan"], c["gf"], c["seed"])
    und = compare(got["aligned"], c["rows"], c["margins"])
    print("%s: seed %d, %d reads, %d sites, %d undecided" % (which, c["seed"], len(c["rows"]), sum(len(r) for r in c["rows"]), und))
    assert und <= 2
    assert got["seq"][5] == "" and set(got["aligned"][5]) == {"-"}                # the read over the all-gap block
    g7 = c["plan"]["start"] <= 307
    assert all(row[307 - s] != "-" for row, s, e, ok in zip(got["aligned"], c["plan"]["start"], c["plan"]["end"], g7) if ok and e >= 307)   # gapFrac = 0
    one = c["D"].sim_reads(sub_plan(c["plan"], 0, 1), c["gf"], c["seed"])         # R = 1
    assert one["aligned"] == got["aligned"][:1] and one["seq"] == got["seq"][:1]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_a_leaf_at_rc_zero_gives_its_own_bases(which):
    c = case(which); db = c["db"]
    kids = np.zeros(db.n_nodes, int); np.add.at(kids, db.parent[db.parent >= 0], 1)
    leaves = np.array([i for i in range(db.n_nodes) if kids[i] == 0 and db.parent[i] >= 0], np.int32)
    n = len(leaves)
    plan = dict(node=leaves, rc=np.zeros(n), start=np.zeros(n, np.int32), end=np.full(n, db.cs_len - 1, np.int32))
    gf = np.minimum(c["gf"], 0.5)                                                  # enough sites that are no gap
    got = c["D"].sim_reads(plan, gf, 77)
    seen = 0
    for r, u in enumerate(leaves):
        row = np.frombuffer(got["aligned"][r].encode(), np.uint8)
        own = db.seq[u]
        at = (own >= 0) & (row != ord("-"))
        seen += int(at.sum())
        assert np.array_equal(row[at], np.frombuffer(b"ACGT", np.uint8)[own[at]]), "leaf %d" % u
    assert seen > n * 10


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["synth40", "otus70"])
def test_outputs_agree_with_each_other_and_with_split_calls(which):
    c = case(which)
    got = c["D"].sim_reads(c["plan"], c["gf"], c["seed"], read0=1000, mate=True)
    for r in range(len(got["aligned"])):
        assert got["seq"][r] == got["aligned"][r].replace("-", "") and got["seq_len"][r] == len(got["seq"][r])
        assert got["mate"][r] == E.revcom_as_read(got["seq"][r])
    assert any(len(s) > BLOCK for s in got["seq"]) or which == "synth40"          # a sequence compacted over more than one tile
    rows, margins = restate(c["db"], c["gf"], c["plan"], c["seed"], read0=1000)
    assert compare(got["aligned"], rows, margins) <= 2
    parts, a = [], 0
    for n in (1, 23, 43):                                                          # three calls of unequal size: 67 reads
        parts.append(c["D"].sim_reads(sub_plan(c["plan"], a, a + n), c["gf"], c["seed"], read0=1000 + a, mate=True)); a += n
    assert a == len(got["aligned"])
    for k in ("aligned", "seq", "mate"):
        assert sum((p[k] for p in parts), []) == got[k]
    t = E.sim_timing()
    assert t["kernel"] > 0 and t["to_device"] > 0 and t["to_host"] > 0


@pytest.mark.gpu
def test_sim_reads_refuses_bad_plans_and_goes_on():
    c = case("synth40"); db, D, L = c["db"], c["D"], c["db"].cs_len
    root = int(np.nonzero(db.parent < 0)[0][0])
    lib = E.load_library()
    import ctypes as C
    good = sub_plan(c["plan"], 0, 9)
    for k, v in (("node", root), ("node", db.n_nodes), ("node", -1), ("end", L), ("start", L - 1), ("rc", 1.5), ("rc", -0.1), ("rc", np.nan), ("start", -1)):
        plan = {x: y.copy() for x, y in good.items()}
        plan[k][4] = v                                                              # read 4 is (leaf, 0, L - 300, L - 1): start = L - 1 is fine, so
        if (k, v) == ("start", L - 1):
            plan["end"][4] = L - 2                                                 # start > end
        node = plan["node"]; rc = plan["rc"]; st = plan["start"]; en = plan["end"]
        total = 4096
        al = np.full(total, 0x5a, np.uint8); sq = al.copy(); mt = al.copy(); ln = np.full(9, -7, np.int32)
        rcode = lib.hu_sim_reads(D.h, C.c_int64(9), E._p(node, C.c_int32), E._p(rc, C.c_double), E._p(st, C.c_int32), E._p(en, C.c_int32), E._p(c["gf"], C.c_double),
                                 C.c_uint64(1), C.c_uint64(0), C.c_int(1), al.ctypes.data_as(C.c_char_p), sq.ctypes.data_as(C.c_char_p), mt.ctypes.data_as(C.c_char_p), E._p(ln, C.c_int32))
        assert rcode == -1, (k, v, rcode)                                          # HU_ERR_ARG
        assert "read 4" in lib.hu_last_error().decode()
        assert (al == 0x5a).all() and (sq == 0x5a).all() and (mt == 0x5a).all() and (ln == -7).all()      # the outputs are untouched
        with pytest.raises(E.EngineError):
            D.sim_reads(plan, c["gf"], 1)
    got = D.sim_reads(c["plan"], c["gf"], c["seed"])                              # a later valid call still matches
    assert compare(got["aligned"], c["rows"], c["margins"]) <= 2


@pytest.mark.gpu
def test_windowed_database_is_refused():
    db = synth_db("synth40")
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    W = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, db.up[:, 100:300], db.down[:, 100:300], db.height, md, db.anno_id, db.anno_dist, win_start=100, win_len=200)
    try:
        with pytest.raises(E.EngineError, match="column window"):
            W.sim_reads(dict(node=[1], rc=[0.5], start=[120], end=[130]), np.zeros(db.cs_len), 1)
    finally:
        W.close()


def leaf_rows_as_text(db):
    kids = np.zeros(db.n_nodes, int); np.add.at(kids, db.parent[db.parent >= 0], 1)
    return np.frombuffer(b"ACGT-", np.uint8)[np.where(db.seq[kids == 0] >= 0, db.seq[kids == 0], 4)]       # in node-id order


def want_gap_frac(rows):
    st = E.msa_stats(rows)
    with np.errstate(invalid="ignore"):
        return st["gap_wcount"] / (((st["res_wcount"][0] + st["res_wcount"][2]) + (st["res_wcount"][1] + st["res_wcount"][3])) + st["gap_wcount"])


@pytest.mark.gpu
def test_gap_fractions():
    # 70_otus: a pruned alignment, every column holds a residue
    c = case("otus70"); db, D = c["db"], c["D"]
    rows = leaf_rows_as_text(db)
    want = want_gap_frac(rows)
    got = D.sim_gap_frac()
    assert np.array_equal(got, want) and ((got >= 0) & (got < 1)).all() and got.min() < 0.2 and got.max() > 0.8
    wide = np.insert(rows, [0, 17, 17, rows.shape[1]], ord("-"), axis=1)          # four columns MSA::prune drops
    assert np.array_equal(D.sim_gap_frac(wide), want)
    with pytest.raises(E.EngineError, match="columns"):
        D.sim_gap_frac(rows[:, :-1])
    # the synthetic database keeps columns no leaf has a residue in: its own rows give 1 there, as an alignment they are refused
    c = case("synth40"); db, D = c["db"], c["D"]
    rows = leaf_rows_as_text(db)
    got = D.sim_gap_frac()
    empty = (rows == ord("-")).all(0)
    assert empty.any() and np.array_equal(got, want_gap_frac(rows)) and (got[empty] == 1).all() and (got[~empty] < 1).all()
    with pytest.raises(E.EngineError, match="%d columns of the alignment hold a residue" % (~empty).sum()):
        D.sim_gap_frac(rows)


@pytest.mark.gpu
def test_program_end_to_end(tmp_path):
    db = synth_db("synth40"); L = db.cs_len
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    common = [pre, "-N", "40", "-S", "12345", "-m", "450", "-s", "40", "--prefix", "sim_"]
    for a in (["a.fa"], ["b.fa", "--batch", "7"], ["k.fa", "-k", "--batch", "13"], ["p1.fa", "p2.fa", "-r", "100", "-k"], ["c.fa", "-r", "50", "--batch", "40"]):
        r = run(common[:1] + a + common[1:], tmp_path)
        assert r.returncode == 0 and r.stdout == "", r.stderr
    raw = lambda n: (tmp_path / n).read_bytes()
    assert raw("a.fa") == raw("b.fa")                                              # --batch does not show
    A, K, P1, P2, Cc = (read_fasta(tmp_path / n) for n in ("a.fa", "k.fa", "p1.fa", "p2.fa", "c.fa"))
    assert [r[0] for r in A] == ["sim_%d" % i for i in range(1, 41)] == [r[0] for r in K] == [r[0] for r in P2]
    total = 0
    for a, k, p1, p2, cc in zip(A, K, P1, P2, Cc):
        d, dk = parse_desc(a[1]), parse_desc(k[1])
        c, p = (int(x) for x in d["branchID"].split("->"))
        assert db.parent[c] == p and int(d["taxonID"]) == (c if float(d["branchPoint"]) <= 0.5 else p)
        assert d["taxonName"] == '"%s"' % db.annos[int(d["taxonID"])]
        s, e = int(d["csStart"]), int(d["csEnd"])
        assert 0 <= s <= e < L and int(d["seqLen"]) == len(a[2]) and e - s + 1 >= len(a[2]) and set(a[2]) <= set("ACGT")
        assert len(k[2]) == L == int(dk["seqLen"]) and k[2][:s] == "." * s and k[2][e + 1:] == "." * (L - 1 - e) and "." not in k[2][s:e + 1]
        assert k[2].replace(".", "").replace("-", "") == a[2]
        assert {x: y for x, y in dk.items() if x != "seqLen"} == {x: y for x, y in d.items() if x != "seqLen"}
        assert p1[1] == a[1] == p2[1] == cc[1]                                     # a mate file switches -k off; seqLen is the length before -r
        assert p1[2] == a[2][:100] and p2[2] == E.revcom_as_read(a[2])[:100] and cc[2] == a[2][:50]
        total += len(a[2])
    assert total > 40 * 20
    # the reads go through the assignment program: one line per read
    r = run([pre, "a.fa", "-o", "a.tsv"], tmp_path, binary=CLI)
    assert r.returncode == 0, r.stderr
    lines = (tmp_path / "a.tsv").read_text().strip().split("\n")
    body = [x for x in lines if not x.startswith("#") and not x.startswith("id\t")]
    assert len(body) == 40 and [x.split("\t")[0] for x in body] == [r[0] for r in A]


@pytest.mark.gpu
def test_program_regions_and_msa(tmp_path):
    db = synth_db("otus70"); L = db.cs_len
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    (tmp_path / "r.bed").write_text("cs\t20\t200\tx\ncs\t0\t%d\ncs\t300\t%d\nshort\t1\n" % (L, L - 1))
    with open(tmp_path / "m.fasta", "w") as f:
        for i, row in enumerate(leaf_rows_as_text(db)):
            f.write(">s%d\n..%s.\n" % (i, row.tobytes().decode()))                 # three columns without a residue: pruned
    r = run([pre, "r.fa", "-N", "30", "-S", "9", "-R", "r.bed"], tmp_path)
    assert r.returncode == 0 and "Region (0,%d] is not in the consensus range, ignored" % L in r.stderr, r.stderr
    got = {(int(parse_desc(x[1])["csStart"]), int(parse_desc(x[1])["csEnd"])) for x in read_fasta(tmp_path / "r.fa")}
    assert got == {(21, 200), (301, L - 1)}
    r = run([pre, "m.fa", "-N", "30", "-S", "9", "-R", "r.bed", "--msa", "m.fasta"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "m.fa").read_bytes() == (tmp_path / "r.fa").read_bytes()    # the same rows in the same order: the same fractions
