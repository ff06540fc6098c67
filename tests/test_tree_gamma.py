"""hmmufotu-amd-tree --ml-lengths --gamma K: branch lengths and the shape under the discrete Gamma of rates.

The yardstick is the restatement in this file, which shares no code with the library: the pruning of test_tree_blen's RefTree per
category at the lengths rate_c blen, the mixture as the per-column log of the mean of the categories' likelihoods, f_u, f_u' and
f_u'' from the two partials of every category at the ends of the branch, each branch's optimum by bisection on the restated f', and
the category rates from scipy's incomplete gamma function and its inverse.  The library's rates are held to a file that a committed
script wrote with scipy (tests/golden/make_tree_gamma_golden.py); that test reads the file alone.

The bar of the scores: the deviation of f relative to |f|, of f' and f'' relative to the sums of the absolute values of their column
terms, as section 22 has it.  Measured over the cases of this file, the device's shapes included: 1.15e-12 on the host path and
1.14e-12 on the device (MI355X), both at 12 leaves x 257 columns, HKY85, K = 2, alpha = 0.3; four times the larger, 4.6e-12, rounded up
to a power of two is SCORE_BAR = 2^-37 = 7.28e-12.  Section 22's were 6.0e-13
and 5.5e-13, and the loss has the same origin: a leaf whose base differs from its neighbourhood's on a short branch, where L_j(t) is of
the order of t and a difference of spectral terms of the order of 1.
"""
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy.special import gammainc, gammaincc, gammaincinv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E, synth  # noqa: E402
from test_tree_blen import RefModel, RefTree, random_tree, make_case  # noqa: E402
import test_tree_blen as B  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "tree_gamma")
TAU, EPS = B.TAU, B.EPS
HOST_MEASURED = 1.15e-12      # 12 leaves x 257 columns, HKY85, K = 2, alpha = 0.3
DEVICE_MEASURED = 1.14e-12    # the same case
SCORE_BAR = 2.0 ** -37        # 7.28e-12: 4 x 1.15e-12 = 4.6e-12, rounded up to a power of two
assert 4 * max(HOST_MEASURED, DEVICE_MEASURED) <= SCORE_BAR <= 1e-10


# ---- the restatement ----

def ref_rates(k, alpha):
    """K equally probable categories of Gamma(shape alpha, rate alpha), each rate the mean of its category"""
    if k == 1:
        return np.ones(1)
    q = gammaincinv(alpha, np.arange(1, k) / k)
    p = np.concatenate([[0.0], gammainc(alpha + 1, q)])
    return np.concatenate([k * np.diff(p), [k * gammaincc(alpha + 1, q[-1])]])


class RefGamma:
    """K trees of RefTree, pruned at rate_c blen"""

    def __init__(self, c, k, alpha, blen):
        self.c, self.k, self.rho = c, k, ref_rates(k, alpha)
        self.m = c.ref.m
        self.trees = [RefTree(c.parent, c.seq, self.m).messages(r * np.asarray(blen)) for r in self.rho]

    def per_col(self):
        v = np.array([np.log(t.up[t.root] @ self.m.pi) + t.us[t.root] for t in self.trees])
        mx = v.max(0)
        return mx + np.log(np.exp(v - mx).mean(0))

    def loglik(self):
        return math.fsum(self.per_col())

    def branch(self, u, t):
        """f, f', f'' of branch u at t and the sums of the absolute column terms of f' and f''"""
        sc = np.array([tr.us[u] + tr.ds[u] for tr in self.trees])
        mx = sc.max(0)
        L0 = L1 = L2 = 0.0
        for r, tr, s in zip(self.rho, self.trees, sc):
            x = tr.up[u] * self.m.pi[None, :]; y = tr.down[u]; w = np.exp(s - mx) / self.k
            L0 = L0 + w * np.einsum("ja,ab,jb->j", x, self.m.P(r * t), y)
            L1 = L1 + w * r * np.einsum("ja,ab,jb->j", x, self.m.P(r * t, 1), y)
            L2 = L2 + w * r * r * np.einsum("ja,ab,jb->j", x, self.m.P(r * t, 2), y)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = L1 / L0; h = L2 / L0 - g * g
            f = math.fsum(np.log(L0) + mx)
        return f, math.fsum(g), math.fsum(h), math.fsum(np.abs(g)), math.fsum(np.abs(h))

    def slope(self, u, t):
        return self.branch(u, t)[1]

    def optimum(self, u, lo, hi):
        if not self.slope(u, lo) > 0:
            return lo
        if not self.slope(u, hi) < 0:
            return hi
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if self.slope(u, mid) > 0:
                lo = mid
            else:
                hi = mid
        return 0.5 * (lo + hi)


def ref_loglik(c, k, alpha, blen):
    return RefGamma(c, k, alpha, blen).loglik()


def deviation(ref, got, u, t):
    """of the scores of branch u; a sum that is exactly 0 has no scale and is left out"""
    f, g, h, ag, ah = ref.branch(u, t)
    worst = 0.0
    for have, want, scale in ((got["f"][u], f, abs(f)), (got["d1"][u], g, ag), (got["d2"][u], h, ah)):
        if scale != 0:
            worst = max(worst, abs(have - want) / scale)
    return worst


def score_deviation(c, k, alpha, host, device=0):
    ref = RefGamma(c, k, alpha, c.start)
    worst = 0.0
    for t in B.score_points(c):
        got = E.tree_gamma_branch_scores(c.parent, c.start, c.seq, c.md, k=k, alpha=alpha, t=np.where(c.parent >= 0, t, 0.0), host=host, device=device)
        worst = max([worst] + [deviation(ref, got, u, t[u]) for u in range(1, len(c.parent))])
    return worst


def check_step(c, ref, got):
    """the restated slope condition for every branch; returns the kinds met"""
    kinds = set()
    assert got["n_capped"] == 0 and not got["capped"].any()
    for u in range(1, len(c.parent)):
        t = got["t_star"][u]
        assert c.min_len <= t <= c.max_len
        if t == c.min_len:
            kinds.add("min"); assert ref.slope(u, c.min_len) <= 0, (c.name, u)
        elif t == c.max_len:
            kinds.add("max"); assert ref.slope(u, c.max_len) >= 0, (c.name, u)
        else:
            kinds.add("inner")
            assert ref.slope(u, max(t - 2 * TAU, c.min_len)) >= 0 and ref.slope(u, min(t + 2 * TAU, c.max_len)) <= 0, (c.name, u, t)
    return kinds


# ---- the rates ----

def test_rates_are_the_golden_files():
    with open(os.path.join(GOLD, "rates.json")) as f:
        rec = json.load(f)
    assert sorted({r["k"] for r in rec}) == [1, 2, 4, 8, 16] and sorted({r["alpha"] for r in rec}) == [0.05, 0.3, 1.0, 7.0, 100.0] and len(rec) == 25
    worst = 0.0
    for r in rec:
        got, want = E.gamma_rates(r["k"], r["alpha"]), np.array(r["rates"])
        assert got.shape == want.shape and (np.diff(got) > 0).all()
        worst = max(worst, np.abs(got / want - 1).max())
        assert abs(math.fsum(got) - r["k"]) <= 1e-13, r
    print("largest relative deviation of a rate: %.3g" % worst)
    assert worst <= 1e-12


# ---- one category, the pulley principle, the scores ----

def test_one_category_is_the_fixed_rate_entry():
    for c in B.cases():
        kw = dict(min_len=c.min_len, max_len=c.max_len, host=True)
        a = E.tree_branch_step(c.parent, c.start, c.seq, c.md, **kw)
        g = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, k=1, alpha=0.7, **kw)
        for u in range(1, len(c.parent)):
            f, d1, d2, ag, ah = c.ref.messages(c.start).branch(u, c.start[u])
            assert abs(g["f"][u] - a["f"][u]) <= SCORE_BAR * abs(f) and abs(g["d1"][u] - a["d1"][u]) <= SCORE_BAR * ag and abs(g["d2"][u] - a["d2"][u]) <= SCORE_BAR * ah
        assert np.abs(g["t_star"] - a["t_star"]).max() <= 2 * TAU
        ll = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, max_rounds=1, host=True)["ll_start"]
        got = E.tree_gamma_loglik(c.parent, c.start, c.seq, c.md, k=1, alpha=0.7, host=True)
        assert abs(got["ll"] - ll) <= SCORE_BAR * abs(ll) and np.array_equal(got["per_col"], got["per_cat"][0])


def test_pulley_every_branch_gives_the_gamma_loglik():
    for c in B.cases():
        for k, alpha in ((4, 0.5), (2, 5.0)):
            ref = RefGamma(c, k, alpha, c.start)
            want = ref.loglik()
            got = E.tree_gamma_branch_scores(c.parent, c.start, c.seq, c.md, k=k, alpha=alpha, host=True)
            f = got["f"][1:]
            assert np.abs(f - want).max() <= SCORE_BAR * abs(want), c.name
            assert np.abs(f - f[0]).max() <= SCORE_BAR * abs(want)
            for u in range(1, len(c.parent)):
                assert abs(ref.branch(u, c.start[u])[0] - want) <= 1e-12 * abs(want)
            ll = E.tree_gamma_loglik(c.parent, c.start, c.seq, c.md, k=k, alpha=alpha, host=True)
            assert abs(ll["ll"] - want) <= SCORE_BAR * abs(want) and np.abs(ll["per_col"] - ref.per_col()).max() <= SCORE_BAR * abs(want)
            assert got["f"][0] == 0 and got["d1"][0] == 0


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("alpha", [0.3, 1.0, 5.0])
def test_scores_against_the_restatement_host(k, alpha):
    worst = max(score_deviation(c, k, alpha, host=True) for c in B.cases())
    print("largest deviation of the host path's scores, K %d alpha %g: %.3g" % (k, alpha, worst))
    assert worst <= SCORE_BAR


# ---- the step ----

def test_step_finds_each_branchs_optimum_host():
    kinds = set()
    for c in B.cases():
        got = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, k=4, alpha=0.5, min_len=c.min_len, max_len=c.max_len, host=True)
        kinds |= check_step(c, RefGamma(c, 4, 0.5, c.start), got)
        sc = E.tree_gamma_branch_scores(c.parent, c.start, c.seq, c.md, k=4, alpha=0.5, host=True)
        assert np.array_equal(sc["f"], got["f"]) and np.array_equal(sc["d1"], got["d1"]) and np.array_equal(sc["d2"], got["d2"])
    assert kinds == {"min", "max", "inner"}


# ---- the fit ----

def why_case():
    """12 leaves x 400 columns, HKY85, true lengths exponential(0.12) + 0.02, the columns' rates drawn from the eight category rates of
    shape 0.5, 5 % gaps"""
    def make():
        rng = np.random.default_rng(11)
        c = B.Case()
        c.name = "why"; c.min_len, c.max_len = 0.0, 10.0
        c.parent = random_tree(12, rng)
        n, L = len(c.parent), 400
        c.sm = synth.load_model("HKY85")
        c.md = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par)
        c.true = rng.exponential(0.12, n) + 0.02
        c.true[0] = 0.0
        col = ref_rates(8, 0.5)[rng.integers(0, 8, L)]
        seq = synth.evolve_sequences(c.parent, c.true, L, c.sm, col, rng)
        seq[rng.random(seq.shape) < 0.05] = -2
        inner = np.zeros(n, bool); inner[c.parent[c.parent >= 0]] = True
        seq[inner] = -2
        c.seq = np.ascontiguousarray(seq, np.int8)
        c.start = np.where(c.parent >= 0, 0.1, 0.0)
        c.ref = RefTree(c.parent, c.seq, RefModel(c.sm))
        c.fixed = E.tree_optimize_lengths(c.parent, c.start, c.seq, c.md, max_rounds=1000, host=True)
        c.fit = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, max_rounds=1000, host=True)
        return c
    return B.cached("gamma why", make)


def check_fit(c, r, k, eps_ll=0.01):
    lls = [r["ll_start"]] + [p["ll"] for p in r["passes"]]
    assert all(b >= a for a, b in zip(lls, lls[1:])), lls
    assert r["ll_final"] == lls[-1] and r["n_capped"] == 0 and r["alpha"] == r["passes"][-1]["alpha"]
    assert np.abs(r["rates"] / ref_rates(k, r["alpha"]) - 1).max() <= 1e-12
    blen, alpha = r["blen"], r["alpha"]
    assert ((blen[1:] >= c.min_len) & (blen[1:] <= c.max_len)).all()
    ref = RefGamma(c, k, alpha, blen)
    want = ref.loglik()
    assert abs(r["ll_final"] - want) <= SCORE_BAR * abs(want)
    return ref, want


def test_fit_on_the_case_of_the_issue():
    c = why_case()
    r = c.fit
    print(r["stop"], r["alpha"], r["ll_start"], r["ll_final"], r["passes"], "fixed-rate:", c.fixed["ll_final"], c.fixed["blen"].sum(), "gamma:", r["blen"].sum(),
          "true:", c.true.sum())
    assert c.fixed["stop"] == "converged" and r["stop"] == "converged" and 2 <= len(r["passes"]) <= 10
    ref, want = check_fit(c, r, 4)
    assert r["passes"][-1]["n_rounds"] < 1000                 # the last fit converged: every length is at its own optimum
    for u in range(1, len(c.parent)):
        assert abs(r["blen"][u] - ref.optimum(u, c.min_len, c.max_len)) <= 2 * EPS, u
    for fac in (math.exp(0.05), math.exp(-0.05)):
        assert ref_loglik(c, 4, r["alpha"] * fac, r["blen"]) <= want + 0.01
    assert r["ll_final"] - c.fixed["ll_final"] >= 100
    assert r["blen"].sum() > c.fixed["blen"].sum()
    assert abs(r["ll_start"] - ref_loglik(c, 4, 1.0, c.fixed["blen"])) <= SCORE_BAR * abs(want)


def test_fit_with_a_fixed_alpha_is_one_pass_and_a_second_run_gives_the_same_bits():
    c = why_case()
    r = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, alpha=0.7, max_rounds=1000, host=True)
    assert r["stop"] == "fixed alpha" and len(r["passes"]) == 1 and r["alpha"] == 0.7 == r["passes"][0]["alpha"]
    ref, want = check_fit(c, r, 4)
    for u in range(1, len(c.parent)):
        assert abs(r["blen"][u] - ref.optimum(u, c.min_len, c.max_len)) <= 2 * EPS, u
    again = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, max_rounds=1000, host=True)
    assert np.array_equal(again["blen"], c.fit["blen"]) and again["alpha"] == c.fit["alpha"] and again["passes"] == c.fit["passes"]
    big = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, max_rounds=1000, host=True, mem_budget=1 << 40)
    assert np.array_equal(big["blen"], c.fit["blen"])              # no dependence on the memory budget


# ---- refusals of the entries ----

def test_entries_refuse_what_the_header_says():
    c = B.cases()[0]
    n, L = c.seq.shape
    dg = E.model_desc(c.sm.type_id, c.sm.pi, c.sm.par, dg_rates=[0.1, 0.4, 1.0, 2.5])
    for fn in (E.tree_gamma_loglik, E.tree_gamma_branch_scores, E.tree_gamma_branch_step, E.tree_gamma_fit):
        with pytest.raises(E.EngineError, match="error -1: .*discrete Gamma"):
            fn(c.parent, c.start, c.seq, dg, host=True)
        for kw in (dict(k=0), dict(k=17), dict(alpha=0.01), dict(alpha=200.0)):
            with pytest.raises(E.EngineError, match="error -1"):
                fn(c.parent, c.start, c.seq, c.md, host=True, **kw)
        with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.gamma_need(n, L, 4)):
            fn(c.parent, c.start, c.seq, c.md, host=True, mem_budget=1 << 20)
    for kw in (dict(eps_ll=0.0), dict(max_outer=0), dict(eps=1e-7), dict(max_len=0.0)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.tree_gamma_fit(c.parent, c.start, c.seq, c.md, host=True, **kw)
    for k, a in ((0, 1.0), (17, 1.0), (4, 0.01), (4, 200.0)):
        with pytest.raises(E.EngineError, match="error -1"):
            E.gamma_rates(k, a)
    assert E.gamma_need(n, L, 4) == 64 * 4 * n * L + n * L + 40 * L + (1 << 20)
    cols = E.gamma_lds_cols(4)
    assert cols == 269 and E.gamma_lds_cols(2) == 541 and E.gamma_lds_cols(16) == 65 and E.gamma_lds_cols(1) == 1085
    assert E.gamma_need(10, cols + 1, 4) - E.gamma_need(10, cols, 4) == 10 * 257 + 40 + 10 * 128 * (cols + 1)     # the scratch of a slab of all 10 branches
    assert E.gamma_need(65536, 300, 4) - 64 * 4 * 65536 * 300 - 65536 * 300 - 40 * 300 - (1 << 20) == 2048 * 128 * 300   # 1/64 of the messages on a large tree


# ---- the program ----

def sm(name):
    return B.sm(name)


def test_program_start_tree_round_trip_and_log(tmp_path):
    """70_otus from the joins' tree as --start-tree: the fixed-rate fit, then the stage; two rounds and a given alpha keep the test short
    (the estimate runs through the program in test_program_support_labels_are_those_of_the_run_without_the_stage)"""
    start, out, log = tmp_path / "start.tree", tmp_path / "out.tree", tmp_path / "g.log"
    r = B._run([B._bin(), B.FASTA70, "--host", "-sm", sm("HKY85"), "-o", start])
    assert r.returncode == 0, r.stderr
    r = B._run([B._bin(), B.FASTA70, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", start, "--ml-rounds", 2, "--gamma", 4, "--gamma-alpha", 0.8,
                "--gamma-log", log, "-o", out, "-v"])
    assert r.returncode == 0, r.stderr
    assert re.search(r"Discrete Gamma of 4 rates fitted: alpha \d+\.\d+, log-likelihood -\d+\.\d+ -> -\d+\.\d+ in 1 pass\(es\), stop: fixed alpha", r.stderr), r.stderr
    assert re.search(r"^rates: \S+ \S+ \S+ \S+$", r.stderr, re.M) and "shape searches" in r.stderr
    a, b = E.newick_parse(start.read_text()), E.newick_parse(out.read_text())
    assert B.same_topology(a, b) and out.read_text().endswith(";\n")
    # the lengths are, bit for bit, the library's on the same tree: the fixed-rate fit from the start tree's lengths, then the stage
    rows = fasta_rows(B.FASTA70)
    parent = np.asarray(a["parent"], np.int32)
    keep = (np.array(list(rows.values())) >= 0).any(axis=0)
    seq = np.full((len(parent), int(keep.sum())), -2, np.int8)
    for u, nm in enumerate(a["names"]):
        if nm:
            seq[u] = rows[nm][keep]
    m = synth.load_model("HKY85")
    md = E.model_desc(m.type_id, m.pi, m.par)
    blen0 = np.where(parent >= 0, np.clip(np.asarray(a["blen"], float), 0.0, 10.0), 0.0)
    fixed = E.tree_optimize_lengths(parent, blen0, seq, md, max_rounds=2, host=True)
    want = E.tree_gamma_fit(parent, fixed["blen"], seq, md, k=4, alpha=0.8, max_rounds=2, host=True)
    assert np.array_equal(np.asarray(b["blen"])[parent >= 0], want["blen"][parent >= 0])
    # the log: a header, the start, one line per pass, the rates, the reason
    lines = log.read_text().splitlines()
    assert lines[0] == "pass\talpha\tll\trounds" and lines[-1] == "# stop: fixed alpha" and lines[-2].startswith("# rates: ") and len(lines) == 5
    rec = [x.split("\t") for x in lines[1:-2]]
    assert [int(x[0]) for x in rec] == [0, 1] and float(rec[0][1]) == 0.8 and int(rec[0][3]) == 0
    assert float(rec[0][2]) == want["ll_start"] and float(rec[1][2]) == want["ll_final"] >= want["ll_start"] and float(rec[1][1]) == want["alpha"] and int(rec[1][3]) == 2
    assert [float(x) for x in lines[-2][len("# rates: "):].split("\t")] == list(want["rates"])


def fasta_rows(path):
    """the rows of a FASTA file in the codes of the program (msa_encode_table)"""
    import gzip
    rows, name = {}, None
    enc = E.msa_encode_table()
    with gzip.open(path, "rb") as f:
        for line in f:
            line = line.strip()
            if line.startswith(b">"):
                name = line[1:].split()[0].decode(); rows[name] = []
            elif line:
                rows[name].append(enc[np.frombuffer(line, np.uint8)])
    return {k: np.concatenate(v) for k, v in rows.items()}


def test_program_without_the_flag_writes_what_it_wrote_before(tmp_path):
    """70_otus on the host path with --ml-lengths, against the file the parent commit wrote"""
    out = tmp_path / "ml.tree"
    r = B._run([B._bin(), B.FASTA70, "--host", "-sm", sm("HKY85"), "--ml-lengths", "--ml-rounds", 2, "-o", out])
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLD, "70_otus_ml2_host_HKY85.tree"), "rb") as f:
        assert out.read_bytes() == f.read()


def test_program_refusals_come_before_a_device_and_leave_no_file(tmp_path):
    c, names, fa, tree, keep = B.program_case(tmp_path)
    ml = [fa, "-sm", sm("GTR"), "--ml-lengths"]
    before = set(os.listdir(tmp_path))
    for args, msg in (([fa, "-sm", sm("GTR"), "--gamma", "4"], "--gamma goes with --ml-lengths"),
                      (ml + ["--gamma-alpha", "0.5"], "go with --gamma"), (ml + ["--gamma-rounds", "3"], "go with --gamma"),
                      (ml + ["--gamma-eps", "0.1"], "go with --gamma"), (ml + ["--gamma-log", tmp_path / "g.log"], "go with --gamma"),
                      (ml + ["--gamma", "1"], "--gamma must be 2 to 16"), (ml + ["--gamma", "17"], "--gamma must be 2 to 16"),
                      (ml + ["--gamma", "4", "--gamma-alpha", "0.01"], "--gamma-alpha must be 0.05 to 100"),
                      (ml + ["--gamma", "4", "--gamma-alpha", "200"], "--gamma-alpha must be 0.05 to 100"),
                      (ml + ["--gamma", "4", "--gamma-rounds", "0"], "--gamma-rounds"), (ml + ["--gamma", "4", "--gamma-eps", "0"], "--gamma-eps"),
                      (ml + ["--gamma", "4", "--gamma-eps", "-1"], "--gamma-eps"),
                      (ml + ["--gamma", "4", "--mem", "0.0012"], r"--gamma: .* need \d+ bytes .* --mem allows 1200000 bytes"),
                      (ml + ["--gamma", "4", "--mem", "0.0012", "--start-tree", tree], r"--gamma: .* need \d+ bytes .* --mem allows 1200000 bytes")):
        r = B._run([B._bin()] + args + ["-o", tmp_path / "o.tree"])
        assert r.returncode != 0 and re.search(msg, r.stderr), (args, r.stderr)
        assert "device" not in r.stderr, r.stderr
        assert set(os.listdir(tmp_path)) == before, args


def test_program_support_labels_are_those_of_the_run_without_the_stage(tmp_path):
    c, names, fa, tree, keep = B.program_case(tmp_path)
    outs = []
    for flags in ([], ["--gamma", "4"]):
        o = tmp_path / ("s%d.tree" % len(flags))
        r = B._run([B._bin(), fa, "--host", "-sm", sm("GTR"), "--ml-lengths", "--start-tree", tree, "--support", 50, "-o", o] + flags)
        assert r.returncode == 0, r.stderr
        outs.append(E.newick_parse(o.read_text()))
    a, b = outs
    assert B.same_topology(a, b) and any(re.fullmatch(r"[01]\.\d{3}", nm or "") for nm in a["names"])
    assert not np.array_equal(a["blen"], b["blen"])


# ---- the host code under the sanitizers ----

def test_host_code_under_the_sanitizers(tmp_path):
    """hu_gamma_host.cpp and hu_blen_host.cpp (no HIP headers) with tests/san/gamma_driver.cpp under AddressSanitizer + UBSan, run as a
    stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gamma_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "gamma_driver.cpp"), os.path.join(CSRC, "hu_gamma_host.cpp"), os.path.join(CSRC, "hu_blen_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "12 cases" in r.stdout


# ---- the device ----

# leaves, columns, categories: the edges of a thread's stride (256 columns) and of a wave, one column, the column counts on either side
# of the switch from LDS to the global scratch for K = 1, 2 and 4, and 16 categories at the one shape where they stay in LDS
DEVICE_SHAPES = [(3, 1, 1), (3, 1, 4), (4, 63, 2), (5, 64, 4), (33, 65, 16), (33, 65, 1), (4, 255, 4), (5, 256, 2), (33, 257, 4), (5, 1000, 2), (33, 1000, 4), (4, 1000, 1),
                 (5, E.gamma_lds_cols(2), 2), (5, E.gamma_lds_cols(2) + 1, 2), (5, E.gamma_lds_cols(4), 4), (5, E.gamma_lds_cols(4) + 1, 4),
                 (4, E.gamma_lds_cols(1), 1), (4, E.gamma_lds_cols(1) + 1, 1)]
ALPHA_OF = {1: 1.0, 2: 5.0, 4: 0.5, 16: 0.3}


def step_deviation(c, k, alpha, got):
    ref = RefGamma(c, k, alpha, c.start)
    return max(deviation(ref, got, u, c.start[u]) for u in range(1, len(c.parent)))


def test_host_scores_on_the_devices_shapes():
    """the host path is the device tests' measure of t*, so it is held to the restatement on their inputs too"""
    worst = 0.0
    for n_leaves, L, k in DEVICE_SHAPES:
        c = B.device_case(n_leaves, L)
        got = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, k=k, alpha=ALPHA_OF[k], host=True, min_len=c.min_len, max_len=c.max_len)
        worst = max(worst, step_deviation(c, k, ALPHA_OF[k], got))
    print("largest deviation of the host path's scores on the device's shapes: %.3g" % worst)
    assert worst <= SCORE_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 4])
def test_scores_against_the_restatement_device(k):
    B._need_gpu()
    worst = max(score_deviation(c, k, alpha, host=False) for c in B.cases() for alpha in (0.3, 1.0, 5.0))
    print("largest deviation of the device's scores, K %d: %.3g" % (k, worst))
    assert worst <= SCORE_BAR


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L,k", DEVICE_SHAPES)
def test_device_against_host(n_leaves, L, k):
    """t* within 2 tau of the host path's, the scores under the bar, the same bits twice"""
    B._need_gpu()
    c = B.device_case(n_leaves, L)
    kw = dict(k=k, alpha=ALPHA_OF[k], min_len=c.min_len, max_len=c.max_len)
    host = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, host=True, **kw)
    dev = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, **kw)
    again = E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, **kw)
    for key in ("t_star", "f", "d1", "d2", "capped"):
        assert np.array_equal(dev[key], again[key]), key
    assert dev["n_capped"] == 0 and host["n_capped"] == 0
    gap = np.abs(dev["t_star"] - host["t_star"]).max()
    worst = step_deviation(c, k, ALPHA_OF[k], dev)
    print("n %d L %d K %d: largest |t* device - t* host| %.3g, largest score deviation %.3g" % (n_leaves, L, k, gap, worst))
    assert gap <= 2 * TAU and worst <= SCORE_BAR
    sc = E.tree_gamma_branch_scores(c.parent, c.start, c.seq, c.md, k=k, alpha=ALPHA_OF[k])
    assert np.array_equal(sc["f"], dev["f"]) and np.array_equal(sc["d1"], dev["d1"]) and np.array_equal(sc["d2"], dev["d2"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_leaves,L,k", [(33, 257, 4), (5, 64, 16), (130, 255, 2)])
def test_per_category_values_are_those_of_the_fixed_rate_sweep(n_leaves, L, k):
    """per_cat of hu_tree_gamma_loglik against hu_tree_loglik on hu_tree_evaluate at the lengths rate_c blen, bit for bit: the sweep over
    the categories is the fixed-rate sweep; and K runs of the fixed-rate kernels in its place give the same"""
    B._need_gpu()
    import torch
    c = B.device_case(n_leaves, L)
    n = len(c.parent)
    got = E.tree_gamma_loglik(c.parent, c.start, c.seq, c.md, k=k, alpha=ALPHA_OF[k])
    rho = E.gamma_rates(k, ALPHA_OF[k])
    up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    for ci in range(k):
        E.tree_evaluate(c.parent, rho[ci] * c.start, c.seq, c.md, up.data_ptr(), down.data_ptr())
        torch.cuda.synchronize()
        per, tot = E.tree_loglik(n, L, 0, c.md, up.data_ptr())
        assert np.array_equal(per, got["per_cat"][ci]), ci
    mx = got["per_cat"].max(0)
    want = mx + np.log(np.exp(got["per_cat"] - mx).mean(0))
    assert np.abs(got["per_col"] - want).max() <= 1e-12 * np.abs(want).max() and got["ll"] == sum(got["per_col"].tolist())
    ref = ref_loglik(c, k, ALPHA_OF[k], c.start)
    assert abs(got["ll"] - ref) <= SCORE_BAR * abs(ref)
    rer = E.tree_gamma_loglik(c.parent, c.start, c.seq, c.md, k=k, alpha=ALPHA_OF[k], sweep_reruns=True)
    assert np.array_equal(rer["per_cat"], got["per_cat"]) and rer["ll"] == got["ll"]


@pytest.mark.gpu
def test_fit_on_the_device_against_the_host_path():
    B._need_gpu()
    c = why_case()
    r = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, max_rounds=1000)
    h = c.fit
    print(r["stop"], r["alpha"], h["alpha"], r["ll_final"], h["ll_final"], len(r["passes"]))
    check_fit(c, r, 4)
    assert len(r["passes"]) == len(h["passes"]) and r["stop"] == h["stop"]
    assert abs(r["alpha"] / h["alpha"] - 1) <= 1e-6
    assert abs(r["ll_final"] - h["ll_final"]) <= SCORE_BAR * abs(h["ll_final"])
    assert np.abs(r["blen"] - h["blen"]).max() <= 2 * EPS
    again = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=4, max_rounds=1000)
    assert np.array_equal(again["blen"], r["blen"]) and again["alpha"] == r["alpha"]
    # beyond LDS (K = 16 at 400 columns), a fixed alpha: one pass on the global scratch, against the host path
    r16 = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=16, alpha=0.5, max_rounds=1000)
    h16 = E.tree_gamma_fit(c.parent, c.fixed["blen"], c.seq, c.md, k=16, alpha=0.5, max_rounds=1000, host=True)
    assert np.abs(r16["blen"] - h16["blen"]).max() <= 2 * EPS and abs(r16["ll_final"] - h16["ll_final"]) <= SCORE_BAR * abs(h16["ll_final"])


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers():
    B._need_gpu()
    c = B.cases()[0]
    n, L = c.seq.shape
    with pytest.raises(E.EngineError, match=r"error -4: .*need %d bytes .*budget is 1048576 bytes" % E.gamma_need(n, L, 4)):
        E.tree_gamma_branch_step(c.parent, c.start, c.seq, c.md, k=4, mem_budget=1 << 20)


@pytest.mark.gpu
def test_program_on_the_device_against_the_host_path(tmp_path):
    """hmmufotu-amd-tree --gamma 4 on 70_otus: the same topology and names, the lengths within 2 eps"""
    B._need_gpu()
    start = tmp_path / "start.tree"
    r = B._run([B._bin(), B.FASTA70, "--host", "-sm", sm("HKY85"), "-o", start])
    assert r.returncode == 0, r.stderr
    outs = []
    for flags in (["--host"], []):
        o = tmp_path / ("g%d.tree" % len(flags))
        r = B._run([B._bin(), B.FASTA70, "-sm", sm("HKY85"), "--ml-lengths", "--start-tree", start, "--ml-rounds", 2, "--gamma", 4, "--gamma-alpha", 0.8, "-o", o, "-v"] + flags)
        assert r.returncode == 0, r.stderr
        assert "Discrete Gamma of 4 rates fitted" in r.stderr
        outs.append(E.newick_parse(o.read_text()))
    a, b = outs
    assert B.same_topology(a, b)
    assert np.abs(np.asarray(a["blen"]) - np.asarray(b["blen"])).max() <= 2 * EPS
