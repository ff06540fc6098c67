"""hmmufotu-amd-train-dm: MSA -> the Dirichlet prior file (src/hmmufotu-train-dm.cpp:88-374).

Every check is a Python restatement written here from the reference: the scaled weights and weighted counts (MSA::sclaleWeight,
MSA::updateWeightedCounts, src/MSA.cpp:280-293), the five training sets of src/hmmufotu-train-dm.cpp:253-333 with their search loop
that drops a transition into the last column, momentInit, weightGradient, cost, compPostP and trainML of
src/math/DirichletDensity.cpp and src/math/DirichletMixture.cpp with the epsilons of src/BandedHMMP7Prior.cpp:32-35, and Eigen's
isApprox.  lgamma and digamma are numpy functions of this file (shift to x >= 15, then the Stirling series), pinned to 50-digit values
in tests/golden/dm_special.npz (tests/golden/make_dm_special_golden.py).  Both errors are taken relative to max(1, |f(x)|): lgamma has
roots at 1 and 2 as digamma has one at 1.4616.

Bars.  numpy special functions: 1e-13 (some twenty operations on intermediates below 40, each within an ulp or two; measured 7.9e-15
for lgamma, 1.0e-15 for digamma).  Device digamma: 64 ulp = 1.5e-14 (at most ten divisions and additions of the recurrence, a
logarithm, a division and seven terms of the series, each within an ulp or two of an intermediate no larger than 2.4 max(1, |psi|)).
Device lgamma: the measured maximum, 2.2e-16, rounded up to one digit, times 4: 1.2e-15 (it may not exceed 1e-12).  Host moment fit: 1e-9.  Trained alpha,
q and cost: 1e-6; what is read back from a written file: 5e-6.  Training data: bit for bit.

CPU part: refusals of the program, the shuffle against std::random_shuffle itself, the moment fit, the writer against the reference's
own file byte for byte, the host entries under AddressSanitizer + UBSan, the numpy special functions.
GPU part: the training data, the device's special functions, the optimiser at fixed iteration counts, independence of the chunk and
of the batch, convergence and the four other ways a training ends, the program on 70_otus, and the chain train-dm -> train-hmm ->
build --no-hmm -> sim -> hmmufotu-amd against the oracle's pipeline."""
import functools
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from hmmufotu_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINDIR = os.path.join(ROOT, "hmmufotu_amd", "bin")
BIN, TRAINHMM, BUILD, SIM, CLI = (os.path.join(BINDIR, x) for x in ("hmmufotu-amd-train-dm", "hmmufotu-amd-train-hmm", "hmmufotu-amd-build",
                                                                    "hmmufotu-amd-sim", "hmmufotu-amd"))
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70, TREE70, DM = os.path.join(REF, "70_otus.fasta.gz"), os.path.join(REF, "70_otus.tree"), os.path.join(REF, "gg_97_otus.dm")
SM_JC69 = os.path.join(REF, "gg_97_otus_JC69.sm")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dm_special.npz"))
M_, I_, D_, P_ = 0, 1, 2, 3
REL_NUMPY = 1e-13
REL_DIGAMMA = 64 * 2.0 ** -52
REL_LGAMMA = 4 * 3e-16                                       # the measured 2.2e-16 rounded up to one digit, times 4, for other ROCm point releases
REL_HOST = 1e-9
REL_TRAIN = 1e-6
REL_TEXT = 5e-6
WG = 256                                                     # HU_DM_WG: lanes of a training workgroup
EPS = dict(eta=0.001, abs_eps_cost=0.0, rel_eps_cost=1e-6, abs_eps_params=0.0, rel_eps_params=1e-4)


# ----------------------------------------------------------------------------- special functions in numpy
def np_shift(x, to=15.0):
    """z = x + n >= to and the product x (x + 1) .. (x + n - 1), for x > 0"""
    z = np.array(x, np.float64, copy=True)
    prod = np.ones_like(z)
    for _ in range(int(to)):
        low = z < to
        prod = np.where(low, prod * z, prod)
        z = np.where(low, z + 1, z)
    return z, prod


def np_lgamma(x):
    z, prod = np_shift(np.asarray(x, np.float64))
    f = 1 / (z * z)
    series = (1 / z) * (1 / 12 - f * (1 / 360 - f * (1 / 1260 - f * (1 / 1680 - f * (1 / 1188 - f * (691 / 360360 - f * (1 / 156)))))))
    return ((z - 0.5) * np.log(z) - z + 0.5 * np.log(2 * np.pi) + series) - np.log(prod)


def np_digamma(x):
    z = np.array(x, np.float64, copy=True)
    r = np.zeros_like(z)
    for _ in range(15):
        low = z < 15.0
        with np.errstate(divide="ignore"):
            r = np.where(low, r - 1 / z, r)
        z = np.where(low, z + 1, z)
    f = 1 / (z * z)
    series = f * (1 / 12 - f * (1 / 120 - f * (1 / 252 - f * (1 / 240 - f * (1 / 132 - f * (691 / 32760 - f * (1 / 12)))))))
    return r + (np.log(z) - 0.5 / z - series)


def special_err(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ----------------------------------------------------------------------------- the restatement: training data
def py_encode_table():
    """encode(toupper(c)) of IUPACNucl (src/IUPACNucl.cpp:34-50, src/DegenAlphabet.cpp:51-63)"""
    first = dict(A="A", C="C", G="G", T="T", U="T", M="A", R="A", W="A", S="C", Y="C", K="G", V="A", H="A", D="A", B="C", N="A")
    t = np.full(256, -1, np.int8)
    for ch in "-._":
        t[ord(ch)] = -2
    for ch, b in first.items():
        t[ord(ch)] = t[ord(ch.lower())] = "ACGT".index(b)
    return t


ENC = py_encode_table()


def ssum(x):
    """the serial sum 0 + x0 + x1 + ..."""
    x = np.asarray(x, np.float64).ravel()
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def as_rows(rows):
    if isinstance(rows, np.ndarray):
        return np.ascontiguousarray(rows, np.uint8)
    return np.frombuffer(b"".join(r.encode("latin1") if isinstance(r, str) else bytes(r) for r in rows), np.uint8).reshape(len(rows), -1)


def py_msa_weights(rows):
    """MSA::updateSeqWeight (src/MSA.cpp:256-278) in numpy"""
    code = ENC[as_rows(rows)].astype(int)
    n, L = code.shape
    cnt = np.stack([(code == b).sum(0) for b in range(4)]).astype(float)
    nz = (cnt > 0).sum(0)
    with np.errstate(divide="ignore"):
        inv = np.where(cnt > 0, 1.0 / (nz[None, :] * cnt), 0.0)
    res = code >= 0
    w = np.array([ssum(inv[code[i][res[i]], np.nonzero(res[i])[0]]) for i in range(n)])
    ln = res.sum(1)
    w = np.where(ln > 0, w / np.maximum(ln, 1), w)
    return w * (n / ssum(w))


def py_training_data(rows, weight, pri_rate=0.05, symfrac=0.5):
    """src/hmmufotu-train-dm.cpp:236-333.  Every entry is the sum of the scaled weights of its rows in ascending i, which is the order
    the reference adds them in (j outer, i inner, one entry per (state pair, j)).  The next cell of (i, j) is the first k > j that is
    a match column or holds a residue; the reference's loop leaves k one past it and drops the cell when k >= L, so a next cell in
    column L - 1 is dropped as "none" is."""
    code = ENC[as_rows(rows)]
    n, L = code.shape
    w = np.asarray(weight, np.float64) * ((1 / pri_rate) / n)                           # sclaleWeight
    wres = np.stack([np.cumsum(np.where(code == b, w[:, None], 0.0), 0)[-1] for b in range(4)])      # updateWeightedCounts
    wgap = np.cumsum(np.where(code == -2, w[:, None], 0.0), 0)[-1]
    num = (wres[0] + wres[2]) + (wres[1] + wres[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        mask = num / (num + wgap) >= symfrac
    res = code >= 0
    own = np.where(mask[None, :], np.where(res, M_, D_), np.where(res, I_, P_))
    nxt = np.full(own.shape, P_)
    for i in range(n):
        at = np.nonzero(own[i] != P_)[0]
        ok = at[1:] + 1 < L                                                             # k = (found column) + 1 must stay below L
        nxt[i, at[:-1][ok]] = own[i, at[1:][ok]]
    me, ie, mt, it, dt = [], [], [], [], []
    for j in range(L):
        (me if mask[j] else ie).append(wres[:, j])
        if j >= L - 1:
            continue
        t = lambda a, b: ssum(w[(own[:, j] == a) & (nxt[:, j] == b)])
        cm, ci, cd = [t(M_, M_), t(M_, I_), t(M_, D_)], [t(I_, M_), t(I_, I_)], [t(D_, M_), t(D_, D_)]
        if any(cm):
            mt.append(cm)
        if any(ci):
            it.append(ci)
        if any(cd):
            dt.append(cd)
    arr = lambda v, k: np.array(v, np.float64).reshape(-1, k).T
    return dict(mask=mask, me=arr(me, 4), ie=arr(ie, 4), mt=arr(mt, 3), it=arr(it, 2), dt=arr(dt, 2), own=own, nxt=nxt, w=w)


# ----------------------------------------------------------------------------- the restatement: moment fit and training
def py_moment_init(data, L=1, idx=None):
    """DirichletDensity::momentInit (src/math/DirichletDensity.cpp:105-133) for L = 1, DirichletMixture::momentInit
    (src/math/DirichletMixture.cpp:208-252) otherwise; alpha [K][L]"""
    data = np.asarray(data, np.float64)
    K, M = data.shape
    alpha = np.ones((K, L))
    if M < (2 if L == 1 else 2 * L):
        return alpha
    x = data if L == 1 else data[:, idx]
    s = x.sum(0)
    N = s.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        x = x * (N / s)
        for j in range(L):
            blk = x if L == 1 else x[:, j * M // L: j * M // L + M // L]
            mean = blk.mean(1)
            var = ((blk - mean[:, None]) ** 2).sum(1) / blk.shape[1]
            an = 0.0
            for i in range(K):
                an = (var[i] - N * mean[i] + 1) / (mean[i] - 1 / N - var[i])
                if an > 0:
                    break
            if an <= 0:
                continue
            alpha[:, j] = mean * an / N
    return alpha


def py_logp(data, alpha, pre=None):
    """logP [L][M] of compPostP / lpdf: C + S, for all components and columns at once.  pre: the terms that hold no alpha"""
    n = data.sum(0)
    lg_n1, lg_d1 = pre if pre is not None else (np_lgamma(n + 1), np_lgamma(data + 1))
    asum = alpha.sum(0)
    lg_a = np_lgamma(np.concatenate([alpha.ravel(), asum]))
    lg_alpha, lg_asum = lg_a[:alpha.size].reshape(alpha.shape), lg_a[alpha.size:]
    C = lg_n1[None, :] + lg_asum[:, None] - np_lgamma(n[None, :] + asum[:, None])
    S = (np_lgamma(data[:, None, :] + alpha[:, :, None]) - lg_d1[:, None, :] - lg_alpha[:, :, None]).sum(0)
    return C + S


def py_train(data, alpha0, q0=None, max_iter=0, eta=0.001, abs_eps_cost=0.0, rel_eps_cost=1e-6, abs_eps_params=0.0, rel_eps_params=1e-4):
    """trainML of a density (alpha0 [K] or [K][1]) or a mixture (alpha0 [K][L]) after its momentInit; the sums unshifted as the reference
    has them.  ratios: deltaC / (rel_eps_cost cOld) of the last two iterations; pratios: |alpha - alpha_old|^2 over isApprox's bound."""
    data = np.asarray(data, np.float64)
    K, M = data.shape
    alpha = np.array(alpha0, np.float64).reshape(K, -1)
    L = alpha.shape[1]
    q = np.full(L, 1.0 / L) if q0 is None else np.array(q0, np.float64)
    w = np.log(alpha)
    n = data.sum(0)
    with np.errstate(all="ignore"):
        cost = lambda lp, q: float(-np.log((q[:, None] * np.exp(lp)).sum(0)).sum()) if L > 1 else float(-lp[0].sum())
        pre = (np_lgamma(n + 1), np_lgamma(data + 1))
        lp = py_logp(data, alpha, pre)
        c = cost(lp, q)
        it, ratios, pratios, status = 0, [], [], None
        while status is None:
            if max_iter > 0 and it >= max_iter:
                status = "max-it"
                break
            it += 1
            c_old, a_old = c, alpha.copy()
            p = q[:, None] * np.exp(lp)
            p = p / p.sum(0)                                                            # compPostP
            asum = alpha.sum(0)
            psi = np_digamma(np.concatenate([alpha.ravel(), asum]))
            psi_alpha, psi_asum = psi[:alpha.size].reshape(alpha.shape), psi[alpha.size:]
            S = (p[None, :, :] * (np_digamma(data[:, None, :] + alpha[:, :, None]) - np_digamma(n[None, :] + asum[:, None])[None, :, :])).sum(2)
            grad = alpha * (p.sum(1)[None, :] * (psi_asum[None, :] - psi_alpha) + S)
            w = w + eta * grad
            alpha = np.exp(w)
            if (alpha == 0).any():
                status, c = "nan-overfit", float("nan")
                break
            if L > 1 and q.min() < 1.0 / M:
                status, c = "nan-unused", float("nan")
                break
            lp = py_logp(data, alpha, pre)
            c = cost(lp, q)
            dc = c_old - c
            p = q[:, None] * np.exp(lp)
            q = (p / p.sum(0)).sum(1) / M
            ratios.append(dc / (abs_eps_cost + rel_eps_cost * c_old))
            prec = abs_eps_params + rel_eps_params * np.sqrt((a_old ** 2).sum())
            bound = prec * prec * min((alpha ** 2).sum(), (a_old ** 2).sum())
            approx = ((alpha - a_old) ** 2).sum() <= bound
            pratios.append(((alpha - a_old) ** 2).sum() / bound)
            if approx and dc >= 0 and dc < abs_eps_cost + rel_eps_cost * c_old:
                status = "converged"
            elif not np.isfinite(c):
                status = "not-finite"
    return dict(alpha=alpha, q=q, cost=c, iterations=it, status=status, ratios=ratios[-2:], pratios=pratios[-2:])


def rel_diff(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(d)) if d.size else 0.0


def check_trained(got, want, what, bar=REL_TRAIN):
    assert got["status"] == want["status"] and got["iterations"] == want["iterations"], (what, got["status"], got["iterations"], want["status"], want["iterations"])
    if want["status"].startswith("nan"):
        assert np.isnan(got["cost"])
        return 0.0
    d = max(rel_diff(got["alpha"], want["alpha"]), rel_diff(got["q"], want["q"]), rel_diff(got["cost"], want["cost"]))
    assert d <= bar, (what, d)
    return d


# ----------------------------------------------------------------------------- inputs
def read_fasta(path):
    op = gzip.open if str(path).endswith(".gz") else open
    names, seqs = [], []
    with op(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0]); seqs.append([])
            else:
                seqs[-1].append(line.strip())
    return names, ["".join(s) for s in seqs]


def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for nm, s in zip(names, seqs):
            f.write(">%s made up\n" % nm)
            for a in range(0, len(s), 60):
                f.write(s[a:a + 60] + "\n")


def make_columns(rng, K, M, conc=None):
    """Dirichlet-multinomial-like columns of total weight <= 20, every fifth with an entry that is exactly 0"""
    conc = rng.uniform(0.3, 4.0, K) if conc is None else conc
    d = rng.dirichlet(conc, M).T * rng.uniform(0.5, 20.0, M)
    d[rng.integers(0, K, M)[::5], np.arange(M)[::5]] = 0.0
    return d


@functools.lru_cache(None)
def otus70():
    """the restatement on the pruned 70_otus alignment: rows, weights, the five training sets"""
    rows = as_rows(read_fasta(FASTA70)[1])
    rows = np.ascontiguousarray(rows[:, (ENC[rows] >= 0).any(0)])
    w = py_msa_weights(rows)
    td = py_training_data(rows, w)
    return types.SimpleNamespace(rows=rows, w=w, td=td)


@functools.lru_cache(None)
def otus70_mixtures(max_iter, n_seed, seed=1):
    """n_seed independent restatement runs of the match-emission mixture (qM = 5), their shuffles drawn one after the other from
    srand(seed) by hu_dm_shuffle, which test_shuffle pins to std::random_shuffle"""
    me = otus70().td["me"]
    out = []
    for s in range(n_seed):
        idx = E.dm_shuffle(me.shape[1], seed if s == 0 else None)
        out.append(py_train(me, py_moment_init(me, 5, idx), max_iter=max_iter))
    return out


@functools.lru_cache(None)
def otus70_densities(max_iter):
    td = otus70().td
    return {k: py_train(td[k], py_moment_init(td[k]), max_iter=max_iter) for k in ("ie", "mt", "it", "dt")}


def run(args, cwd, binary=BIN):
    return subprocess.run([binary] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=600)


def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ============================================================================= CPU
def test_program_is_built():
    assert os.path.exists(BIN), "hmmufotu-amd-train-dm missing: run __graft_entry__.build()"
    assert np.array_equal(ENC, E.msa_encode_table())


def test_numpy_special_functions():
    x = GOLD["x"]
    assert len(x) == 222 and abs(x.min() / 1e-5 - 1) < 1e-12 and abs(x.max() / 1e4 - 1) < 1e-12 and (np.abs(x - 1.4616321449683623) < 1e-9).sum() >= 10
    e_lg, e_dg = special_err(np_lgamma(x), GOLD["lgamma"]), special_err(np_digamma(x), GOLD["digamma"])
    print("numpy lgamma and digamma against 50 digits: %.3g, %.3g" % (e_lg, e_dg))
    assert e_lg <= REL_NUMPY and e_dg <= REL_NUMPY


def test_refusals(tmp_path):
    rng = np.random.default_rng(3)
    names = ["s%d" % i for i in range(6)]
    seqs = ["".join(rng.choice(list("ACGT-"), 80)) for _ in names]
    fa = tmp_path / "hand.fasta"
    write_fasta(fa, names, seqs)

    def refused(args, *words):
        r = run(args, tmp_path)
        lines = [x for x in r.stderr.strip().split("\n") if x]
        assert r.returncode != 0 and r.stdout == "" and len(lines) == 1 and all(w in lines[0] for w in words), (args, r.returncode, r.stderr)
        assert "device" not in r.stderr                # refused before a device is asked for: this test runs without one

    refused([fa, "--fmt", "msa"], "'msa'", "not read here")
    msa = tmp_path / "hand.msa"; msa.write_bytes(b"HmmUFOtu")
    refused([msa], "'msa'", "not read here")
    refused([fa, "--fmt", "fastq"], "Unsupported sequence format 'fastq'")
    for bad in ("1", "0", "11", "-3"):
        refused([fa, "-qM", bad], "-qM must between 2 and 10")
    for bad in ("-0.25", "1.5", "nan"):
        refused([fa, "-symfrac", bad], "-symfrac must between 0 and 1")
    for bad in ("0", "1.01", "-1", "nan"):
        refused([fa, "--pri-rate", bad], "--pri-rate must be in (0, 1]")
    refused([fa, "--max-it", "-1"], "--max-it must be a non-negative integer")
    for bad in ("0", "-2"):
        refused([fa, "-n", bad], "-n must be between 1 and")
    refused([fa, "--chunk", "-1"], "--chunk must be a positive integer")
    wide = tmp_path / "wide.fasta"                                                     # 65,536 columns stay after pruning
    write_fasta(wide, ["a", "b"], ["ACGT" * 16384 + "--", "-" * 65535 + "A" + "--"])
    refused([wide, "-o", "out.dm"], "65536 columns after pruning", "65535")
    refused([tmp_path / "missing.fasta"], "Unable to open seq file")
    assert not os.path.exists(tmp_path / "out.dm")


SHUFFLE_DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char** argv) {
	srand((unsigned) atoi(argv[1]));
	for(int a = 2; a < argc; ++a) {
		std::vector<int> idx(atoi(argv[a]));
		for(size_t t = 0; t < idx.size(); ++t) idx[t] = (int) t;
		std::random_shuffle(idx.begin(), idx.end());
		for(int v : idx) printf("%d ", v);
		printf("\n");
	}
}
"""


def test_shuffle(tmp_path):
    """hu_dm_shuffle against srand(seed); std::random_shuffle(...) itself, a second shuffle from the same stream included"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    (tmp_path / "shuffle.cpp").write_text(SHUFFLE_DRIVER)
    exe = str(tmp_path / "shuffle")
    r = subprocess.run(["g++", "-std=c++11", "-Wno-deprecated-declarations", "-o", exe, str(tmp_path / "shuffle.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = [1, 2, 10, 1285, 1285, 10]
    for seed in (1, 20261018):
        out = subprocess.run([exe, str(seed)] + [str(m) for m in sizes], capture_output=True, text=True, check=True).stdout.strip("\n").split("\n")
        for k, m in enumerate(sizes):
            got = E.dm_shuffle(m, seed if k == 0 else None)
            want = np.array(out[k].split(), np.int32)
            assert np.array_equal(got, want), (seed, k, m)
            assert sorted(got) == list(range(m))
        assert not np.array_equal(E.dm_shuffle(1285, seed), np.arange(1285))
    assert len(E.dm_shuffle(0)) == 0


def test_moment_init():
    rng = np.random.default_rng(11)
    worst = 0.0
    for K in (2, 3, 4):                                                                 # densities
        for M in (1, 2, 50):
            d = make_columns(rng, K, M)
            got, want = E.dm_moment_init(d), py_moment_init(d)
            assert got.shape == (K, 1)
            worst = max(worst, rel_diff(got, want))
            assert (got == 1).all() if M < 2 else (got != 1).all()
    for L, M in ((2, 3), (5, 9), (10, 19)):                                             # M = 2 L - 1: skipped
        d = make_columns(rng, 4, M)
        assert (E.dm_moment_init(d, L, E.dm_shuffle(M, 5)) == 1).all() and (py_moment_init(d, L, np.arange(M)) == 1).all()
    for L, M in ((2, 4), (5, 10), (10, 20), (3, 50), (5, 1285), (7, 100)):              # M = 2 L, and M that L does not divide
        d = make_columns(rng, 4, M)
        idx = E.dm_shuffle(M, 7)
        got, want = E.dm_moment_init(d, L, idx), py_moment_init(d, L, idx)
        worst = max(worst, rel_diff(got, want))
        assert got.shape == (4, L)
    # block 0: its first category is constant (variance 0, mean 1 / N: 0 / 0, no alphaNorm > 0), its second fits; block 1: every
    # column the same, so no category fits and its alpha stays 1
    blk0 = make_columns(rng, 4, 6, conc=np.array([5.0, 1.0, 1.0, 1.0])) + 0.05
    blk0 = blk0 / blk0.sum(0) * 10.0
    blk0[0] = 5.0; blk0[1:] = blk0[1:] / blk0[1:].sum(0) * 5.0
    blk1 = np.tile(np.array([[4.0], [3.0], [2.0], [1.0]]), (1, 6))
    d = np.concatenate([blk0, blk1], 1)
    want = py_moment_init(d, 2, np.arange(12))
    got = E.dm_moment_init(d, 2, np.arange(12))
    assert (want[:, 1] == 1).all() and (want[:, 0] != 1).all() and (got[:, 1] == 1).all()
    mean = (blk0 * (10.0 / blk0.sum(0))).mean(1); var = ((blk0 - mean[:, None]) ** 2).sum(1) / 6
    assert not (var[0] - 10 * mean[0] + 1) / (mean[0] - 0.1 - var[0]) > 0               # the first category does not fit, a later one does
    worst = max(worst, rel_diff(got, want))
    print("moment fit against the restatement: %.3g" % worst)
    assert worst <= REL_HOST
    with pytest.raises(E.EngineError):
        E.dm_moment_init(d, 2, np.arange(12) + 1)                                        # an index out of range


def test_writer(tmp_path):
    """the reference's own file read and written back: byte for byte"""
    text = open(DM).read()
    costs = [float(l.split(":")[1]) for l in text.split("\n") if l.startswith("Training cost:")]
    assert costs == [7098.26, 571.255, 592.092, 65.7982, 258.478]
    p = E.hmm_prior_read(DM).as_dict()
    out = tmp_path / "back.dm"
    E.dm_write(out, p["me_q"], p["me_alpha"], p["ie_alpha"], p["mt_alpha"], p["it_alpha"], p["dt_alpha"], costs)
    assert out.read_bytes() == open(DM, "rb").read()
    rng = np.random.default_rng(2)
    digits15 = lambda v: np.array([float("%.15g" % x) for x in np.ravel(v)]).reshape(np.shape(v))
    for L in (2, 10):                                                                   # numbers of 15 digits come back from 16 printed ones exactly
        q = digits15(rng.dirichlet(np.ones(L))); a = digits15(np.exp(rng.normal(0, 3, (4, L))))
        dens = [digits15(np.exp(rng.normal(0, 4, k))) for k in (4, 3, 2, 2)]
        E.dm_write(out, q, a, *dens, [1e-7, 123456789.0, 0.0, 65.7982, 1.5])
        back = E.hmm_prior_read(out)
        g = back.as_dict()
        assert back.me_L == L and np.array_equal(g["me_q"], q) and np.array_equal(g["me_alpha"], a)
        assert all(np.array_equal(g[k], v) for k, v in zip(("ie_alpha", "mt_alpha", "it_alpha", "dt_alpha"), dens))
        lines = out.read_text().split("\n")
        assert lines[2] == "Training cost: 1e-07" and "Training cost: 1.23457e+08" in lines and lines[3] == "K: 4 L: %d" % L
        assert len({len(l) for l in lines[7:11]}) == 1                                  # the alpha rows are aligned
    with pytest.raises(E.EngineError, match="unable to write"):
        E.dm_write(tmp_path / "no" / "dir.dm", p["me_q"], p["me_alpha"], p["ie_alpha"], p["mt_alpha"], p["it_alpha"], p["dt_alpha"], costs)


def test_sanitizer_on_the_moment_fit_and_the_writer(tmp_path):
    """hu_dm_host.cpp, hu_hmm_io.cpp and tests/san/dm_train_driver.cpp under g++ -fsanitize=address,undefined, run stand-alone"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dm_train_driver")
    csrc = os.path.join(ROOT, "hmmufotu_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
           os.path.join(ROOT, "tests", "san", "dm_train_driver.cpp"), os.path.join(csrc, "hu_dm_host.cpp"), os.path.join(csrc, "hu_hmm_io.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, DM, str(tmp_path / "scratch.dm"), "400"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + "\n" + r.stderr[-4000:])
    assert "400 trials" in r.stdout and "byte for byte" in r.stdout


# ============================================================================= GPU: the training data
LETTERS = list("ACGT") * 6 + list("acgt") * 2 + list("RYKMSWBDHVNUn") + list("---..__") * 2 + list("!*Z0 ")
SETS = ("me", "ie", "mt", "it", "dt")


def random_rows(rng, n, L, gappy=0.0):
    a = rng.choice(np.frombuffer("".join(LETTERS).encode(), np.uint8), (n, L))
    a[rng.random((n, L)) < gappy] = ord("-")
    return np.ascontiguousarray(a)


def check_data(rows, w, pri_rate=0.05, symfrac=0.5, what=""):
    rows = as_rows(rows)
    want = py_training_data(rows, w, pri_rate, symfrac)
    got = E.dm_training_data(rows, w, pri_rate, symfrac)
    assert np.array_equal(got["mask"], want["mask"]), what
    for k, dim in zip(SETS, (4, 4, 3, 2, 2)):
        assert got[k].shape == want[k].shape and got[k].shape[0] == dim, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)                               # bit for bit
    for k in ("mt", "it", "dt"):
        assert (got[k] != 0).any(0).all()                                               # no all-zero column
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 256, 257])
def test_training_data_on_random_rows(L):
    need_gpu()
    for n in (1, 2, 7, 8, 9, 513):
        rng = np.random.default_rng(1000 * n + L)
        rows = random_rows(rng, n, L, gappy=0.35)                                        # lower-case, IUPAC and invalid bytes among them
        rows[0, 0] = ord("A")
        w = rng.random(n) * 2 + 0.01
        for pri_rate in (0.05, 1.0):
            got, want = check_data(rows, w, pri_rate, 0.5, "random %d x %d at %g" % (n, L, pri_rate))
        if n >= 7 and L >= 63:
            assert got["mt"].shape[1] > 0 and got["it"].shape[1] > 0 and got["dt"].shape[1] > 0 and (got["mt"][2] > 0).any() and (got["dt"][1] > 0).any()
        if L == 1:
            assert got["mt"].shape[1] == got["it"].shape[1] == got["dt"].shape[1] == 0


def hand_rows(cols):
    """rows from column strings"""
    return np.ascontiguousarray(np.array([np.frombuffer(c.encode(), np.uint8) for c in cols]).T)


@pytest.mark.gpu
def test_training_data_drops_transitions_into_the_last_column():
    """The reference's search loop (src/hmmufotu-train-dm.cpp:287-294) increments k past the cell it found before it tests k >= L.
    Four rows, equal weights; a column is a match column when at least two of its four rows hold a residue (symfrac 0.5)."""
    need_gpu()
    w = np.ones(4)
    #                 j = 0     1       2       3 (L - 2)  4 (L - 1)
    for last, kind in (("ACGT", "match column with residues"), ("A-C-", "match column, rows 1 and 3 deleted"), ("---G", "insert column with a residue")):
        rows = hand_rows(["ACGT", "AC-T", "---A", "AC-T", last])
        got, want = check_data(rows, w, 1.0, 0.5, kind)
        assert list(want["mask"]) == [True, True, False, True, last != "---G"]
        # column 3 would hold M->M (or M->D, or M->I) into column 4: none is counted, so match column 3 has no column in MT and DT,
        # and the transitions into column 3 = L - 2 are there: from column 1 (M->M rows 0 1, D->D row 2; row 3 goes M->I) and 2 (I->M)
        assert got["mt"].shape == (3, 2) and got["dt"].shape == (2, 1) and got["it"].shape == (2, 1), (kind, got["mt"], got["dt"], got["it"])
        scale = 1.0 / 4
        assert np.array_equal(got["mt"], np.array([[3, 2], [0, 1], [1, 0]]) * scale)
        assert np.array_equal(got["it"][:, 0], np.array([1, 0]) * scale) and np.array_equal(got["dt"][:, 0], np.array([0, 1]) * scale)
        assert got["me"].shape[1] == int(want["mask"].sum()) and got["ie"].shape[1] == 5 - int(want["mask"].sum())      # emissions: every column


@pytest.mark.gpu
def test_training_data_on_hand_made_alignments():
    need_gpu()
    rng = np.random.default_rng(77)
    cols, kinds = [], [("m", 3), ("i", 70), ("m", 2), ("i", 300), ("m", 4), ("i", 9), ("m", 2)]
    for kind, length in kinds:                                                          # insert runs of 70 and 300 columns
        for _ in range(length):
            c = rng.choice(np.frombuffer(b"ACGTacgtRN", np.uint8), 12)
            c[rng.random(12) < (0.1 if kind == "m" else 0.8)] = rng.choice(np.frombuffer(b"-._!", np.uint8))
            cols.append(c)
    rows = np.ascontiguousarray(np.stack(cols, 1))
    rows[4, 3:73] = ord("-"); rows[4, 75:375] = ord("_")                                # M -> M across 70 and 300 columns
    rows[5, 3:73] = ord("-"); rows[5, 72] = ord("A")                                    # one insert at the far end of a run
    rows[:, 376] = np.frombuffer(b"A-C-G-T-A-C-", np.uint8); rows[:, 377] = np.frombuffer(b"-A-C-G-T-A-C", np.uint8)
    rows[1, :] = ord("-")                                                               # a row without a residue
    w = py_msa_weights(rows)
    assert w[1] == 0
    got, want = check_data(rows, w, 0.05, 0.5, "hand-made")
    K = int(want["mask"].sum())
    assert K >= 10 and got["me"].shape[1] == K and got["ie"].shape[1] == rows.shape[1] - K
    # two columns: every transition of column 0 goes into column L - 1, so no set has a transition column
    g2, _ = check_data(hand_rows(["ACGT", "ACGT"]), np.ones(4), 1.0, 0.5, "two columns")
    assert g2["mt"].shape[1] == g2["it"].shape[1] == g2["dt"].shape[1] == 0 and g2["me"].shape[1] == 2
    # insert column 1 holds one residue whose row is deleted in the next match column: I->D is not counted, the column's counts are
    # all zero, it does not appear, and insert column 3 (I->M) closes up; match column 4 goes into the last column and is absent too
    g5, w5 = check_data(hand_rows(["ACGT", "A---", "-CGT", "-C--", "ACGT", "ACGT"]), np.ones(4), 1.0, 0.5, "a column without counts")
    assert list(w5["mask"]) == [True, False, True, False, True, True]
    assert np.array_equal(g5["it"], np.array([[1.0], [0.0]]) / 4) and np.array_equal(g5["mt"], np.array([[3, 2], [1, 1], [0, 0]]) / 4)
    assert np.array_equal(g5["dt"], np.array([[1.0], [0.0]]) / 4) and g5["ie"].shape[1] == 2
    with pytest.raises(E.EngineError, match="weight"):
        E.dm_training_data(rows, -np.ones(12))
    with pytest.raises(E.EngineError, match="pri_rate"):
        E.dm_training_data(rows, w, 0.0)


@pytest.mark.gpu
def test_training_data_on_70otus():
    need_gpu()
    o = otus70()
    assert o.rows.shape == (125, 1486)
    st = E.msa_stats(o.rows)
    assert rel_diff(st["seq_weight"], o.w) <= 1e-12                                     # the restated weights are the engine's
    got, want = check_data(o.rows, st["seq_weight"], 0.05, 0.5, "70_otus")
    assert [got[k].shape for k in SETS] == [(4, 1285), (4, 201), (3, 1285), (2, 198), (2, 1096)]
    t = E.dm_training_data_timing()
    assert t["peak_bytes"] >= 0 and t["counts_kernel"] > 0 and t["to_device"] > 0                # small buffers may come from memory the runtime already holds


# ============================================================================= GPU: the special functions
@pytest.mark.gpu
def test_device_special_functions():
    """The training kernel's lgamma (the device library's) and digamma (hu_kern_dm.h) at the golden points.  Measured on an MI355X,
    ROCm 7.2: lgamma 2.2e-16, digamma 9.7e-16, relative to max(1, |f|).  The bar for lgamma is that maximum rounded up to one digit, times 4, and
    may not exceed 1e-12: above that the 1e-6 bar on trained parameters has no headroom over thousands of iterations."""
    need_gpu()
    lg, dg = E.dm_special(GOLD["x"])
    e_lg, e_dg = special_err(lg, GOLD["lgamma"]), special_err(dg, GOLD["digamma"])
    print("device lgamma and digamma against 50 digits: %.3g, %.3g" % (e_lg, e_dg))
    assert REL_LGAMMA <= 1e-12
    assert e_lg <= REL_LGAMMA and e_dg <= REL_DIGAMMA




# ============================================================================= GPU: the optimiser
def fixed_problems():
    """densities K = 2, 3, 4 and mixtures K = 4, L = 2, 5, 10 at the sizes where a lane takes one column, none, or several"""
    rng = np.random.default_rng(2026)
    out = []
    for K in (2, 3, 4):
        for M in (1, 2, 63, 64, 65, WG + 1, 1025):
            d = make_columns(rng, K, M)
            a0 = py_moment_init(d)
            if M == 65:
                a0[0, 0] = 3e-4                                                         # as small as the insert-transition alphas start
            out.append(dict(data=d, alpha0=a0, name="density K=%d M=%d" % (K, M)))
    for L in (2, 5, 10):
        for M in (2 * L, 63, 64, 65, WG + 1, 1025):
            d = make_columns(rng, 4, M)
            a0 = py_moment_init(d, L, rng.permutation(M))
            if M == 64:
                a0[1, L - 1] = 3e-4
            out.append(dict(data=d, alpha0=a0, name="mixture L=%d M=%d" % (L, M)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [1, 2, 25])
def test_optimiser_at_a_fixed_iteration_count(max_iter):
    """alpha, q, cost, iteration count and status against the restatement; bar 1e-6, measured 7.6e-12 over the three counts"""
    need_gpu()
    probs = fixed_problems()
    got = E.dm_train(probs, max_iter=max_iter)
    worst = 0.0
    for p, g in zip(probs, got):
        want = py_train(p["data"], p["alpha0"], max_iter=max_iter)
        assert want["status"] in ("max-it", "converged", "nan-unused"), (p["name"], want["status"])      # small M against large L: a coefficient soon falls below 1 / M
        worst = max(worst, check_trained(g, want, p["name"]))
    print("optimiser after %d iteration(s), %d problems: largest relative difference %.3g" % (max_iter, len(probs), worst))


@pytest.mark.gpu
def test_chunk_and_batch_independence():
    need_gpu()
    probs = [p for p in fixed_problems() if p["name"] in ("density K=2 M=65", "density K=4 M=1025", "density K=3 M=1", "mixture L=2 M=4", "mixture L=5 M=65",
                                                          "mixture L=10 M=1025", "mixture L=10 M=20", "density K=3 M=%d" % (WG + 1), "mixture L=5 M=%d" % (WG + 1))]
    assert len(probs) == 9
    same = lambda a, b: all(np.array_equal(x[k], y[k], equal_nan=True) if k in ("alpha", "q") else (x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]))
                            for x, y in zip(a, b) for k in ("alpha", "q", "cost", "iterations", "status"))
    launches = []
    base = E.dm_train(probs, max_iter=30, progress=lambda it, running: launches.append((it, running)))      # the default chunk
    assert launches == [(30, 0)]
    for chunk in (1, 7):
        launches.clear()
        assert same(E.dm_train(probs, max_iter=30, chunk=chunk, progress=lambda it, running: launches.append((it, running))), base), chunk
        assert len(launches) == -(-30 // chunk) and launches[-1] == (30, 0)
    for k in (0, 5, 8):                                                                 # alone
        assert same(E.dm_train([probs[k]], max_iter=30), [base[k]]), k


def convergence_inputs():
    """a density on 256 columns; an L = 2 mixture on 128 + 128 sparse columns, whose alphas stay below 1 so that isApprox's bound,
    which goes with |alpha|^4, is the criterion that is met last; the shuffle of its moment fit"""
    rng = np.random.default_rng(5150)
    dens = make_columns(rng, 3, 256, conc=np.array([2.0, 0.7, 0.4]))
    rng = np.random.default_rng(5150)
    mix = np.concatenate([make_columns(rng, 4, 128, conc=0.03 * np.array([6.0, 1.0, 1.0, 0.5])), make_columns(rng, 4, 128, conc=0.03 * np.array([0.5, 1.0, 5.0, 2.0]))], 1)
    return dens, mix, rng.permutation(256)


@pytest.mark.gpu
def test_convergence_and_the_exits():
    """(a) A density and an L = 2 mixture on 256 columns run to convergence with max_iter 0 (147 and 411 iterations).  In the
    restatement (measured difference of alpha, q and cost on the device: 7.0e-13) deltaC / (1e-6 cOld) of the second-to-last and the last iteration is 0.399 and 0.375 for the density, 0.160 and 0.159
    for the mixture: outside [0.9, 1.1], the cost's criterion has long been met.  What ends both runs is isApprox on alpha:
    |alpha - alpha_old|^2 over its bound is 1.052 then 0.989 for the density, 1.006 then 0.994 for the mixture, at least 0.5 per cent
    from 1 where rounding moves it by 1e-10 or so, so rounding cannot move the stop.
    (b) L = 5 on 12 columns ends NaN-unused.  Near-identical columns, which the issue proposed, do not end so from a fresh start: no
    block's moment fit succeeds, all five components start at alpha = 1 and stay equal with q = 1 / 5; Dirichlet-multinomial columns do.
    (c) A step so long that exp(w) underflows to 0 ends NaN-overfit.  (d) max_iter 3 ends max-it after 3 iterations."""
    need_gpu()
    dens, mix, perm = convergence_inputs()
    pa = dict(data=dens, alpha0=py_moment_init(dens))
    pb = dict(data=mix, alpha0=py_moment_init(mix, 2, perm))
    rng = np.random.default_rng(8)
    few = make_columns(rng, 4, 12)
    pc = dict(data=few, alpha0=py_moment_init(few, 5, rng.permutation(12)))
    over = make_columns(rng, 2, 40)
    over[1] = 0.0                                                                       # the second category is never seen: its alpha only falls
    pd = dict(data=over, alpha0=np.array([2.0, 1.0]))
    wa, wb, wc = py_train(**pa), py_train(**pb), py_train(**pc)
    for want in (wa, wb):
        print("converged after %d iterations; deltaC / (1e-6 cOld) of the last two: %s; |alpha - alpha_old|^2 over its bound: %s" % (want["iterations"], want["ratios"], want["pratios"]))
        assert want["status"] == "converged" and len(want["ratios"]) == 2 and all(not 0.9 <= x <= 1.1 for x in want["ratios"])
        assert want["pratios"][0] > 1.005 and want["pratios"][1] < 0.995 and max(want["ratios"]) < 0.9
    assert wc["status"] == "nan-unused" and wc["iterations"] > 1
    ga, gb, gc = E.dm_train([pa, pb, pc])
    d = max(check_trained(ga, wa, "density to convergence"), check_trained(gb, wb, "mixture to convergence"))
    print("to convergence: largest relative difference %.3g" % d)
    assert ga["status"] == gb["status"] == "converged"
    check_trained(gc, wc, "unused component")
    assert gc["status"] == "nan-unused" and np.isnan(gc["cost"])
    wd = py_train(pd["data"], pd["alpha0"], eta=1e4)
    gd = E.dm_train([pd], eta=1e4)[0]
    assert wd["status"] == "nan-overfit" and gd["status"] == "nan-overfit" and gd["iterations"] == wd["iterations"] and np.isnan(gd["cost"])
    g3 = E.dm_train([pa, pb], max_iter=3)
    assert [g["status"] for g in g3] == ["max-it", "max-it"] and [g["iterations"] for g in g3] == [3, 3]
    empty = E.dm_train([dict(data=np.zeros((2, 0)), alpha0=np.ones(2))])[0]             # an empty set trains nothing
    assert empty["status"] == "converged" and empty["iterations"] == 0 and empty["cost"] == 0 and (empty["alpha"] == 1).all()


# ============================================================================= GPU: the program
def read_dm(path):
    p = E.hmm_prior_read(path)
    costs = [float(l.split(":")[1]) for l in open(path).read().split("\n") if l.startswith("Training cost:")]
    return p.as_dict(), costs, int(p.me_L)


def check_file(path, mixture, dens):
    g, costs, L = read_dm(path)
    assert L == 5 and len(costs) == 5
    d = [rel_diff(g["me_q"], mixture["q"]), rel_diff(g["me_alpha"], mixture["alpha"]), rel_diff(costs[0], mixture["cost"])]
    for k, (name, c) in enumerate(zip(("ie", "mt", "it", "dt"), costs[1:])):
        d += [rel_diff(g[name + "_alpha"], dens[name]["alpha"][:, 0]), rel_diff(c, dens[name]["cost"])]
    print("file against the restatement, largest relative difference: %.3g" % max(d))
    assert max(d) <= REL_TEXT, d


@pytest.mark.gpu
def test_program_on_70otus(tmp_path):
    need_gpu()
    r = run([FASTA70, "-o", "p.dm", "--max-it", "200", "-s", "1", "-n", "1", "-v"], tmp_path)
    assert r.returncode == 0, r.stderr
    err = r.stderr.split("\n")
    for line in ("MSA loaded", "MSA pruned", "MSA database created for 125 X 1486 aligned sequences", "Random seed: 1", "Best Match Emission model found at seed 1 after 200 iterations"):
        assert line in err, (line, r.stderr)
    assert r.stdout == "" and sum(l.startswith("  seed ") for l in err) == 1
    check_file(tmp_path / "p.dm", otus70_mixtures(200, 1)[0], otus70_densities(200))
    assert (tmp_path / "p.dm").read_text().startswith("Match emission:\nDirichlet Mixture Model\nTraining cost: ")
    quiet = run([FASTA70, "--max-it", "200", "-s", "1", "--chunk", "13"], tmp_path)      # stdout without -o; another chunk, the same bytes
    assert quiet.returncode == 0 and quiet.stdout == (tmp_path / "p.dm").read_text() and [l for l in quiet.stderr.split("\n") if l and not l.startswith("  seed 1 trained")] == []
    # three seeds side by side: the cheapest of three independent runs is written
    r3 = run([FASTA70, "-o", "p3.dm", "--max-it", "200", "-s", "1", "-n", "3"], tmp_path)
    assert r3.returncode == 0, r3.stderr
    want = otus70_mixtures(200, 3)
    listed = [float(l.split("cost:")[1]) for l in r3.stderr.split("\n") if l.startswith("  seed ")]
    assert len(listed) == 3 and rel_diff(listed, [w["cost"] for w in want]) <= REL_TEXT
    costs = [w["cost"] for w in want]
    assert len(set(costs)) == 3
    check_file(tmp_path / "p3.dm", want[int(np.argmin(costs))], otus70_densities(200))
    # no match column: refused after the data is made
    write_fasta(tmp_path / "gappy.fasta", ["a", "b", "c"], ["AC-GT-", "-CGT-A", "A-G-TA"])
    rk = run(["gappy.fasta", "-symfrac", "0.99"], tmp_path)
    assert rk.returncode != 0 and rk.stdout == "" and "no column of 6 reaches the symbol fraction 0.99" in rk.stderr and rk.stderr.count("\n") == 1


@pytest.mark.gpu
def test_densities_of_70otus_to_convergence():
    """the four densities without a cap through the library entry; the restatement needs 141 (IE), 127 (MT), 5,902 (IT) and 270 (DT)
    iterations; measured difference 5.6e-14"""
    need_gpu()
    td = otus70().td
    want = otus70_densities(0)
    assert [want[k]["iterations"] for k in ("ie", "mt", "it", "dt")] == [141, 127, 5902, 270]
    got = E.dm_train([dict(data=td[k], alpha0=E.dm_moment_init(td[k])) for k in ("ie", "mt", "it", "dt")])
    d = max(check_trained(g, want[k], k) for g, k in zip(got, ("ie", "mt", "it", "dt")))
    print("densities of 70_otus to convergence: largest relative difference %.3g" % d)


@pytest.mark.gpu
def test_trained_prior_in_a_database(tmp_path):
    """train-dm -> train-hmm -dm <that file> -> build --no-hmm -> sim -> hmmufotu-amd: every program exits 0, the profile loads, and
    the engine agrees with the oracle's pipeline on the same two files (the pattern of test_trained_profile_in_a_database)"""
    need_gpu()
    from oracle import oracle_py as O, parity
    r = run([FASTA70, "-o", "own.dm", "--max-it", "300", "-s", "1"], tmp_path)
    assert r.returncode == 0, r.stderr
    h = run([FASTA70, "-dm", "own.dm", "-o", "db.hmm"], tmp_path, TRAINHMM)
    assert h.returncode == 0, h.stderr
    b = run([FASTA70, TREE70, "--no-hmm", "-sm", SM_JC69, "-n", "db"], tmp_path, BUILD)
    assert b.returncode == 0, b.stderr
    s = run(["db", "reads.fa", "-N", "200", "-S", "7", "-m", "400", "-s", "30", "--msa", FASTA70], tmp_path, SIM)
    assert s.returncode == 0, s.stderr
    ids, reads = read_fasta(tmp_path / "reads.fa")
    assert len(reads) == 200
    c = run(["db", "reads.fa", "-o", "out.tsv"], tmp_path, CLI)
    assert c.returncode == 0, c.stderr
    f = E.parse_files(str(tmp_path / "db.hmm"), str(tmp_path / "db.ptu"))
    assert f["K"] == 1285 and f["L"] == 1486
    reads = [x for x in reads if len(x) >= 60]
    assert len(reads) >= 150
    Db = E.Database.load(str(tmp_path / "db.hmm"), str(tmp_path / "db.ptu"))
    hmm = types.SimpleNamespace(K=f["K"], L=f["L"], EM=f["EM"], EI=f["EI"], T=f["T"], p2cs=f["p2cs"])
    vps = E.SeedIndex(f["parent"], f["seq"], hmm).lookup(reads)
    B = E.Batch(Db, len(reads)); B.set_reads(reads, vps); B.assign(E.default_opts())
    recs = B.alignments(want_align=False)["recs"]; best = B.placements(); cand = B.candidates()
    md = f["model"]
    m = O.Model(md.type, list(md.pi), list(md.par))
    H = O.Hmm(f["K"], f["L"], f["EM"], f["EI"], f["T"], f["p2cs"], 0)
    T = O.Tree(f["parent"], f["blen"], f["seq"], f["up"], f["down"], f["height"], m, None, None)
    res = O.pipeline_batch(H, T, reads, vps, opts=O.default_opts(tieMode=1), threads=4, want_cands=True)
    assert (recs["status"] == res["aln_ints"][:, 7]).all() and np.array_equal(recs["cost"], res["cost"])
    assert (recs["status"] == E.READ_OK).sum() >= 0.9 * len(reads)
    assert (best["n_cand"] == res["n_cand"]).all()
    per = []
    for i in np.nonzero(recs["status"] == E.READ_OK)[0]:
        k = int(res["n_cand"][i]); a, b_ = int(cand["offs"][i]), int(cand["offs"][i + 1])
        per.append(parity.classify_read(res["cand_node"][i, :k], res["cand_est"][i, :k], res["cand_ratio0"][i, :k], cand["c_node"][a:b_], f["parent"],
                                        pos=int(res["best_pos"][i])))
    tot = parity.summarize(per)
    print("profile under the trained prior, %d reads:" % len(reads), tot)
    assert tot["set_differs"] == 0 and tot["swaps_unexplained"] == 0 and tot["best_unexplained"] == 0, tot
    B.close(); Db.close()
