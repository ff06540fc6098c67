"""hmmufotu-amd-train-hmm: MSA + Dirichlet priors -> a profile HMM file (src/hmmufotu-train-hmm.cpp:87-228).

Every check is a Python restatement written here from the reference: the match columns and the counting loops of BandedHMMP7::build
(src/BandedHMMP7.cpp:386-541, determineMatchingState of src/BandedHMMP7.h:713-716), the priors' meanPostP
(src/math/DirichletMixture.cpp:45-61, src/math/DirichletDensity.cpp:25-27) with math.lgamma, the bisection of
src/math/RootFinder.cpp:22-76 and the relative entropy of src/math/LinearAlgebraBasic.h:90-98.  Where the order of a sum matters the
restatement adds serially (np.cumsum, or a Python loop), once in the engine's association (every column first, then the columns in
ascending j) and once in the reference's (element by element, j outer, i inner).

CPU part: the program's refusals, the prior reader on the fixture and on damaged copies, the match columns of hand-made counts,
hu_hmm_estimate on hand-made counts and on the counts the restatement makes from 70_otus, the writer through the engine's reader and
the oracle's profile, the reader and the writer under AddressSanitizer + UBSan.
GPU part: hu_hmm_counts against the restatement at every shape where a kernel changes path, the program on 70_otus, and the chain
train-hmm + build --no-hmm -> sim -> hmmufotu-amd against the oracle's pipeline on the same two files.

One refusal of the issue's list cannot be shown without a device: "no column reaches symfrac" needs the weighted counts, which
hu_msa_stats computes on the device.  The CPU part checks it at the library (hu_hmm_match_columns), the GPU part at the program.

Recorded on 70_otus (125 rows x 1486 pruned columns, symfrac 0.5): K = 1285, effN = 15.0783 after 38 bisection passes.  The largest
relative difference between hu_hmm_estimate and the restatement, over all CPU cases: 2.8e-13 on a probability (math.lgamma is CPython's
own implementation), 0 on effN.  hu_hmm_counts against the restatement in the reference's element order: 2.5e-15 on E_I and T(I, .),
1.1e-13 on COMPO; bit-equal everywhere to the restatement summed column first."""
import functools
import gzip
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from hmmufotu_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINDIR = os.path.join(ROOT, "hmmufotu_amd", "bin")
BIN, BUILD, SIM, CLI = (os.path.join(BINDIR, x) for x in ("hmmufotu-amd-train-hmm", "hmmufotu-amd-build", "hmmufotu-amd-sim", "hmmufotu-amd"))
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70, TREE70, DM = os.path.join(REF, "70_otus.fasta.gz"), os.path.join(REF, "70_otus.tree"), os.path.join(REF, "gg_97_otus.dm")
SM_JC69 = os.path.join(REF, "gg_97_otus_JC69.sm")
M, I, D, P = 0, 1, 2, 7                                      # p7_state, src/BandedHMMP7.h:157
REL_HOST = 1e-9                                              # host double arithmetic on the same libm, DESIGN.md section 3
REL_TEXT = 5e-6                                              # 6 printed digits
REL_ORDER = 1e-12                                            # another association of a few thousand positive terms


# ----------------------------------------------------------------------------- the restatement
def py_encode_table():
    """encode(toupper(c)) of IUPACNucl (src/IUPACNucl.cpp:34-50, src/DegenAlphabet.cpp:51-63): a degenerate letter is the first base of
    its expansion, '-' '.' '_' are gaps (-2), every other byte is invalid (-1)"""
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


def sum4(x):
    return (x[0] + x[2]) + (x[1] + x[3])


def as_rows(rows):
    if isinstance(rows, np.ndarray):
        return np.ascontiguousarray(rows, np.uint8)
    return np.frombuffer(b"".join(r.encode("latin1") if isinstance(r, str) else bytes(r) for r in rows), np.uint8).reshape(len(rows), -1)


def py_msa_weights(rows):
    """MSA::updateSeqWeight / updateWeightedCounts (src/MSA.cpp:256-293) in numpy: weights, weighted residue and gap counts"""
    code = ENC[as_rows(rows)].astype(int)
    n, L = code.shape
    cnt = np.stack([(code == b).sum(0) for b in range(4)]).astype(float)               # [4][L]
    nz = (cnt > 0).sum(0)
    with np.errstate(divide="ignore"):
        inv = np.where(cnt > 0, 1.0 / (nz[None, :] * cnt), 0.0)
    res = code >= 0
    w = np.array([ssum(inv[code[i][res[i]], np.nonzero(res[i])[0]]) for i in range(n)])
    ln = res.sum(1)
    w = np.where(ln > 0, w / np.maximum(ln, 1), w)
    w = w * (n / ssum(w))
    wres = np.stack([np.cumsum(np.where(code == b, w[:, None], 0.0), 0)[-1] for b in range(4)])
    wgap = np.cumsum(np.where(code == -2, w[:, None], 0.0), 0)[-1]
    return w, wres, wgap


def py_match_columns(wres, wgap, n_seq, symfrac):
    """src/BandedHMMP7.cpp:405-411 and :517-530 with MSA::symWFrac, CSBaseAt, wIdentityAt (src/MSA.cpp:52-85)"""
    wres, wgap = np.asarray(wres, float), np.asarray(wgap, float)
    num = (wres[0] + wres[2]) + (wres[1] + wres[3])
    with np.errstate(divide="ignore", invalid="ignore"):
        mask = num / (num + wgap) >= symfrac
    mx = np.argmax(wres[:, mask], 0)                                                    # the first maximum
    ident = wres[:, mask][mx, np.arange(int(mask.sum()))] / n_seq
    cons = "".join("ACGT"[b].lower() if x < 0.9 else "ACGT"[b] for b, x in zip(mx, ident))
    return dict(mask=mask, K=int(mask.sum()), map=(np.nonzero(mask)[0] + 1).astype(np.int32), cons=cons, identity=ident)


def py_states(rows, mask):
    """determineMatchingState of every cell, and for every cell the state of the next non-P cell of its row (P: none)"""
    code = ENC[as_rows(rows)]
    res = code >= 0
    m = np.asarray(mask, bool)[None, :]
    own = np.where(m, np.where(res, M, D), np.where(res, I, P)).astype(np.int8)
    nxt = np.full(own.shape, P, np.int8)
    for i in range(len(own)):
        at = np.nonzero(own[i] != P)[0]
        nxt[i, at[:-1]] = own[i, at[1:]]
    return code, own, nxt


def py_counts(rows, w, mask, order):
    """the counts of src/BandedHMMP7.cpp:424-477 (smN taken as the state at jN; a row without a residue adds nothing).
    order "element": every entry is added to in the reference's order, j outer, i inner.  order "column": every column is summed over i
    first and the columns of an entry are then added in ascending j, which is what the engine does."""
    code, own, nxt = py_states(rows, mask)
    n, L = code.shape
    mask = np.asarray(mask, bool)
    cs2p = np.cumsum(mask); K = int(cs2p[-1])
    has = (code >= 0).any(1)
    w = np.where(has, np.asarray(w, float), 0.0)
    W = np.broadcast_to(w[:, None], code.shape)
    ok = (nxt != P) & ~((own == I) & (nxt == D)) & ~((own == D) & (nxt == I))

    def total(sel, cols):
        if order == "element":
            return ssum(W[:, cols].T[sel[:, cols].T])                                  # the transposed view is walked column by column
        s = 0.0
        for j in cols:
            s += ssum(w[sel[:, j]])
        return s

    sel_m = [(own == M) & (code == b) for b in range(4)]
    sel_i = [(own == I) & (code == b) for b in range(4)]
    sel_t = {(a, b): (own == a) & (nxt == b) & ok for a in (M, I, D) for b in (M, I, D)}
    match_cols = np.nonzero(mask)[0]
    ins_cols = [np.nonzero(~mask & (cs2p == k))[0] for k in range(K + 1)]
    em, ei, t = np.zeros((K + 1, 4)), np.zeros((K + 1, 4)), np.zeros((K + 1, 3, 3))
    for k in range(K + 1):
        if k > 0:
            mc = match_cols[k - 1:k]
            for b in range(4):
                em[k, b] = total(sel_m[b], mc)
            for a, b in ((M, M), (M, I), (M, D), (D, M), (D, D)):
                t[k, a, b] = total(sel_t[a, b], mc)
        for b in range(4):
            ei[k, b] = total(sel_i[b], ins_cols[k])
        for b in (M, I):
            t[k, I, b] = total(sel_t[I, b], ins_cols[k])
    for b in range(4):
        em[0, b] = total(sel_m[b], match_cols)
    start, end = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for i in range(n):                                                                 # :466-477
        if has[i]:
            at = np.nonzero(code[i] >= 0)[0]
            start[i], end[i] = at[0], at[-1]
            t[0, M, own[i, at[0]]] += w[i]
            t[K, own[i, at[-1]], M] += w[i]
    return dict(e_m=em, e_i=ei, t=t, K=K, start=start, end=end)


def read_prior(path):
    """the numbers of a .dm file by their labels"""
    lines = open(path).read().split("\n")
    nums = lambda s: [float(x) for x in s.split()]
    out = {}
    for key, head in (("me", "Match emission:"), ("ie", "Insert emission:"), ("mt", "Match transition:"), ("it", "Insert transition:"), ("dt", "Delete transition:")):
        at = lines.index(head)
        if key == "me":
            k, l = int(lines[at + 3].split()[1]), int(lines[at + 3].split()[3])
            out["me_q"] = np.array(nums(lines[at + 5]))
            out["me_alpha"] = np.array([nums(lines[at + 7 + i]) for i in range(k)])
            assert out["me_alpha"].shape == (k, l) and len(out["me_q"]) == l
        else:
            out[key + "_alpha"] = np.array(nums(lines[at + 5]))
    return out


def py_density_post(alpha, f):
    n = len(alpha)
    s = (lambda x: sum4(x)) if n == 4 else (lambda x: (x[0] + x[1]) + x[2]) if n == 3 else (lambda x: x[0] + x[1])
    return [(f[i] + alpha[i]) / (s(f) + s(alpha)) for i in range(n)]


class PyEstimator:
    def __init__(self, counts, n_seq, prior):
        self.em, self.ei, self.t = (np.asarray(counts[k], float).tolist() for k in ("e_m", "e_i", "t"))
        self.K, self.n_seq = len(self.em) - 1, n_seq
        self.q = prior["me_q"].tolist(); self.al = prior["me_alpha"].tolist(); self.pr = {k: v.tolist() for k, v in prior.items()}
        self.L = len(self.q)
        self.asum = [sum4([self.al[i][j] for i in range(4)]) for j in range(self.L)]
        self.lb0 = [sum(math.lgamma(self.al[i][j]) for i in range(4)) - math.lgamma(self.asum[j]) for j in range(self.L)]

    def mix_post(self, d):
        """DirichletMixture::meanPostP"""
        ds = sum4(d)
        logb = []
        for j in range(self.L):
            x = [self.al[i][j] + d[i] for i in range(4)]
            s = 0.0
            for v in x:
                s += math.lgamma(v)
            logb.append((s - math.lgamma(sum4(x))) - self.lb0[j])
        mx = max(logb)
        X = [0.0] * 4
        for j in range(self.L):
            wj = self.q[j] * math.exp(logb[j] - mx)
            for i in range(4):
                X[i] += wj * (self.al[i][j] + d[i]) / (self.asum[j] + ds)
        xs = sum4(X)
        return [v / xs for v in X]

    def entropy(self, x):
        """RelativeEntropyTargetFunc (src/BandedHMMP7.cpp:1122-1135) + 1: of estimateParams only the match emissions enter it"""
        r = x / self.n_seq
        ent = 0.0
        for k in range(1, self.K + 1):
            p = self.mix_post([c * r for c in self.em[k]])
            e = 0.0
            for v in p:
                if v > 0:
                    e += v * math.log(v / 0.25)
            ent += (1.0 / math.log(2)) * e
        return ent / self.K

    def run(self):
        f = lambda x: self.entropy(x) - 1.0
        xl, xr, x, passes = 0.0, float(self.n_seq), float("nan"), 0
        fxl, fxr = f(xl), f(xr)
        if not fxl * fxr >= 0:
            while True:                                                                # rootBisection; f(xl), f(xr) are not evaluated again
                passes += 1
                x = (xl + xr) / 2
                fx = f(x)
                if fx == 0:
                    break
                xmag = 0 if (xl < 0 and xr > 0) else x
                if xr - xl < 1e-10 + 1e-10 * xmag:
                    break
                if (fx > 0) if fxl > 0 else (fx < 0):
                    xl, fxl = x, fx
                else:
                    xr = x
        eff = self.n_seq if math.isnan(x) else x
        r = eff / self.n_seq
        K = self.K
        pm, pi, pt = np.zeros((K + 1, 4)), np.zeros((K + 1, 4)), np.zeros((K + 1, 3, 3))
        for k in range(K + 1):
            T = [[c * r for c in row] for row in self.t[k]]
            pm[k] = self.mix_post([c * r for c in self.em[k]])
            pi[k] = py_density_post(self.pr["ie_alpha"], [c * r for c in self.ei[k]])
            pt[k] = T
            pt[k, M] = py_density_post(self.pr["mt_alpha"], T[M])
            pt[k, I, :2] = py_density_post(self.pr["it_alpha"], T[I][:2])
            pt[k, D, M], pt[k, D, D] = py_density_post(self.pr["dt_alpha"], [T[D][M], T[D][D]])
        pt[0, D, M], pt[0, D, D] = 1, 0
        pt[K, M, D], pt[K, D, M], pt[K, D, D] = 0, 1, 0
        return dict(p_m=pm, p_i=pi, p_t=pt, eff_n=float(eff), passes=passes, f0=fxl, f1=fxr)


def rel_diff(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape
    both_inf = np.isinf(got) & np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(both_inf | (got == want), 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(d)) if d.size else 0.0


def check_estimate(got, want, what):
    d = {k: rel_diff(got[k], want[k]) for k in ("p_m", "p_i", "p_t", "eff_n")}
    print("%s: K = %d, effN = %.17g after %d passes; largest relative difference %s" % (what, len(want["p_m"]) - 1, want["eff_n"], want["passes"], d))
    assert max(d.values()) <= REL_HOST, d
    assert got["passes"] == want["passes"]
    K = len(want["p_m"]) - 1
    t = got["p_t"]
    assert t[0, D, M] == 1 and t[0, D, D] == 0 and t[K, M, D] == 0 and t[K, D, M] == 1 and t[K, D, D] == 0
    assert (t[:, I, D] == 0).all() and (t[:, D, I] == 0).all()
    assert abs(t[K, M].sum() - 1) > 1e-6 or K == 0                                     # T[K].row(M) is not renormalised after M->D is cleared
    return d


# ----------------------------------------------------------------------------- the text of a profile
def costs(p):
    with np.errstate(divide="ignore"):
        return -np.log(np.asarray(p, float))


def parse_hmm_text(text):
    """tags in file order, and per k the match line's extra fields and the numbers as written"""
    lines = text.split("\n")
    at = next(i for i, l in enumerate(lines) if l.startswith("HMM\t"))
    tags = [(l.split(None, 1)[0], l.split(None, 1)[1] if len(l.split(None, 1)) > 1 else "") for l in lines[:at]]
    body = lines[at + 2:]
    assert body[-2:] == ["//", ""]
    body = body[:-2]
    assert len(body) % 3 == 0
    out = dict(tags=tags, match=[], insert=[], trans=[])
    for k in range(len(body) // 3):
        out["match"].append(body[3 * k].split("\t")); out["insert"].append(body[3 * k + 1].split("\t")); out["trans"].append(body[3 * k + 2].split("\t"))
    return out


def check_profile_file(path, want, mc, n_seq, cs_len):
    """a written profile against probabilities `want` and match columns `mc`: both readers, the tags, the MAP column, the CONS letters"""
    text = open(path).read()
    f = parse_hmm_text(text)
    K = mc["K"]
    names = [t[0] for t in f["tags"]]
    assert names == ["HMMER3/f", "NAME", "LENG", "ALPH", "MAXL", "RF", "MM", "CONS", "CS", "MAP", "NSEQ", "EFFN", "DATE"], names
    tag = dict(f["tags"])
    assert (tag["LENG"], tag["ALPH"], tag["MAXL"], tag["RF"], tag["MM"], tag["CONS"], tag["CS"], tag["MAP"], tag["NSEQ"]) == \
        (str(K), "DNA", str(cs_len), "no", "no", "yes", "no", "yes", str(n_seq))
    assert abs(float(tag["EFFN"]) - want["eff_n"]) <= REL_TEXT * want["eff_n"]
    assert len(f["match"]) == K + 1 and f["match"][0][:2] == ["", "COMPO"] and len(f["match"][0]) == 6
    for k in range(1, K + 1):
        m = f["match"][k]
        assert m[0] == "" and m[1] == str(k) and m[6:] == [str(mc["map"][k - 1]), mc["cons"][k - 1], "-", "-", "-"], (k, m)
    assert all(x[:2] == ["", ""] and len(x) == 6 for x in f["insert"]) and all(x[:2] == ["", ""] and len(x) == 9 for x in f["trans"])
    assert f["trans"][0][7:] == ["-0", "*"] and f["trans"][K][4] == "*" and f["trans"][K][7:] == ["-0", "*"]      # the specials: cost of 1, cost of 0
    out = E.parse_files(str(path), None)                                               # the engine's reader
    assert out["K"] == K and out["L"] == cs_len and np.array_equal(out["p2cs"][1:], mc["map"])
    t7 = want["p_t"].reshape(K + 1, 9)[:, [0, 1, 2, 3, 4, 6, 8]]
    d = [rel_diff(out["EM"], costs(want["p_m"])), rel_diff(out["EI"], costs(want["p_i"])), rel_diff(out["T"], costs(t7))]
    print("file against the probabilities, largest relative difference of a cost (match, insert, transition):", d)
    assert max(d) <= REL_TEXT, d
    from oracle import oracle_py as O                                                  # the oracle's profile from what was read: same entry / exit costs
    H = O.Hmm(K, cs_len, out["EM"], out["EI"], out["T"], out["p2cs"], 0)
    entry, exit_, _ = H.params()
    assert np.array_equal(out["entry_cost"], entry) and np.array_equal(out["exit_cost"], exit_)
    return out


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


@functools.lru_cache(None)
def otus70(symfrac=0.5):
    """the restatement on the pruned 70_otus alignment: rows, weights, match columns, counts (both orders), estimate"""
    rows = as_rows(read_fasta(FASTA70)[1])
    rows = np.ascontiguousarray(rows[:, (ENC[rows] >= 0).any(0)])
    w, wres, wgap = py_msa_weights(rows)
    mc = py_match_columns(wres, wgap, len(rows), symfrac)
    col = py_counts(rows, w, mc["mask"], "column")
    est = PyEstimator(col, len(rows), read_prior(DM)).run()
    return types.SimpleNamespace(rows=rows, w=w, wres=wres, wgap=wgap, mc=mc, col=col, est=est)


def run(args, cwd, binary=BIN):
    return subprocess.run([binary] + [str(a) for a in args], cwd=str(cwd), capture_output=True, text=True, timeout=300)


def need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ============================================================================= CPU
def test_program_is_built():
    assert os.path.exists(BIN), "hmmufotu-amd-train-hmm missing: run __graft_entry__.build()"
    assert np.array_equal(ENC, E.msa_encode_table())


DAMAGE = {                                                                              # name -> (from, to, words of the refusal)
    "truncated block": ("alpha:\n0.9067752788895972  7.258155079351504\n", "alpha:\n0.9067752788895972\n", ("Delete transition:", "the file ends after 1 of 2 numbers")),
    "wrong K": ("Insert transition:\nDirichlet Density Model\nTraining cost: 65.7982\nK: 2\n", "Insert transition:\nDirichlet Density Model\nTraining cost: 65.7982\nK: 3\n",
                ("Insert transition:", "K is 3, 2 expected")),
    "mixture over three residues": ("K: 4 L: 5", "K: 3 L: 5", ("Match emission:", "K is 3, 4 expected")),
    "missing label": ("Mixture coefficients:\n", "", ("Match emission:", "'Mixture coefficients:' is missing")),
    "missing block": ("Match transition:\n", "Match transitions\n", ("Match transition:", "is missing")),
    "non-number": ("0.5215297663524403", "0.52152976x3524403", ("Insert emission:", "'0.52152976x3524403' is not a finite number")),
    "too many components": ("L: 5", "L: 500", ("Match emission:", "L is 500")),
    "a row too long": ("38.24555835803766\n", "38.24555835803766 1.5\n", ("Match emission:", "more than 20 numbers")),
}


def damaged(tmp_path, name):
    a, b, words = DAMAGE[name]
    text = open(DM).read()
    assert text.count(a) == 1
    p = tmp_path / (name.replace(" ", "_") + ".dm")
    p.write_text(text.replace(a, b))
    return p, words


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

    refused([fa, "-dm", DM, "--fmt", "msa"], "'msa'", "not read here")
    msa = tmp_path / "hand.msa"; msa.write_bytes(b"HmmUFOtu")
    refused([msa, "-dm", DM], "'msa'", "not read here")                                # the format guessed from the name
    refused([fa, "-dm", DM, "--fmt", "fastq"], "Unsupported sequence format 'fastq'")
    for bad in ("0", "1", "-0.25", "1.5", "nan"):
        refused([fa, "-dm", DM, "-f", bad], "symfrac must between 0 and 1")
    refused([fa, "-dm", DM, "--symfrac", "1"], "symfrac must between 0 and 1")
    refused([fa], "-dm FILE is required")
    refused([fa, "-dm", tmp_path / "none.dm"], "Failed to read in the HMM Prior file", "unable to open")
    for name in DAMAGE:
        p, words = damaged(tmp_path, name)
        refused([fa, "-dm", p, "-o", "out.hmm"], "Failed to read in the HMM Prior file", *words)
    wide = tmp_path / "wide.fasta"                                                     # 65,536 columns stay after pruning, one more than the index arrays hold
    write_fasta(wide, ["a", "b"], ["ACGT" * 16384 + "--", "-" * 65535 + "A" + "--"])
    refused([wide, "-dm", DM], "65536 columns after pruning", "65535")
    refused([tmp_path / "missing.fasta", "-dm", DM], "Unable to open seq file")
    assert not os.path.exists(tmp_path / "out.hmm")


def test_prior_reader():
    got = E.hmm_prior_read(DM)
    want = read_prior(DM)
    assert got.me_L == 5 and want["me_alpha"].shape == (4, 5)
    g = got.as_dict()
    for k in want:
        assert np.array_equal(g[k], want[k]), k                                         # the file's numbers, exactly
    assert want["me_alpha"][1, 0] == 53.61311379271075 and want["dt_alpha"][1] == 7.258155079351504 and want["mt_alpha"][1] == 0.03116046642943362


@pytest.mark.parametrize("name", sorted(DAMAGE))
def test_prior_reader_refuses(tmp_path, name):
    p, words = damaged(tmp_path, name)
    with pytest.raises(E.EngineError) as e:
        E.hmm_prior_read(p)
    assert all(w in str(e.value) for w in words), str(e.value)


def test_match_columns():
    n_seq = 4
    #          at symfrac  just below   all gaps   no weight  tie A/G     identity 0.9  below 0.9   first of C=T
    wres = np.array([[1.0, 1.0,         0.0,       0.0,       1.5,        0.2,          0.2,        0.0],
                     [0.5, 0.5,         0.0,       0.0,       0.5,        3.6,          3.5,        1.25],
                     [0.25, 0.25,       0.0,       0.0,       1.5,        0.1,          0.2,        0.5],
                     [0.25, 0.25,       0.0,       0.0,       0.5,        0.1,          0.1,        1.25]])
    wgap = np.array([2.0, 2.000000001,             4.0,     0.0,       0.0,        0.0,          0.0,        1.0])
    got = E.hmm_match_columns(wres, wgap, n_seq, 0.5)
    want = py_match_columns(wres, wgap, n_seq, 0.5)
    assert list(got["mask"]) == [True, False, False, False, True, True, True, True] == list(want["mask"])
    assert got["K"] == 5 and list(got["map"]) == [1, 5, 6, 7, 8] == list(want["map"])
    assert got["cons"] == "aaCcc" == want["cons"] and np.array_equal(got["identity"], want["identity"])
    assert got["identity"][2] == 0.9 and got["identity"][3] < 0.9
    for bad in (0.0, 1.0, -1.0, 2.0, float("nan")):
        with pytest.raises(E.EngineError, match="symfrac must between 0 and 1"):
            E.hmm_match_columns(wres, wgap, n_seq, bad)
    with pytest.raises(E.EngineError, match="no column of 3 reaches"):                  # K = 0
        E.hmm_match_columns(wres[:, 1:4], wgap[1:4], n_seq, 0.5)
    big = np.ones((4, 65536))
    with pytest.raises(E.EngineError, match="65536 columns"):
        E.hmm_match_columns(big, np.zeros(65536), n_seq, 0.5)
    assert E.hmm_match_columns(big[:, :65535], np.zeros(65535), n_seq, 0.5)["K"] == 65535


def hand_counts(rng, K, n_seq, strength=0.9):
    """counts of n_seq sequences: at every position `strength` of them on one base, a little on the others"""
    em = rng.random((K + 1, 4)) * 0.03 * n_seq
    em[np.arange(1, K + 1), rng.integers(0, 4, K)] += strength * n_seq
    em[0] = em[1:].sum(0)
    ei = rng.random((K + 1, 4)) * 0.1 * n_seq
    t = rng.random((K + 1, 3, 3)) * n_seq
    t[:, I, D] = 0; t[:, D, I] = 0
    if K > 1:
        em[2] = 0; ei[2] = 0; t[2] = 0                                                  # a position nothing was counted at
    return dict(e_m=em, e_i=ei, t=t)


@pytest.mark.parametrize("K,n_seq", [(1, 5), (3, 40), (17, 1000)])
def test_estimate_on_hand_counts(K, n_seq):
    c = hand_counts(np.random.default_rng(K), K, n_seq)
    pr = E.hmm_prior_read(DM)
    got = E.hmm_estimate(c["e_m"], c["e_i"], c["t"], n_seq, pr)
    want = PyEstimator(c, n_seq, read_prior(DM)).run()
    assert want["f0"] < 0 < want["f1"] and 30 <= want["passes"] <= 50 and 0 < want["eff_n"] < n_seq
    check_estimate(got, want, "hand-made counts")
    assert np.allclose(got["p_m"].sum(1), 1, rtol=0, atol=1e-14) and np.allclose(got["p_i"].sum(1), 1, rtol=0, atol=1e-14)
    with pytest.raises(E.EngineError):
        E.hmm_estimate(-c["e_m"], c["e_i"], c["t"], n_seq, pr)


def test_estimate_without_a_sign_change():
    """counts too weak to reach one bit of relative entropy: the root finder returns NaN and effN stays n_seq"""
    c = hand_counts(np.random.default_rng(5), 4, 3, strength=0.02)
    got = E.hmm_estimate(c["e_m"], c["e_i"], c["t"], 3, E.hmm_prior_read(DM))
    want = PyEstimator(c, 3, read_prior(DM)).run()
    assert want["f0"] < 0 and want["f1"] < 0 and want["passes"] == 0 and want["eff_n"] == 3.0
    assert got["eff_n"] == 3.0 and got["passes"] == 0
    check_estimate(got, want, "no sign change")


def test_estimate_on_70otus():
    o = otus70()
    assert o.rows.shape == (125, 1486)
    got = E.hmm_estimate(o.col["e_m"], o.col["e_i"], o.col["t"], 125, E.hmm_prior_read(DM))
    check_estimate(got, o.est, "70_otus")
    assert o.est["passes"] > 30 and 1 < o.est["eff_n"] < 125


def test_writer_round_trip(tmp_path):
    o = otus70()
    p = tmp_path / "w.hmm"
    E.hmm_write(p, o.est["p_m"], o.est["p_i"], o.est["p_t"], o.mc["map"], o.mc["cons"], 1486, 125, o.est["eff_n"], name="some/path.fasta.gz",
                version="test-v0", date="Sun Oct 18 12:00:00 2026")
    text = p.read_text()
    assert text.startswith("HMMER3/f\ttest-v0\nNAME\tsome/path.fasta.gz\nLENG\t%d\nALPH\tDNA\nMAXL  1486\n" % o.mc["K"])
    assert "\nDATE  Sun Oct 18 12:00:00 2026\nHMM\t\tA\tC\tG\tT\n\t\tm->m\tm->i\tm->d\ti->m\ti->i\td->m\td->d\n\tCOMPO\t" in text
    check_profile_file(p, o.est, o.mc, 125, 1486)
    assert any(c.islower() for c in o.mc["cons"]) and any(c.isupper() for c in o.mc["cons"])
    # by hand: a zero probability is "*" on the insert and transition lines; six digits
    pm = np.array([[0.25, 0.25, 0.25, 0.25], [0.7, 0.1, 0.1, 0.1]]); pi = np.array([[0.25] * 4, [1.0, 0.0, 0.0, 0.0]])
    pt = np.zeros((2, 3, 3)); pt[0, M] = [0.9, 0.05, 0.05]; pt[0, I, :2] = [0.5, 0.5]; pt[0, D, M] = 1; pt[1, M] = [1 / 3, 2 / 3, 0]; pt[1, I, :2] = [0.123456789, 0.876543211]; pt[1, D, M] = 1
    q = tmp_path / "h.hmm"
    E.hmm_write(q, pm, pi, pt, [3], "g", 5, 2, 1.23456789)
    lines = q.read_text().split("\n")
    assert "EFFN  1.23457" in lines
    assert lines[-5:] == ["\t1\t0.356675\t2.30259\t2.30259\t2.30259\t3\tg\t-\t-\t-", "\t\t-0\t*\t*\t*", "\t\t1.09861\t0.405465\t*\t2.09186\t0.131769\t-0\t*", "//", ""]
    with pytest.raises(E.EngineError, match="unable to write"):
        E.hmm_write(tmp_path / "no" / "dir.hmm", pm, pi, pt, [3], "g", 5, 2, 1.0)


def test_sanitizer_on_the_prior_reader_and_the_writer(tmp_path):
    """hu_hmm_io.cpp and tests/san/dm_driver.cpp under g++ -fsanitize=address,undefined, as tests/test_sanitizer.py builds its driver;
    run stand-alone on the fixture and on damaged copies of it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "dm_driver")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe,
           os.path.join(ROOT, "tests", "san", "dm_driver.cpp"), os.path.join(ROOT, "hmmufotu_amd", "csrc", "hu_hmm_io.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, DM, str(tmp_path / "scratch.dm"), "600"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:] + "\n" + r.stderr[-4000:])
    assert "600 trials" in r.stdout and " 0 refused" not in r.stdout and " 0 accepted" not in r.stdout


# ============================================================================= GPU
LETTERS = list("ACGT") * 6 + list("acgt") * 2 + list("RYKMSWBDHVNUn") + list("---..__") * 2 + list("!*Z0 ")


def random_rows(rng, n, L, gappy=0.0):
    a = rng.choice(np.frombuffer("".join(LETTERS).encode(), np.uint8), (n, L))
    a[rng.random((n, L)) < gappy] = ord("-")
    return np.ascontiguousarray(a)


def check_counts(rows, w, mask, what=""):
    """hmm_counts against the restatement in both orders"""
    rows = as_rows(rows)
    col = py_counts(rows, w, mask, "column")
    ele = py_counts(rows, w, mask, "element")
    got = E.hmm_counts(rows, w, col["start"], col["end"], mask)
    K = col["K"]
    assert got["e_m"].shape == (K + 1, 4) and got["t"].shape == (K + 1, 3, 3)
    for k in ("e_m", "e_i", "t"):
        assert np.array_equal(got[k], col[k]), (what, k)                                # column first, then ascending j: bit for bit
    # what a single match column gives (and the begin / end sums) is the reference's element order bit for bit
    assert np.array_equal(got["e_m"][1:], ele["e_m"][1:]) and np.array_equal(got["t"][:, M], ele["t"][:, M]) and np.array_equal(got["t"][:, D], ele["t"][:, D])
    d = [rel_diff(got["e_i"], ele["e_i"]), rel_diff(got["t"][:, I], ele["t"][:, I]), rel_diff(got["e_m"][0], ele["e_m"][0])]
    print("%s %d x %d, K = %d: E_I, T(I, .), COMPO against the element order: %s" % (what, rows.shape[0], rows.shape[1], K, d))
    assert max(d) <= REL_ORDER, d
    assert (got["t"][:, I, D] == 0).all() and (got["t"][:, D, I] == 0).all() and (got["t"][0, D] == 0).all()
    return got, col


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(1, 1), (2, 63), (7, 64), (8, 65), (9, 256), (513, 257), (513, 1), (1, 257), (9, 65), (8, 64)])
def test_counts_on_random_rows(n, L):
    need_gpu()
    rng = np.random.default_rng(1000 * n + L)
    rows = random_rows(rng, n, L, gappy=0.2)
    rows[0, 0] = ord("A")                                                               # at least one residue
    mask = rng.random(L) < 0.6
    mask[int(rng.integers(L))] = True
    w = rng.random(n) * 2 + 0.01
    got, col = check_counts(rows, w, mask, "random")
    if n >= 7 and L >= 63:
        assert (got["e_i"] > 0).any() and (got["t"][:, M, D] > 0).any() and (got["t"][:, D, D] > 0).any() and (got["t"][:, I, I] > 0).any()


def hand_alignment(rng, n, runs):
    """columns from runs of (kind, length): "m" a match column (few gaps), "i" an insert column (mostly gaps); returns rows, mask"""
    cols, mask = [], []
    for kind, length in runs:
        for _ in range(length):
            c = rng.choice(np.frombuffer(b"ACGTacgtRN", np.uint8), n)
            c[rng.random(n) < (0.15 if kind == "m" else 0.7)] = rng.choice(np.frombuffer(b"-._!", np.uint8))
            cols.append(c); mask.append(kind == "m")
    return np.ascontiguousarray(np.stack(cols, 1)), np.array(mask)


@pytest.mark.gpu
def test_counts_on_hand_made_alignments():
    need_gpu()
    rng = np.random.default_rng(77)
    # inserts before the first match column (k = 0) and after the last (k = K); an insert run of 70 and one of 300 columns, so that the
    # search for the next state crosses a wave's and a workgroup's columns
    rows, mask = hand_alignment(rng, 12, [("i", 5), ("m", 3), ("i", 70), ("m", 2), ("i", 300), ("m", 4), ("i", 9)])
    rows[1, :] = ord("-")                                                               # a row with no residue
    rows[2, :5] = np.frombuffer(b"AC-GT", np.uint8)                                     # begins in an insert column
    rows[2, -9:] = np.frombuffer(b"--a--c--g", np.uint8)                                # ends in one
    rows[3, :5] = ord("-"); rows[3, 5] = ord("G")                                       # begins in the first match column
    rows[3, -9:] = ord("."); rows[3, -10] = ord("t")                                    # ends in the last match column
    rows[4, 8:78] = ord("-"); rows[4, 80:380] = ord("_")                                # both long runs empty: M -> M across 70 and 300 columns
    rows[5, 8:78] = ord("-"); rows[5, 77] = ord("A")                                    # one insert at the far end of the run
    rows[6, 80:380] = ord("-"); rows[6, 80] = ord("c"); rows[6, 78:80] = ord("-")       # D D, then an insert: D -> I is not counted
    rows[4, [7, 78, 79, 380]] = np.frombuffer(b"ACGT", np.uint8); rows[2, 383] = ord("A")
    w = rng.random(12) + 0.5
    w[1] = 3.0                                                                          # the weight of the empty row must not show
    got, col = check_counts(rows, w, mask, "hand-made")
    K = col["K"]
    assert K == 9 and col["start"][1] == -1 and got["e_i"][0].sum() > 0 and got["e_i"][K].sum() > 0
    assert got["t"][0, M, I] > 0 and got["t"][0, M, M] > 0 and got["t"][K, I, M] > 0 and got["t"][K, M, M] > 0 and got["t"][K, M, I] > 0
    total = w.sum() - w[1]
    assert abs(got["t"][0, M].sum() - total) <= 1e-12 * total and abs(got["t"][K, :, M].sum() - total) <= 1e-12 * total
    assert got["t"][3, M, M] >= w[4] and got["t"][5, M, M] >= w[4]                       # row 4 steps over both runs
    # every column a match column: no insert anywhere
    rows2, mask2 = hand_alignment(rng, 9, [("m", 130)])
    got2, _ = check_counts(rows2, rng.random(9) + 0.1, mask2, "all match")
    assert (got2["e_i"] == 0).all() and (got2["t"][:, I] == 0).all() and (got2["t"][:, M, I] == 0).all()
    # refusals of the arguments, before the device
    with pytest.raises(E.EngineError, match="start"):
        E.hmm_counts(rows, w, np.where(col["start"] >= 0, 0, -1), col["end"], mask)     # column 0 of most rows is a gap
    with pytest.raises(E.EngineError, match="weight"):
        E.hmm_counts(rows, -w, col["start"], col["end"], mask)


@pytest.mark.gpu
def test_counts_on_70otus():
    need_gpu()
    o = otus70()
    st = E.msa_stats(o.rows)
    assert rel_diff(st["seq_weight"], o.w) <= 1e-12 and rel_diff(st["res_wcount"], o.wres) <= 1e-12      # the restated weights are the engine's
    mc = E.hmm_match_columns(st["res_wcount"], st["gap_wcount"], 125, 0.5)
    assert np.array_equal(mc["mask"], o.mc["mask"]) and mc["cons"] == o.mc["cons"] and np.array_equal(mc["map"], o.mc["map"])
    got, col = check_counts(o.rows, st["seq_weight"], mc["mask"], "70_otus")
    assert np.array_equal(col["start"], st["start"]) and np.array_equal(col["end"], st["end"])


def program_profile(tmp_path, name="p.hmm"):
    r = run([FASTA70, "-dm", DM, "-o", name, "-v"], tmp_path)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.gpu
def test_program_on_70otus(tmp_path):
    need_gpu()
    r = program_profile(tmp_path)
    o = otus70()
    for line in ("MSA loaded", "MSA pruned", "MSA database created for 125 X 1486 aligned sequences", "Profile size: %d match columns of 1486" % o.mc["K"],
                 "Banded HMM profile trained", "Banded HMM profile written"):
        assert line in r.stderr.split("\n"), (line, r.stderr)
    assert r.stdout == ""
    out = check_profile_file(tmp_path / "p.hmm", o.est, o.mc, 125, 1486)                 # LENG, NSEQ, MAP, CONS equal; the numbers at 5e-6
    text = (tmp_path / "p.hmm").read_text()
    assert text.startswith("HMMER3/f\thmmufotu-amd-train-hmm-v1.5.1\nNAME\t%s\nLENG\t%d\n" % (FASTA70, o.mc["K"]))
    quiet = run([FASTA70, "-dm", DM], tmp_path)                                         # stdout without -o, nothing on stderr without -v
    strip = lambda s: "\n".join(l for l in s.split("\n") if not l.startswith("DATE  "))
    assert quiet.returncode == 0 and quiet.stderr == "" and strip(quiet.stdout) == strip(text)
    # another threshold gives another profile; one that no column reaches is refused (every column of these three rows has a gap)
    r9 = run([FASTA70, "-dm", DM, "-f", "0.9"], tmp_path)
    assert r9.returncode == 0 and "LENG\t%d\n" % otus70(0.9).mc["K"] in r9.stdout and otus70(0.9).mc["K"] < o.mc["K"]
    write_fasta(tmp_path / "gappy.fasta", ["a", "b", "c"], ["AC-GT-", "-CGT-A", "A-G-TA"])
    rk = run(["gappy.fasta", "-dm", DM, "-f", "0.99"], tmp_path)
    assert rk.returncode != 0 and rk.stdout == "" and "no column of 6 reaches the symbol fraction 0.99" in rk.stderr and rk.stderr.count("\n") == 1


@pytest.mark.gpu
def test_trained_profile_in_a_database(tmp_path):
    """<DB>.hmm from hmmufotu-amd-train-hmm beside <DB>.ptu from hmmufotu-amd-build --no-hmm: the database loads, hmmufotu-amd-sim draws
    reads from it, hmmufotu-amd assigns them, and the engine agrees with the oracle's pipeline on the same two files at the bar of
    tests/test_build_program.py: equal statuses, costs and candidate counts, every difference in the ids a documented tie"""
    need_gpu()
    from oracle import oracle_py as O, parity
    program_profile(tmp_path, "db.hmm")
    b = run([FASTA70, TREE70, "--no-hmm", "-sm", SM_JC69, "-n", "db"], tmp_path, BUILD)
    assert b.returncode == 0, b.stderr
    s = run(["db", "reads.fa", "-N", "200", "-S", "7", "-m", "400", "-s", "30", "--msa", FASTA70], tmp_path, SIM)
    assert s.returncode == 0, s.stderr
    ids, reads = read_fasta(tmp_path / "reads.fa")
    assert len(reads) == 200
    c = run(["db", "reads.fa", "-o", "out.tsv"], tmp_path, CLI)
    assert c.returncode == 0, c.stderr
    body = [x for x in (tmp_path / "out.tsv").read_text().strip().split("\n") if not x.startswith("#") and not x.startswith("id\t")]
    assert [x.split("\t")[0] for x in body] == ids
    f = E.parse_files(str(tmp_path / "db.hmm"), str(tmp_path / "db.ptu"))
    o = otus70()
    assert f["K"] == o.mc["K"] and f["L"] == 1486
    keep = [i for i, r in enumerate(reads) if len(r) >= 60]
    reads = [reads[i] for i in keep]
    assert len(reads) >= 150
    D_ = E.Database.load(str(tmp_path / "db.hmm"), str(tmp_path / "db.ptu"))
    hmm = types.SimpleNamespace(K=f["K"], L=f["L"], EM=f["EM"], EI=f["EI"], T=f["T"], p2cs=f["p2cs"])
    ix = E.SeedIndex(f["parent"], f["seq"], hmm)
    vps = ix.lookup(reads)
    B = E.Batch(D_, len(reads)); B.set_reads(reads, vps); B.assign(E.default_opts())
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
    print("trained 70_otus profile, %d reads:" % len(reads), tot)
    assert tot["set_differs"] == 0 and tot["swaps_unexplained"] == 0 and tot["best_unexplained"] == 0, tot
    B.close(); D_.close()
