"""hmmufotu-amd-tree: the pair counts and the distances of an alignment's rows, neighbour joining on the host and on the
device, and the program.

The yardstick is a restatement in this file that shares no code with the library: the pair counts from comparisons of the codes, the
distance formulas in float64 with libm's log, and neighbour joining in exact arithmetic.  The exact NJ holds every distance as an
integer over a common power of two (fractions.Fraction only where a join divides by r - 2), with the rules of DESIGN.md §21: the
least (Q, i, j) over the slots, the new node in slot i, the last slot moved into slot j.

Bounds.  On additive matrices with lengths in multiples of 2^-10 and on integer matrices Q, R and d_uk stay exact in float64, so the
join order must be identical.  A length is l_i = d_ij / 2 + (R_i - R_j) / (2 (r - 2)), two roundings, and l_j = d_ij - l_i, one more:
within 2^-52 (|d_ij| + |R_i - R_j| / (2 (r - 2))) of the exact value; on the additive matrices every length is exact.

The distance bar: the largest relative deviation of the library from the float64 restatement with libm's log, measured over the
cases of this file (70_otus and the synthetic rows, all six types), is 0 on the host path, whose log is libm's too, and 3.66e-16 on
the device (n 65, 1000 columns; 3.6e-16 on 70_otus); four times it, 1.46e-15, rounded up to a power of two is 2^-49 = 1.78e-15.  The
cap is 1e-12: beyond it a formula is wrong."""
import gzip
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
REF = os.path.join(ROOT, "tests", "golden", "ref_data")
FASTA70 = os.path.join(REF, "70_otus.fasta.gz")
DIST_BAR = 2.0 ** -49
assert DIST_BAR <= 1e-12
TYPES = ("pdist", "JC69", "K80", "F81", "HKY85", "TN93")
PI = np.array([0.21, 0.24, 0.31, 0.24])


def _bin(name="hmmufotu-amd-tree"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


def sm(name):
    return os.path.join(REF, "gg_97_otus_%s.sm" % name)


# ---- the restatement: counts and distances ----

def ref_counts(rows):
    """[n][n][4] N, P_R, P_Y, Q from comparisons of the codes: A C G T = 0 1 2 3, purines A G, pyrimidines C T"""
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    out = np.zeros((n, n, 4), np.int64)
    pur = (rows == 0) | (rows == 2)
    for i in range(n):
        for j in range(i, n):
            a, b = rows[i], rows[j]
            both = (a >= 0) & (b >= 0)
            diff = both & (a != b)
            ti = diff & (pur[i] == pur[j])
            c = (both.sum(), (ti & pur[i]).sum(), (ti & ~pur[i]).sum(), (diff & (pur[i] != pur[j])).sum())
            out[i, j] = c; out[j, i] = c
    return out


def ref_formula(kind, pi, N, PR, PY, Q):
    """the reference's subDist in float64, None for a saturated pair (src/JC69.h:103, K80.h:120, F81.h:120, HKY85.h:155, TN93.h:156)"""
    if N == 0:
        return 0.0
    a, c, g, t = (float(x) for x in pi)
    lg = lambda x: math.log(x) if x > 0 else None
    terms = None
    if kind == "pdist":
        return (PR + PY + Q) / N
    if kind == "JC69":
        terms = [(-3.0 / 4.0, lg(1.0 - 4.0 / 3.0 * ((PR + PY + Q) / N)))]
    elif kind == "K80":
        p, q = (PR + PY) / N, Q / N
        terms = [(-1.0 / 2, lg(1 - 2 * p - q)), (-1.0 / 4, lg(1 - 2 * q))]
    elif kind == "F81":
        Ee = 1 - (a * a + c * c + g * g + t * t)
        terms = [(-Ee, lg(1 - ((PR + PY + Q) / N) / Ee))]
    elif kind == "HKY85":
        A = a * g / (a + g) + c * t / (c + t); B = a * g + c * t; Cc = (a + g) * (c + t)
        p, q = (PR + PY) / N, Q / N
        terms = [(-2 * A, lg(1 - p / (2 * A) - (A - B) * q / (2 * A * Cc)))]
    elif kind == "TN93":
        r, y = a + g, c + t
        pr, py, q = PR / N, PY / N, Q / N
        terms = [(-2 * a * g / r, lg(1 - r / (2 * a * g) * pr - 1 / (2 * r) * q)),
                 (-2 * g * c / y, lg(1 - y / (2 * t * c) * py - 1 / (2 * y) * q)),            # g c as src/TN93.h:170 has it
                 (-2 * (r * y - a * g * y / r - t * c * r / y), lg(1 - 1 / (2 * r * y) * q))]
    if any(l is None for _, l in terms):
        return None
    d = 0.0
    for k, (w, l) in enumerate(terms):
        d = w * l if k == 0 else d + w * l
    return d + 0.0


def ref_distances(rows, kind, pi=PI, sat=None):
    cnt = ref_counts(rows)
    n = len(cnt)
    D = np.zeros((n, n)); satur = []
    for i in range(n):
        for j in range(i + 1, n):
            d = ref_formula(kind, pi, *(int(x) for x in cnt[i, j]))
            if d is None:
                satur.append((i, j)); d = math.inf
            D[i, j] = D[j, i] = d
    if satur:
        fill = sat if sat is not None else 2 * D[np.isfinite(D)].max()
        D[np.isinf(D)] = fill
    return D, len(satur)


def rel_dev(got, want):
    """the largest |got - want| / |want|; where want is 0, got must be 0"""
    got, want = np.asarray(got), np.asarray(want)
    z = want == 0
    assert np.all(got[z] == 0)
    return float(np.max(np.abs(got[~z] - want[~z]) / np.abs(want[~z]))) if (~z).any() else 0.0


# ---- the restatement: exact neighbour joining ----

def exact_nj(D, shift):
    """D: floats that are integers over 2^k, k <= some bound; held as integers over 2^shift.  Returns joins (node pairs), lengths
    (Fractions), last3, last_len3 (Fractions), and per join (d_ij, R_i - R_j, r) as Fractions for the bound."""
    n = len(D)
    sc = 1 << shift
    M = np.empty((n, n), dtype=object)
    for i in range(n):
        for j in range(n):
            f = Fraction(float(D[i][j])) * sc
            assert f.denominator == 1
            M[i, j] = int(f)
    R = M.sum(axis=1)
    ids = list(range(n))
    joins, lens, info = [], [], []
    r = n
    for t in range(n - 3):
        A = M[:r, :r]
        Qm = (r - 2) * A - R[:r, None] - R[None, :r]
        iu = np.triu_indices(r, 1)                       # row-major: the first least value is the least (i, j)
        vals = Qm[iu]
        k = int(np.nonzero((vals == vals.min()).astype(bool))[0][0])
        i, j = int(iu[0][k]), int(iu[1][k])
        dij = M[i, j]
        li = Fraction(dij, 2) + Fraction(R[i] - R[j], 2 * (r - 2))
        lj = dij - li
        if li < 0:
            li, lj = Fraction(0), Fraction(dij)
        elif lj < 0:
            li, lj = Fraction(dij), Fraction(0)
        joins.append((ids[i], ids[j])); lens.append((li / sc, lj / sc)); info.append((Fraction(dij, sc), Fraction(R[i] - R[j], sc), r))
        ids[i] = n + t
        for k2 in range(r):
            if k2 == i or k2 == j:
                continue
            s2 = M[i, k2] + M[j, k2] - dij
            assert s2 % 2 == 0, "the common power of two is too small"
            duk = s2 // 2
            R[k2] = R[k2] - M[i, k2] - M[j, k2] + duk
            M[i, k2] = duk; M[k2, i] = duk
        last = r - 1
        if j != last:
            for k2 in range(last):
                if k2 == j:
                    M[j, j] = 0
                else:
                    M[j, k2] = M[last, k2]; M[k2, j] = M[last, k2]
            R[j] = R[last]; ids[j] = ids[last]
        r -= 1
        R[i] = sum(M[i, k2] for k2 in range(r))
    dab, dac, dbc = M[0, 1], M[0, 2], M[1, 2]
    l3 = [Fraction(dab + dac - dbc, 2 * sc), Fraction(dab + dbc - dac, 2 * sc), Fraction(dac + dbc - dab, 2 * sc)]
    return joins, lens, ids[:3], l3, info


def random_additive(n, seed):
    """the path lengths between the leaves of a random unrooted binary tree: lengths in multiples of 2^-10, a third of the inner ones 0"""
    rng = np.random.default_rng(seed)
    edges = [[n, 0], [n, 1], [n, 2]]                    # inner nodes n, n + 1, ...
    nxt = n + 1
    for leaf in range(3, n):
        e = int(rng.integers(len(edges)))
        a, b = edges[e]
        edges[e] = [a, nxt]; edges.append([nxt, b]); edges.append([nxt, leaf]); nxt += 1
    w = []
    for a, b in edges:
        inner = a >= n and b >= n
        w.append(0 if inner and rng.integers(3) == 0 else int(rng.integers(1, 2049)))
    return path_matrix(n, nxt, [(a, b, x / 1024.0) for (a, b), x in zip(edges, w)])


def path_matrix(n, n_nodes, edges):
    adj = [[] for _ in range(n_nodes)]
    for a, b, x in edges:
        adj[a].append((b, x)); adj[b].append((a, x))
    D = np.zeros((n, n))
    for s in range(n):
        dist = {s: 0.0}; st = [s]
        while st:
            u = st.pop()
            for v, x in adj[u]:
                if v not in dist:
                    dist[v] = dist[u] + x; st.append(v)
        D[s] = [dist[k] for k in range(n)]
    return D


def tree_edges(n, tr):
    """the edges of a result of nj: the top node is 2 n - 3"""
    top = 2 * n - 3
    e = [(n + t, int(tr["join"][t][s]), float(tr["len"][t][s])) for t in range(n - 3) for s in range(2)]
    return e + [(top, int(tr["last3"][s]), float(tr["last_len3"][s])) for s in range(3)]


def random_integer(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 1001, (n, n)).astype(np.float64)
    a = np.triu(a, 1)
    return a + a.T


def same_tree(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("join", "len", "last3", "last_len3"))


def check_against_exact(D, tr, shift, exact_lengths):
    n = len(D)
    joins, lens, l3, ll3, info = exact_nj(D, shift)
    assert [tuple(int(v) for v in x) for x in tr["join"]] == joins
    assert [int(v) for v in tr["last3"]] == l3
    clamps = 0
    for t in range(n - 3):
        dij, dR, r = info[t]
        bound = 0 if exact_lengths else Fraction(1, 2 ** 52) * (abs(dij) + abs(dR) / (2 * (r - 2)))
        for s in range(2):
            assert abs(Fraction(float(tr["len"][t][s])) - lens[t][s]) <= bound, (t, s, float(tr["len"][t][s]), float(lens[t][s]))
            clamps += lens[t][s] == 0 and lens[t][1 - s] == dij and dij != 0
    for s in range(3):
        assert Fraction(float(tr["last_len3"][s])) == ll3[s]
    return clamps


# ---- the inputs of the counts and the distances ----

def read_fasta(path):
    names, seqs = [], []
    with gzip.open(path, "rt") as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                names.append(line[1:].split()[0]); seqs.append([])
            else:
                seqs[-1].append(line)
    return names, ["".join(s) for s in seqs]


_CACHE = {}


def rows70():
    """the pruned 70_otus alignment in the codes of msa_encode_table, with its names"""
    if "r70" not in _CACHE:
        names, seqs = read_fasta(FASTA70)
        enc = E.msa_encode_table()
        a = enc[np.frombuffer("".join(seqs).encode(), np.uint8).reshape(len(seqs), -1)]
        keep = (a >= 0).any(axis=0)
        _CACHE["r70"] = (names, np.ascontiguousarray(a[:, keep]))
    return _CACHE["r70"]


def synth_rows(n, L, seed):
    """random rows with gaps; row 1 without a symbol, row 2 a copy of row 0, rows 3 and 4 (n >= 5) all A and all C: saturated"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, L)
    rows = np.where(rng.random((n, L)) < 0.15, rng.integers(0, 4, (n, L)), base[None, :]).astype(np.int8)
    rows[rng.random((n, L)) < 0.1] = -2
    rows[rng.random((n, L)) < 0.02] = -1
    if n > 1:
        rows[1] = -2
    if n > 2:
        rows[2] = rows[0]
    if n >= 5:
        rows[3] = 0; rows[4] = 1
    return rows


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- CPU: neighbour joining on the host path ----

def test_three_nodes_by_hand():
    tr = E.nj([[0, 2, 3], [2, 0, 4], [3, 4, 0]], host=True)
    assert tr["join"].shape == (0, 2) and list(tr["last3"]) == [0, 1, 2] and list(tr["last_len3"]) == [0.5, 1.5, 2.5]


def test_the_classic_five_taxa_by_hand():
    """Saitou and Nei's worked example as the textbooks carry it: (a, b) first with 2 and 3; then Q ties between (u, c) in slots (0, 2)
    and (e, d) in slots (1, 3), the smaller i wins: 3 and 4; v, e, d hang on the top with 2, 1, 2"""
    D = [[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]]
    tr = E.nj(D, host=True)
    assert tr["join"].tolist() == [[0, 1], [5, 2]] and tr["len"].tolist() == [[2, 3], [3, 4]]
    assert tr["last3"].tolist() == [6, 4, 3] and tr["last_len3"].tolist() == [2, 1, 2]
    assert check_against_exact(np.array(D, float), tr, 8, True) == 0
    text = E.nj_newick("abcde", tr)
    assert text == "(((a:2,b:3):3,c:4):2,e:1,d:2);\n"


@pytest.mark.parametrize("n", [4, 5, 33, 65, 130])
def test_host_additive_matrices_are_joined_exactly(n):
    for seed in (1, 2):
        D = cached(("add", n, seed), lambda: random_additive(n, 100 * n + seed))
        tr = E.nj(D, host=True)
        check_against_exact(D, tr, 11, True)
        assert np.array_equal(path_matrix(n, 2 * n - 2, tree_edges(n, tr)), D)


@pytest.mark.parametrize("n", [5, 17, 33, 65])
def test_host_integer_matrices(n):
    clamps = 0
    for seed in (1, 2, 3):
        D = cached(("int", n, seed), lambda: random_integer(n, 7 * n + seed))
        clamps += check_against_exact(D, E.nj(D, host=True), n, False)
    assert n < 17 or clamps >= 1                       # a negative side set to 0 does occur in these inputs


def test_what_nj_refuses():
    for bad, why in (([[0, 1], [1, 0]], "needs 3"), ([[0, 1, 2], [1, 0, 3], [2, 4, 0]], "symmetric"), ([[0, 1, 2], [1, 1, 3], [2, 3, 0]], "diagonal"),
                     ([[0, 1, math.inf], [1, 0, 3], [math.inf, 3, 0]], "finite")):
        with pytest.raises(E.EngineError, match=why):
            E.nj(bad, host=True)


# ---- CPU: the counts and the distances on the host path ----

def dist_cases():
    names, r70 = rows70()
    return [("70_otus", r70), ("synth 9 x 150", synth_rows(9, 150, 3)), ("synth 6 x 1", synth_rows(6, 1, 4)), ("synth 12 x 700", synth_rows(12, 700, 5))]


def test_the_code_table_is_the_one_the_planes_assume():
    enc = E.msa_encode_table()
    assert [int(enc[ord(c)]) for c in "ACGTacgt"] == [0, 1, 2, 3, 0, 1, 2, 3] and enc[ord("-")] < 0 and int(enc.max()) == 3


def test_host_pair_counts_are_exact():
    for what, rows in dist_cases():
        want = cached(("cnt", what), lambda: ref_counts(rows))
        assert np.array_equal(E.msa_pair_counts(rows, host=True), want), what
    _, rows = dist_cases()[1]
    c = E.msa_pair_counts(rows, host=True)
    assert not c[1].any() and not c[0, 2, 1:].any() and c[3, 4, 3] == c[3, 4, 0] == rows.shape[1]


def test_host_distances_meet_the_bar():
    worst = 0.0
    for what, rows in dist_cases():
        for kind in TYPES:
            for sat in (None, 2.5):
                want, ns = cached(("dist", what, kind, sat), lambda: ref_distances(rows, kind, PI, sat))
                got, gs = E.msa_distances(rows, kind, PI, sat, host=True)
                assert gs == ns and np.array_equal(got, got.T) and not got.diagonal().any(), (what, kind)
                dev = rel_dev(got, want)
                worst = max(worst, dev)
                assert dev <= DIST_BAR, (what, kind, dev)
    print("largest relative deviation of the host path: %.3g" % worst)
    _, rows = dist_cases()[1]
    D, ns = E.msa_distances(rows, "JC69", host=True)
    assert ns >= 1 and D[3, 4] == D.max() == 2 * np.unique(D)[-2]
    assert E.msa_distances(rows, "JC69", sat=7.0, host=True)[0][3, 4] == 7.0
    assert E.msa_distances(rows, "pdist", host=True)[1] == 0


def test_what_the_distances_refuse():
    rows = synth_rows(6, 40, 1)
    with pytest.raises(E.EngineError, match="base frequencies"):
        E.msa_distances(rows, "TN93", host=True)
    with pytest.raises(E.EngineError, match="code 4"):
        E.msa_pair_counts(np.full((3, 5), 4, np.int8), host=True)
    with pytest.raises(E.EngineError, match="65535"):
        E.msa_pair_counts(np.zeros((3, 65536), np.int8), host=True)
    allsat = np.array([[0] * 8, [1] * 8, [3] * 8], np.int8)
    with pytest.raises(E.EngineError, match="every pair of rows is saturated"):
        E.msa_distances(allsat, "JC69", host=True)
    assert E.msa_distances(allsat, "JC69", sat=1.0, host=True)[1] == 3


# ---- CPU: the program, --host ----

def write_fasta(path, names, seqs):
    with open(path, "w") as f:
        for nm, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (nm, s))
    return str(path)


def read_dist_out(path):
    with open(path) as f:
        n = int(f.readline())
        names, rows = [], []
        for line in f:
            x = line.rstrip("\n").split("\t")
            names.append(x[0]); rows.append([float(v) for v in x[1:]])
    D = np.array(rows)
    assert D.shape == (n, n) and len(names) == n
    return names, D


def check_program_tree(text, names, D):
    """the text parses to n leaves under a top node of degree 3 with n - 3 more inner nodes, and it is hu_nj's tree of D"""
    n = len(names)
    nw = E.newick_parse(text)
    kids = [len(c) for c in nw["children"]]
    root = int(np.nonzero(nw["parent"] < 0)[0][0])
    assert len(kids) == 2 * n - 2 and kids.count(0) == n and kids[root] == 3 and kids.count(2) == n - 3
    assert sorted(nw["names"][i] for i in range(len(kids)) if kids[i] == 0) == sorted(names)
    assert all(nw["names"][i] == "" for i in range(len(kids)) if kids[i] > 0)
    assert text == E.nj_newick(names, E.nj(D, host=True))


@pytest.mark.parametrize("args,kind,model,sat", [([], "JC69", None, None), (["-sm", sm("GTR")], "TN93", "GTR", None), (["-sm", sm("K80")], "K80", "K80", None),
                                                 (["--dist", "pdist"], "pdist", None, None),
                                                 (["-sm", sm("HKY85"), "--dist", "F81", "--sat", "3"], "F81", "HKY85", 3.0)])
def test_program_on_the_host(tmp_path, args, kind, model, sat):
    out, dist = tmp_path / "out.tree", tmp_path / "dist.txt"
    r = _run([_bin(), FASTA70, "--host", "-o", out, "--dist-out", dist, "-v"] + args)
    assert r.returncode == 0, r.stderr
    if model == "GTR":
        assert "TN93 with the model's base frequencies" in r.stderr
    names, D = read_dist_out(dist)
    n70, rows = rows70()
    assert names == n70
    want, _ = E.msa_distances(rows, kind, model_pi(sm(model)) if model else None, sat, host=True)
    assert np.array_equal(D, want)
    check_program_tree(out.read_text(), names, D)
    r2 = _run([_bin(), FASTA70, "--host"] + args)
    assert r2.returncode == 0 and r2.stdout == out.read_text()


def model_pi(path):
    """the base frequencies of a model file, through the library's own reader"""
    import ctypes as C
    md = E.ModelDesc()
    b = open(path, "rb").read()
    kind = [l.split()[1] for l in b.decode().splitlines() if l.startswith("Type:")][0]
    b = kind.encode() + b"\n" + b                      # the reader takes the type's word first, as the .ptu carries it
    E._chk(E.load_library().hu_model_parse_text(b, C.c_int64(len(b)), C.byref(md)))
    return np.array([md.pi[i] for i in range(4)])


def test_program_quotes_names_and_writes_lengths_in_full(tmp_path):
    fa = write_fasta(tmp_path / "q.fasta", ["a(b)", "c", "d:e", "f"], ["ACGTACGTAC", "ACGTACGTAA", "ACGAACGTAA", "TCGAACG-AA"])
    r = _run([_bin(), fa, "--host"])
    assert r.returncode == 0, r.stderr
    assert "'a(b)':" in r.stdout and "'d:e':" in r.stdout
    nw = E.newick_parse(r.stdout)
    assert sorted(x for x in nw["names"] if x) == ["a(b)", "c", "d:e", "f"]


def test_what_the_program_refuses(tmp_path):
    good = ["ACGTACGTAC", "ACGTACGTAA", "ACGAACGTAA"]
    fa3 = write_fasta(tmp_path / "three.fasta", "abc", good)
    fa2 = write_fasta(tmp_path / "two.fasta", "ab", good[:2])
    dup = write_fasta(tmp_path / "dup.fasta", "aba", good)
    msa = write_fasta(tmp_path / "x.msa", "abc", good)
    wide = write_fasta(tmp_path / "wide.fasta", "abc", [s * 6554 for s in good])
    out = tmp_path / "o.tree"
    for args, why in (([fa2], "at least 3 sequences"), ([dup], "Non-unique seq name"), ([msa], "binary .msa"), ([fa3, "--fmt", "msa"], "binary .msa"),
                      ([fa3, "--dist", "TN93"], "-sm is required"), ([fa3, "--dist", "F81"], "-sm is required"), ([fa3, "--dist", "HKY85"], "-sm is required"),
                      ([fa3, "--dist", "GTR"], "Unsupported distance"), ([fa3, "--sat", "0"], "--sat must be positive"), ([fa3, "--sat", "-1"], "--sat must be positive"),
                      ([wide], "65535 at the most")):
        r = _run([_bin()] + args + ["-o", out, "--dist-out", tmp_path / "o.dist"])
        assert r.returncode != 0 and why in r.stderr, (args, r.stderr)
        assert "device" not in r.stderr and len(r.stderr.strip().splitlines()) == 1, r.stderr
        assert not out.exists() and not (tmp_path / "o.dist").exists()
    r = _run([_bin(), fa3, "--host"])
    assert r.returncode == 0 and r.stdout.count(":") == 3


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_nj_host.cpp (the checks, the host paths and the Newick writer; no HIP headers) with tests/san/nj_driver.cpp under
    AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nj_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "nj_driver.cpp"), os.path.join(CSRC, "hu_nj_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "40"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "125 cases" in r.stdout


# ---- the device ----

def device_rows(n, L):
    """the first n rows and L columns of one set of synthetic rows, so that the sizes share their restatement's inputs"""
    return np.ascontiguousarray(cached(("devrows",), lambda: synth_rows(129, 1000, 9))[:n, :L])


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(3, 70), (63, 70), (64, 70), (65, 70), (129, 70), (65, 1), (65, 63), (65, 64), (65, 65), (65, 129), (65, 1000)])
def test_device_pair_counts_and_distances(n, L):
    """the edges of a tile (64 rows), of a plane word (64 columns) and a partial last chunk (8 words): counts exact, distances under the bar"""
    _need_gpu()
    rows = device_rows(n, L)
    want = cached(("devcnt", n, L), lambda: ref_counts(rows))
    assert np.array_equal(E.msa_pair_counts(rows), want)
    worst = 0.0
    for kind in TYPES:
        for sat in (None, 2.5):
            got, gs = E.msa_distances(rows, kind, PI, sat)
            host, hs = E.msa_distances(rows, kind, PI, sat, host=True)
            assert gs == hs and np.array_equal(got, got.T) and not got.diagonal().any()
            dev = rel_dev(got, host)
            worst = max(worst, dev)
            assert dev <= DIST_BAR, (kind, dev)
    print("largest relative deviation of the device from the host path at n %d, L %d: %.3g" % (n, L, worst))


@pytest.mark.gpu
def test_device_distances_of_70_otus_meet_the_bar():
    _need_gpu()
    names, rows = rows70()
    worst = 0.0
    for kind in TYPES:
        want, ns = cached(("dist", "70_otus", kind, None), lambda: ref_distances(rows, kind, PI, None))
        got, gs = E.msa_distances(rows, kind, PI)
        assert gs == ns
        worst = max(worst, rel_dev(got, want))
    print("largest relative deviation of the device from the restatement on 70_otus: %.3g" % worst)
    assert worst <= DIST_BAR


def device_equals_host(D):
    host = E.nj(D, host=True)
    dev = E.nj(D)
    assert same_tree(dev, host)
    assert same_tree(E.nj(D), dev)                     # a second run: the same bits
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 33, 65, 130])
def test_device_nj_additive_and_integer_matrices(n):
    _need_gpu()
    device_equals_host(cached(("add", n, 1), lambda: random_additive(n, 100 * n + 1)))
    if n in (5, 33, 65):
        device_equals_host(cached(("int", n, 1), lambda: random_integer(n, 7 * n + 1)))
    if n == 5:
        device_equals_host(cached(("int", 17, 1), lambda: random_integer(17, 7 * 17 + 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["JC69", "TN93"])
def test_device_nj_on_the_distances_of_70_otus(kind):
    _need_gpu()
    names, rows = rows70()
    D, _ = E.msa_distances(rows, kind, PI, host=True)
    device_equals_host(D)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257, 513, 1030])
def test_device_nj_sizes(n):
    """across the argmin's 256 lanes, the blocks of 256 of the row sums, and at 1030 its 1024 workgroups, which then take more than one
    row each; float matrices whose every operation rounds, and a constant one where every Q ties"""
    _need_gpu()
    rng = np.random.default_rng(n)
    a = np.triu(rng.random((n, n)) + 0.05, 1)
    device_equals_host(a + a.T)
    device_equals_host(np.ones((n, n)) - np.eye(n))


@pytest.mark.gpu
def test_program_on_the_device(tmp_path):
    """the tree is hu_nj's host tree of the program's own --dist-out matrix (not --host end to end: the device's log may differ from
    libm's in the last bit and flip a near-tie)"""
    _need_gpu()
    out, dist = tmp_path / "out.tree", tmp_path / "dist.txt"
    r = _run([_bin(), FASTA70, "-sm", sm("GTR"), "-o", out, "--dist-out", dist, "-v"])
    assert r.returncode == 0, r.stderr
    assert "joins" in r.stderr
    names, D = read_dist_out(dist)
    check_program_tree(out.read_text(), names, D)
    host, _ = E.msa_distances(rows70()[1], "TN93", model_pi(sm("GTR")), host=True)
    assert rel_dev(D, host) <= DIST_BAR


@pytest.mark.gpu
def test_tree_train_sm_build_end_to_end(tmp_path):
    """hmmufotu-amd-tree -> hmmufotu-amd-train-sm -> hmmufotu-amd-build --no-hmm: a database from the alignment alone"""
    _need_gpu()
    r = _run([_bin(), FASTA70, "-o", "nj.tree"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-train-sm"), FASTA70, "nj.tree", "-o", "nj.sm", "-s", "HKY85"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    r = _run([_bin("hmmufotu-amd-build"), FASTA70, "nj.tree", "--no-hmm", "-sm", "nj.sm", "-n", "njdb"], cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    db = E.parse_files(ptu_path=str(tmp_path / "njdb.ptu"))
    par = db["parent"]
    leaves = db["n_nodes"] - len(set(int(p) for p in par if p >= 0))
    assert leaves == len(rows70()[0]) == 125


@pytest.mark.gpu
def test_device_memory_refusal_names_both_numbers(tmp_path):
    _need_gpu()
    n = 600
    a = np.triu(np.ones((n, n)), 1)
    with pytest.raises(E.EngineError, match=r"need (\d+) bytes of device memory .*, 1048576 bytes are free") as ei:
        E.nj(a + a.T, mem_budget=1 << 20)
    assert "error -4" in str(ei.value)
    assert int(str(ei.value).split("need ")[1].split(" ")[0]) >= n * n * 8 + (1 << 20)
    r = _run([_bin(), FASTA70, "--mem", "0.0001", "-o", tmp_path / "o.tree"])
    assert r.returncode != 0 and "bytes of device memory" in r.stderr and "100000 bytes are free" in r.stderr and not (tmp_path / "o.tree").exists()
