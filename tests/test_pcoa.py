"""hmmufotu-amd-pcoa: hu_pcoa on the host and on the device, and the program.

The yardstick lives in this file and shares no code with the library: B = -1/2 J (d * d) J formed in numpy from the exact d, and
numpy.linalg.eigh of it.  The library's coordinates, eigenvalues and residuals are held against it and against themselves:
  certificate   | B u_a - lambda_a u_a | recomputed here agrees with the reported res_a within the allowance, and res_a <= tol lambda_1
  eigenvalues   | lambda_a - eigh's a-th largest | <= res_a + allowance                                              (Weyl)
  coordinates   on fixtures with a planted spectrum (points whose axes are scaled 8, 4, 2, 1, ...), after the same sign rule:
                | x_a - yardstick's | <= 2 res_a / gap_a sqrt(lambda_a) + allowance sqrt(lambda_1)                    (Davis-Kahan)
                with every gap_a asserted above 1e-3 lambda_1 first
  trace         the bits of engine.permanova's ss_total
The allowance is the yardstick's own rounding, measured: eigvalsh(B) against eigvalsh(P B P') for the reversal P, which have one
spectrum exactly.  The worst difference over the fixtures of this file was 1.04e-15 lambda_1 (OpenBLAS, x86-64); ALLOW is 8 times that."""
import functools
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hmmufotu_amd import engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hmmufotu_amd", "csrc")
ALLOW = 8 * 1.04e-15          # relative to lambda_1; measured 1.04e-15 (test_the_allowance_covers_the_yardsticks_noise prints it)
TOL = 1e-10


def _bin(name="hmmufotu-amd-pcoa"):
    p = os.path.join(ROOT, "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return p


def _run(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120, **kw)


def _need_gpu():
    if E.device_count() < 1:
        pytest.fail("no gfx950 device")


# ---- the yardstick ----

class Yard:
    def __init__(self, d):
        n = len(d)
        J = np.eye(n) - np.ones((n, n)) / n
        self.d = d; self.n = n
        self.B = -0.5 * J @ (d * d) @ J
        w, v = np.linalg.eigh(self.B)
        self.w = w[::-1].copy(); self.v = v[:, ::-1].copy()
        self.l1 = self.w[0]
        self.noise = np.abs(np.linalg.eigvalsh(self.B) - np.linalg.eigvalsh(self.B[::-1, ::-1])).max() / self.l1

    def gap(self, a):
        return np.abs(np.delete(self.w, a) - self.w[a]).min()

    def coords(self, a):
        return sign_rule(self.v[:, a]) * math.sqrt(self.w[a])


def sign_rule(u):
    return u if u[np.argmax(np.abs(u))] > 0 else -u


def euclid(X):
    n = len(X)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = math.sqrt(float(((X[i] - X[j]) ** 2).sum()))
    return d


SEEDS = {3: 1, 4: 4, 7: 6}     # a handful of random points can fall nearly flat: these draws keep every gap above 0.1 lambda_1


@functools.lru_cache(maxsize=None)
def planted(n, q, seed=None):
    """n points in q dimensions, the axes scaled 8, 4, 2, 1, ...: eigenvalues near n (64, 16, 4, 1, ...)"""
    X = np.random.default_rng(SEEDS.get(n, 3) if seed is None else seed).standard_normal((n, q)) * (8.0 / 2.0 ** np.arange(q))
    d = euclid(X)
    d.setflags(write=False)
    return d, Yard(d)


@functools.lru_cache(maxsize=None)
def generic(n, seed=5):
    """n points in n - 1 dimensions: n - 1 positive eigenvalues, no planted gaps"""
    d = euclid(np.random.default_rng(seed).standard_normal((n, n - 1)))
    d.setflags(write=False)
    return d, Yard(d)


@functools.lru_cache(maxsize=None)
def lattice_with_a_negative_axis():
    """27 lattice points (8 p_a, 4 p_b, 2 p_c), a, b, c in 0..2 and p = (0, 1, 2.5): eigenvalues 1824, 456, 114 (p is not symmetric about
    its mean, so no entry of an eigenvector ties with one of the other sign); minus c y y' with y = (1.5, -2.5, 1)[a], which is orthogonal to
    the constant and to every lattice axis: one more eigenvalue, -85.5 c = -300.  y differs only between points with different a, where
    c (y_i - y_j)^2 <= 56.2 stays below the squared distance of at least 64: every squared distance stays positive."""
    idx = np.array([(a, b, c) for a in range(3) for b in range(3) for c in range(3)])
    X = np.array([0.0, 1.0, 2.5])[idx] * np.array([8.0, 4.0, 2.0])
    y = np.array([1.5, -2.5, 1.0])[idx[:, 0]]
    G = X @ X.T - (300.0 / 85.5) * np.outer(y, y)
    D2 = np.diag(G)[:, None] + np.diag(G)[None, :] - 2 * G
    D2 = 0.5 * (D2 + D2.T); np.fill_diagonal(D2, 0.0)
    assert (D2[~np.eye(27, dtype=bool)] > 0).all()
    d = np.sqrt(D2)
    d.setflags(write=False)
    return d, Yard(d)


@functools.lru_cache(maxsize=None)
def bray_curtis(tmp):
    """the Bray-Curtis matrix hmmufotu-amd-unifrac --host writes for a small sparse random table"""
    rng = np.random.default_rng(8)
    counts = rng.integers(0, 30, (12, 14)) * (rng.random((12, 14)) < 0.4); counts[0] += 1
    names = ["site %d" % j for j in range(14)]
    with open(os.path.join(tmp, "t.txt"), "w") as f:
        f.write("# HmmUFOtu v1.5.1 OTU table generated by test\notuID\t" + "\t".join(names) + "\ttaxonomy\n")
        for i, row in enumerate(counts):
            f.write("%d\t%s\t\n" % (i, "\t".join(str(v) for v in row)))
    u = _run([_bin("hmmufotu-amd-unifrac"), os.path.join(tmp, "t.txt"), "--method", "bray-curtis", "--host", "-o", os.path.join(tmp, "bc.txt")])
    assert u.returncode == 0, u.stderr
    m = E.dist_matrix_read(os.path.join(tmp, "bc.txt"))
    assert m["samples"] == names
    return m["dist"], Yard(m["dist"]), names, os.path.join(tmp, "bc.txt")


@pytest.fixture(scope="module")
def bc(tmp_path_factory):
    return bray_curtis(str(tmp_path_factory.mktemp("bc")))


# ---- the bars ----

def col_bar(r, y, a):
    return 2 * r["resid"][a] / y.gap(a) * math.sqrt(r["eigval"][a]) + ALLOW * math.sqrt(y.l1)


def hold(r, y, k, what="", coords=False, tol=TOL):
    """the certificate, the eigenvalues and the trace of every fixture; the coordinates where the spectrum is planted"""
    lam, res, x = r["eigval"], r["resid"], r["coords"]
    assert r["n"] == y.n and r["k"] == k and x.shape == (y.n, k), what
    assert (lam > 0).all() and (np.diff(lam) <= 0).all(), (what, lam)
    u = x / np.sqrt(lam)
    again = np.linalg.norm(y.B @ u - u * lam, axis=0)
    for a in range(k):
        print("%s axis %d: lambda %.17g eigh %.17g res %.3g recomputed %.3g (tol lambda_1 %.3g)" % (what, a + 1, lam[a], y.w[a], res[a], again[a], tol * lam[0]))
        assert abs(np.linalg.norm(u[:, a]) - 1) <= ALLOW, what
        assert abs(again[a] - res[a]) <= ALLOW * y.l1, (what, a, again[a], res[a])
        assert res[a] <= tol * lam[0], (what, a, res[a])
        assert abs(lam[a] - y.w[a]) <= res[a] + ALLOW * y.l1, (what, a, lam[a], y.w[a])
        assert u[np.argmax(np.abs(u[:, a])), a] > 0, what
    assert np.array_equal(r["prop"], lam / r["trace"])
    assert r["trace"] == E.permanova(y.d, [0, 1] + [0] * (y.n - 2), perms=1, host=True)["ss_total"], what
    if coords:
        for a in range(k):
            assert y.gap(a) > 1e-3 * y.l1, (what, a)
            err = np.linalg.norm(x[:, a] - y.coords(a))
            print("%s axis %d: coordinates off by %.3g, bar %.3g" % (what, a + 1, err, col_bar(r, y, a)))
            assert err <= col_bar(r, y, a), (what, a, err, col_bar(r, y, a))


def within_each_other(r1, r2, y, k, what):
    """two certified results of one matrix: within the sum of their bars"""
    for a in range(k):
        assert abs(r1["eigval"][a] - r2["eigval"][a]) <= r1["resid"][a] + r2["resid"][a] + 2 * ALLOW * y.l1, (what, a)
        assert np.linalg.norm(r1["coords"][:, a] - r2["coords"][:, a]) <= col_bar(r1, y, a) + col_bar(r2, y, a), (what, a)


def same_bits(r1, r2):
    return all(r1[f].tobytes() == r2[f].tobytes() for f in ("coords", "eigval", "resid")) and all(r1[f] == r2[f] for f in ("iterations", "m_final", "trace"))


# ---- the host path ----

def test_the_allowance_covers_the_yardsticks_noise(bc):
    ys = [planted(n, q)[1] for n, q in ((3, 2), (4, 3), (7, 3), (65, 3), (63, 3), (64, 3), (129, 3), (280, 3))]
    ys += [generic(7)[1], generic(65)[1], lattice_with_a_negative_axis()[1], bc[1]]
    worst = max(y.noise for y in ys)
    print("the yardstick's noise: %.3g lambda_1 at the most; ALLOW %.3g" % (worst, ALLOW))
    assert worst <= ALLOW
    for y in ys:                                                            # and with it the first axis of every fixture holds its bars
        hold(E.pcoa(y.d, k=1, host=True), y, 1, "n %d first axis" % y.n)


def test_four_points_of_a_square_by_hand():
    """the corners of the unit square: B = X X' of the centred corners, eigenvalues 1, 1, 0, 0.  The two equal eigenvalues fix a plane,
    not its axes: the projector U U' (= B itself here) is compared, not the columns."""
    s = math.sqrt(2.0)
    d = np.array([[0, 1, s, 1], [1, 0, 1, s], [s, 1, 0, 1], [1, s, 1, 0]])
    r = E.pcoa(d, k=2, host=True)
    want = np.array([[0.5, 0, -0.5, 0], [0, 0.5, 0, -0.5], [-0.5, 0, 0.5, 0], [0, -0.5, 0, 0.5]])
    bar = r["resid"].max() + ALLOW + 4 * 2.0 ** -52                       # the rounded sqrt(2) moves a squared diagonal by 2^-51
    assert np.abs(r["eigval"] - 1.0).max() <= bar
    u = r["coords"] / np.sqrt(r["eigval"])
    assert np.abs(u @ u.T - want).max() <= 4 * bar                          # an eigenvalue gap of 1 to the two zeros
    assert abs(r["trace"] - 2.0) <= 4 * 2.0 ** -51 and abs(r["prop"].sum() - 1) <= bar
    assert r["iterations"] == 1 and r["m_final"] == 3
    with pytest.raises(E.EngineError, match=r"only 2 positive axes; 3 asked"):
        E.pcoa(d, k=3, host=True)


@pytest.mark.parametrize("n,k", [(3, 1), (3, 2), (4, 1), (4, 2), (4, 3), (7, 1), (7, 2), (65, 1), (65, 2)])
def test_host_planted_sizes(n, k):
    d, y = planted(n, min(3, n - 1))
    r = E.pcoa(d, k=k, host=True)
    hold(r, y, k, "n %d k %d" % (n, k), coords=True)
    assert r["m_final"] == min(k + 8, n - 1)
    assert r["prop"].sum() <= 1 + ALLOW


@pytest.mark.parametrize("n", [7, 65])
def test_host_every_axis(n):
    """k = n - 1: the block spans the whole centred space and one Rayleigh-Ritz step is exact"""
    d, y = generic(n)
    r = E.pcoa(d, k=n - 1, host=True)
    hold(r, y, n - 1, "n %d every axis" % n)
    assert r["iterations"] == 1 and r["m_final"] == n - 1 and r["positive_in_block"] == n - 1
    assert abs(r["prop"].sum() - 1) <= (n - 1) * ALLOW + r["resid"].sum() / r["trace"]


def test_distances_come_back():
    d, y = planted(65, 3)
    r = E.pcoa(d, k=3, host=True)
    hold(r, y, 3, "distances", coords=True)
    bar = 2 * sum(col_bar(r, y, a) for a in range(3)) + ALLOW * math.sqrt(y.l1)
    assert np.abs(euclid(r["coords"]) - d).max() <= bar


def test_bray_curtis_is_not_euclidean(bc):
    d, y, _, _ = bc
    neg = int((y.w < -ALLOW * y.l1).sum()); posn = int((y.w > ALLOW * y.l1).sum())
    assert neg >= 1 and posn + neg == y.n - 1
    for k in (1, 3, posn):
        r = E.pcoa(d, k=k, host=True)
        hold(r, y, k, "bray-curtis k %d" % k)
    assert r["prop"].sum() > 1                                              # the positive axes alone exceed the trace
    with pytest.raises(E.EngineError, match=r"only %d positive axes; %d asked" % (posn, posn + 1)) as ei:
        E.pcoa(d, k=posn + 1, host=True)
    assert "error -6" in str(ei.value)


def test_a_negative_axis_larger_than_the_kth_positive():
    """magnitudes 1824, 456, 300 (negative), 114: a choice by magnitude takes the negative axis for the third"""
    d, y = lattice_with_a_negative_axis()
    assert abs(y.w[-1] + 300) < 1e-9 and abs(y.w[2] - 114) < 1e-9 and -y.w[-1] > y.w[2]
    r = E.pcoa(d, k=3, oversample=0, host=True)
    hold(r, y, 3, "negative axis", coords=True)
    assert r["m_final"] == 11 and r["positive_in_block"] == 3               # the block of 3 held two positive axes and was widened
    hold(E.pcoa(d, k=3, host=True), y, 3, "negative axis, default block", coords=True)


def test_the_widest_block_refuses_once_its_ritz_values_have_settled():
    """three positive axes and four asked, n - 1 > 64: the block is widened to 64 columns, where the count is what a settled block holds,
    not a count of B's axes, and the message says so"""
    d, y = planted(129, 3)
    with pytest.raises(E.EngineError, match=r"3 positive axes found in a settled block of 64 columns, the widest; 4 asked") as ei:
        E.pcoa(d, k=4, host=True)
    assert "error -6" in str(ei.value)
    with pytest.raises(E.EngineError, match=r"no convergence in 2 iterations: the block of 12 columns holds 3 positive axes of the 4 asked"):
        E.pcoa(d, k=4, max_it=2, host=True)
    with pytest.raises(E.EngineError, match=r"oversample 4294967296 above 2147483647"):
        E.pcoa(d, k=3, oversample=1 << 32)


def test_host_is_deterministic_and_seeds_agree():
    d, y = planted(65, 3)
    a = E.pcoa(d, k=3, oversample=1, host=True); b = E.pcoa(d, k=3, oversample=1, host=True)
    assert same_bits(a, b) and a["iterations"] > 1
    c = E.pcoa(d, k=3, oversample=1, seed=77, host=True)
    assert not same_bits(a, c)
    hold(c, y, 3, "seed 77", coords=True)
    within_each_other(a, c, y, 3, "seeds 1 and 77")


def slabs(n):
    return min(8, -(-n // 128))


def need(n, k, over):
    m = min(k + over, n - 1); mp = -(-m // 16) * 16; c = -(-n // 256)
    return 8 * n * n + 8 * (slabs(n) + 4) * n * mp + 8 * (c + 3) * mp * mp + 8 * c * mp + (1 << 20)


def test_need_and_slabs_are_the_documented_functions():
    for n, k, over in ((3, 1, 0), (3, 2, 8), (65, 3, 8), (280, 3, 30), (4096, 10, 8), (16384, 10, 8), (16384, 3, 61)):
        assert E.pcoa_need(n, k, over) == need(n, k, over), (n, k, over)
    for bad in ((2, 1, 0), (5, 0, 8), (5, 5, 8), (5, 1, -1), (100, 3, 62)):
        assert E.pcoa_need(*bad) == -1, bad
    assert [E.pcoa_slabs(n) for n in (1, 128, 129, 280, 1024, 1025, 16384, 0)] == [1, 1, 2, 3, 8, 8, 8, -1]


def test_what_the_library_refuses():
    d, _ = planted(7, 3)
    for kw, why in ((dict(k=0), "0 axes of 7 samples: between 1 and 6"), (dict(k=7), "7 axes of 7 samples"), (dict(oversample=-1), "oversample -1 below 0"),
                    (dict(tol=0.0), "tol 0: above 0"), (dict(tol=2e-3), "tol 0.002"), (dict(tol=float("nan")), "tol nan"), (dict(max_it=0), "max_it 0 below 1")):
        with pytest.raises(E.EngineError, match=why) as ei:
            E.pcoa(d, **kw)                                                # no host=True: refused before a device is asked for
        assert "error -1" in str(ei.value) and "device" not in str(ei.value)
    with pytest.raises(E.EngineError, match="2 samples: principal coordinates need 3"):
        E.pcoa(np.array([[0.0, 1], [1, 0]]), k=1)
    big, _ = planted(129, 3)
    with pytest.raises(E.EngineError, match="a block of 65 columns .*: 64 at the most"):
        E.pcoa(big, k=3, oversample=62)
    for change, why in ((lambda x: x.__setitem__((1, 2), 9.0), r"not symmetric: d\(1, 2\)"), (lambda x: x.__setitem__((2, 2), 0.5), "sample 2 is at the distance 0.5 from itself"),
                        (lambda x: (x.__setitem__((0, 3), -1.0), x.__setitem__((3, 0), -1.0)), "samples 0 and 3 is negative or not finite"),
                        (lambda x: (x.__setitem__((0, 3), np.inf), x.__setitem__((3, 0), np.inf)), "samples 0 and 3 is negative or not finite"),
                        (lambda x: x.fill(0.0), "every distance is 0")):
        x = d.copy(); change(x)
        with pytest.raises(E.EngineError, match=why) as ei:
            E.pcoa(x, k=2)
        assert "hu_pcoa" in str(ei.value) and "device" not in str(ei.value)


def test_memory_refusal_names_both_numbers():
    d, _ = planted(65, 3)
    with pytest.raises(E.EngineError, match=r"block of 11 columns need %d bytes of device memory .*, 1048576 bytes are free" % need(65, 3, 8)) as ei:
        E.pcoa(d, k=3, mem_budget=1 << 20)
    assert "error -4" in str(ei.value)


def test_no_convergence_is_refused_with_the_worst_residual():
    d, y = planted(65, 3)
    assert E.pcoa(d, k=1, oversample=0, host=True)["iterations"] > 5        # one column: the plain power method
    with pytest.raises(E.EngineError, match=r"no convergence in 1 iterations: axis 1 has the residual [0-9.e+-]+, above tol \* lambda_1 = ") as ei:
        E.pcoa(d, k=1, oversample=0, max_it=1, host=True)
    assert "error -6" in str(ei.value)


# ---- the program ----

def _write_matrix(path, names, d):
    with open(path, "w") as f:
        f.write("".join("\t" + s for s in names) + "\n")
        for s, row in zip(names, d):
            f.write(s + "".join("\t" + repr(float(v)) for v in row) + "\n")


def _read_coords(text, k):
    lines = text.rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["sample"] + ["PC%d" % (a + 1) for a in range(k)]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert all(len(r) == k + 1 for r in rows)
    return [r[0] for r in rows], np.array([[float(v) for v in r[1:]] for r in rows])


def _read_eig(text, k):
    lines = text.rstrip("\n").split("\n")
    assert lines[0] == "axis\teigenvalue\tproportion\tresidual" and len(lines) == k + 4
    rows = [ln.split("\t") for ln in lines[1:k + 1]]
    assert [r[0] for r in rows] == [str(a + 1) for a in range(k)]
    tail = dict(ln[2:].split(": ") for ln in lines[k + 1:])
    assert all(ln.startswith("# ") for ln in lines[k + 1:]) and list(tail) == ["trace", "iterations", "block"]
    return np.array([[float(v) for v in r[1:]] for r in rows]), tail


def test_program_on_the_host(tmp_path):
    d, y = planted(65, 3)
    names = ["s %d" % i for i in range(65)]
    _write_matrix(tmp_path / "d.txt", names, d)
    r = _run([_bin(), tmp_path / "d.txt", "--host", "-k", 2, "--eig-out", tmp_path / "e.txt", "-v"])
    assert r.returncode == 0, r.stderr
    assert "iteration(s)" in r.stderr and "residual" in r.stderr
    lib = E.pcoa(d, k=2, host=True)
    got_names, x = _read_coords(r.stdout, 2)
    assert got_names == names and x.tobytes() == lib["coords"].tobytes()   # 17 significant digits: the doubles themselves
    e, tail = _read_eig((tmp_path / "e.txt").read_text(), 2)
    assert e[:, 0].tobytes() == lib["eigval"].tobytes() and e[:, 1].tobytes() == lib["prop"].tobytes() and e[:, 2].tobytes() == lib["resid"].tobytes()
    assert float(tail["trace"]) == lib["trace"] and int(tail["iterations"]) == lib["iterations"] and int(tail["block"]) == lib["m_final"] == 10
    o = _run([_bin(), tmp_path / "d.txt", "--host", "--axes", 2, "-o", tmp_path / "c.txt", "--seed", 1, "--oversample", 8, "--tol", 1e-10, "--max-it", 1000])
    assert o.returncode == 0 and o.stdout == "" and (tmp_path / "c.txt").read_text() == r.stdout


def test_program_reads_what_unifrac_writes(bc):
    """the program is given the very file hmmufotu-amd-unifrac --host -o wrote: its header, its names with blanks, its numbers"""
    d, y, names, path = bc
    r = _run([_bin(), path, "--host"])
    assert r.returncode == 0, r.stderr
    got_names, x = _read_coords(r.stdout, 3)
    lib = E.pcoa(d, k=3, host=True)                                       # d: the same file through engine.dist_matrix_read
    assert got_names == names and x.tobytes() == lib["coords"].tobytes()
    hold(lib, y, 3, "bray-curtis by the program")


GOOD = "\ta\tb\tc\td\na\t0\t1\t2\t3\nb\t1\t0\t1.5\t2\nc\t2\t1.5\t0\t1\nd\t3\t2\t1\t0\n"


@pytest.mark.parametrize("dist,args,why", [
    (GOOD, ["-k", "0"], "--axes must be at least 1"),
    (GOOD, ["-k", "4"], "4 axes of 4 samples: between 1 and 3"),
    (GOOD, ["--tol", "0"], "--tol must lie above 0"),
    (GOOD, ["--tol", "0.01"], "--tol must lie above 0"),
    (GOOD, ["--max-it", "0"], "--max-it must be at least 1"),
    (GOOD, ["--oversample", "-1"], "--oversample must be non-negative"),
    (GOOD, ["--mem", "-1"], "--mem must be a positive number of GB"),
    (GOOD, ["--bogus"], "unknown option --bogus"),
    (GOOD.replace("\t3\n", "\t4\n", 1), [], "not symmetric: d(0, 3) = 4, d(3, 0) = 3"),
    (GOOD.replace("1.5", "-1.5"), [], "samples 1 and 2 is negative or not finite"),
    (GOOD.replace("c\t2\t1.5\t0", "c\t2\t1.5\t0.25"), [], "sample 2 is at the distance 0.25 from itself"),
    (GOOD.replace("1.5", "x"), [], "line 3: 'x' is not a number"),
    ("\ta\tb\na\t0\t1\nb\t1\t0\n", ["-k", "1"], "2 samples: principal coordinates need 3 at the least"),
    ("\ta\tb\tc\na\t0\t0\t0\nb\t0\t0\t0\nc\t0\t0\t0\n", ["-k", "1"], "every distance is 0"),
    (GOOD, ["--mem", "0.0005"], "need %d bytes of device memory" % need(4, 3, 8)),
])
def test_what_the_program_refuses(tmp_path, dist, args, why):
    (tmp_path / "d.txt").write_text(dist)
    out = tmp_path / "o.txt"; eig = tmp_path / "e.txt"
    r = _run([_bin(), tmp_path / "d.txt", "-o", out, "--eig-out", eig] + args)      # no --host: refused before a device is asked for
    assert r.returncode != 0 and why in r.stderr, r.stderr
    assert len(r.stderr.strip().split("\n")) == 1
    assert "device" not in r.stderr.replace("bytes of device memory", "")
    assert not out.exists() and not eig.exists()
    if "--mem" in args and "need" in why:
        assert ", 536870 bytes are free" in r.stderr


def test_program_refuses_what_the_iteration_cannot_give(tmp_path):
    d, _ = planted(65, 3)
    _write_matrix(tmp_path / "d.txt", ["s%d" % i for i in range(65)], d)
    r = _run([_bin(), tmp_path / "d.txt", "--host", "-k", 1, "--oversample", 0, "--max-it", 1, "-o", tmp_path / "o.txt", "--eig-out", tmp_path / "e.txt"])
    assert r.returncode != 0 and "no convergence in 1 iterations: axis 1 has the residual" in r.stderr and len(r.stderr.strip().split("\n")) == 1
    assert not (tmp_path / "o.txt").exists() and not (tmp_path / "e.txt").exists()
    s = math.sqrt(2.0)
    _write_matrix(tmp_path / "sq.txt", list("abcd"), np.array([[0, 1, s, 1], [1, 0, 1, s], [s, 1, 0, 1], [1, s, 1, 0]]))
    r = _run([_bin(), tmp_path / "sq.txt", "--host", "-k", 3, "-o", tmp_path / "o.txt"])
    assert r.returncode != 0 and "only 2 positive axes; 3 asked" in r.stderr and not (tmp_path / "o.txt").exists()


def test_program_usage_and_missing_files(tmp_path):
    (tmp_path / "d.txt").write_text(GOOD)
    r = _run([_bin(), tmp_path / "d.txt", tmp_path / "d.txt"])
    assert r.returncode != 0 and "Usage:" in r.stderr
    u = _run([_bin()])
    assert u.returncode == 0 and "--eig-out" in u.stderr and "--oversample" in u.stderr and _run([_bin(), "--help"]).returncode == 0
    v = _run([_bin(), "--version"])
    assert v.returncode == 0 and "v1.5.1" in v.stderr
    r = _run([_bin(), tmp_path / "none.txt", "--host"])
    assert r.returncode != 0 and "Unable to open distance matrix" in r.stderr
    r = _run([_bin(), tmp_path / "d.txt", "--host", "-k", 1, "-o", tmp_path / "no" / "where.txt"])
    assert r.returncode != 0 and "Unable to write to" in r.stderr
    r = _run([_bin(), tmp_path / "d.txt", "--host", "-k", 1, "-o", tmp_path / "c.txt", "--eig-out", tmp_path / "no" / "where.txt"])
    assert r.returncode != 0 and "Unable to write to" in r.stderr and not (tmp_path / "c.txt").exists()


def test_host_code_under_the_sanitizers(tmp_path):
    """hu_pcoa_host.cpp (the checks, the iteration, the m x m work and the host's operations; no HIP headers) and hu_permanova_host.cpp
    (the matrix checks and the trace) with tests/san/pcoa_driver.cpp under AddressSanitizer + UBSan, run as a stand-alone program"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "pcoa_driver")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                        "-o", exe, os.path.join(ROOT, "tests", "san", "pcoa_driver.cpp"), os.path.join(CSRC, "hu_pcoa_host.cpp"), os.path.join(CSRC, "hu_permanova_host.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:allocator_may_return_null=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + "\n" + r.stderr[-4000:]
    assert "35 cases" in r.stdout


# ---- the device ----

DEVICE_CASES = [(3, 2, 8, 2), (4, 3, 8, 3), (63, 1, 0, 1), (64, 3, 12, 15), (65, 3, 13, 16), (129, 3, 14, 17), (129, 3, 29, 32), (280, 3, 29, 32), (280, 3, 30, 33),
                (280, 1, 0, 1), (129, 3, 61, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,over,m", DEVICE_CASES)
def test_device_sizes_and_block_widths(n, k, over, m):
    """the row tile's edges (63, 64, 65), a ragged third tile and two slabs (129), three slabs (280); blocks of 1, 15, 16, 17, 32 and 33
    columns: the edges of the 16-wide accumulator tile and of the padding; 64, the widest"""
    _need_gpu()
    assert E.pcoa_slabs(n) == slabs(n) and (n < 280 or slabs(n) >= 2)
    d, y = planted(n, min(3, n - 1))
    what = "n %d m %d" % (n, m)
    dev = E.pcoa(d, k=k, oversample=over)
    assert dev["m_final"] == m
    hold(dev, y, k, what + " device", coords=True)
    host = E.pcoa(d, k=k, oversample=over, host=True)
    hold(host, y, k, what + " host", coords=True)
    within_each_other(dev, host, y, k, what)
    print("%s: device and host give the same bits: %s" % (what, same_bits(dev, host)))


@pytest.mark.gpu
def test_device_is_deterministic():
    _need_gpu()
    d, y = planted(280, 3)
    a = E.pcoa(d, k=3, oversample=1); b = E.pcoa(d, k=3, oversample=1)
    assert same_bits(a, b) and a["iterations"] > 1
    t = E.pcoa_timing()
    assert t["to_device"] > 0 and t["square"] > 0 and t["product"] > 0 and t["small"] > 0 and t["host_mxm"] > 0 and t["to_host"] > 0
    c = E.pcoa(d, k=3, oversample=1, seed=9)
    hold(c, y, 3, "device seed 9", coords=True)
    within_each_other(a, c, y, 3, "device seeds 1 and 9")


@pytest.mark.gpu
def test_device_negative_axes_and_refusals(bc):
    _need_gpu()
    d, y = lattice_with_a_negative_axis()
    r = E.pcoa(d, k=3, oversample=0)
    hold(r, y, 3, "negative axis on the device", coords=True)
    assert r["m_final"] == 11
    d, y, _, _ = bc
    posn = int((y.w > ALLOW * y.l1).sum())
    hold(E.pcoa(d, k=posn), y, posn, "bray-curtis on the device")
    with pytest.raises(E.EngineError, match=r"only %d positive axes; %d asked" % (posn, posn + 1)):
        E.pcoa(d, k=posn + 1)
    big, _ = planted(65, 3)
    with pytest.raises(E.EngineError, match=r"no convergence in 1 iterations: axis 1 has the residual"):
        E.pcoa(big, k=1, oversample=0, max_it=1)
    wide, _ = planted(129, 3)
    with pytest.raises(E.EngineError, match=r"3 positive axes found in a settled block of 64 columns, the widest; 4 asked"):
        E.pcoa(wide, k=4)


@pytest.mark.gpu
def test_program_on_the_device(tmp_path):
    _need_gpu()
    d, y = planted(129, 3)
    names = ["s%d" % i for i in range(129)]
    _write_matrix(tmp_path / "d.txt", names, d)
    r = _run([_bin(), tmp_path / "d.txt", "-o", tmp_path / "dev.txt", "--eig-out", tmp_path / "dev_e.txt", "-v"])
    assert r.returncode == 0, r.stderr
    assert "product kernel" in r.stderr
    h = _run([_bin(), tmp_path / "d.txt", "-o", tmp_path / "host.txt", "--eig-out", tmp_path / "host_e.txt", "--host"])
    assert h.returncode == 0, h.stderr
    res = []
    for tag in ("dev", "host"):
        nm, x = _read_coords((tmp_path / (tag + ".txt")).read_text(), 3)
        e, tail = _read_eig((tmp_path / (tag + "_e.txt")).read_text(), 3)
        assert nm == names
        res.append(dict(n=129, k=3, coords=x, eigval=e[:, 0].copy(), prop=e[:, 1].copy(), resid=e[:, 2].copy(), trace=float(tail["trace"])))
        hold(res[-1], y, 3, "program " + tag, coords=True)
    within_each_other(res[0], res[1], y, 3, "program")


@pytest.mark.gpu
def test_device_memory_refusal_and_a_budget_that_is_respected():
    _need_gpu()
    d, y = planted(129, 3)
    budget = need(129, 3, 8)
    hold(E.pcoa(d, k=3, mem_budget=budget), y, 3, "a budget that fits", coords=True)
    with pytest.raises(E.EngineError, match=r"block of 11 columns need %d bytes of device memory .*, %d bytes are free" % (budget, budget - 1)) as ei:
        E.pcoa(d, k=3, mem_budget=budget - 1)
    assert "error -4" in str(ei.value)
