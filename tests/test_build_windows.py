"""hmmufotu-amd-build --col-window: a database built a window of columns at a time.

CPU part: the program's refusals of --col-window / --mem (no device, no file); the windowed writer (hu_ptu_writer_*) on host messages against
hu_ptu_write_stream's file, byte for byte, for window widths below, at and above the column count, in ascending and in shuffled order, with
its refusals; the width chooser (hu_build_window_plan) against the formula of include/hmmufotu_amd.h restated here.
GPU part: the program with --col-window against the resident build of the same inputs (hand tree and 70_otus; fixed rates and -V -k 4;
a given width and auto under --mem), the held sweep (hu_tree_sweep_*) against hu_tree_evaluate, and the writer fed device buffers.

Byte equality is the bar throughout: a column's values depend on no other column and on no launch geometry, and the sums that cross
columns are integer counts or serial host sums."""
import filecmp
import os

import numpy as np
import pytest

from conftest import get_db
from hmmufotu_amd import engine as E, synth
from test_build_program import (FASTA70, HAND_JOIN, TAX70, TREE70, _file_order, _refused, hand_rows, need_gpu, run_build, sm, write_fasta)


@pytest.fixture()
def hand_inputs(tmp_path):
    fa, tr = tmp_path / "hand.fasta", tmp_path / "hand.tree"
    write_fasta(fa, hand_rows())
    tr.write_text(HAND_JOIN + "\n")
    return tmp_path, fa, tr


# ----------------------------------------------------------------------------- the formula of include/hmmufotu_amd.h, restated
def py_need(n, W, with_var):
    stage = max(32 * W, min(1 << 28, (2 * n - 1) * 32 * W))
    return 64 * n * W + n * W + ((n * W + 4 * W + 4 * n) if with_var else 0) + 8 * W + 2 * stage + 8 * n + 28 * n + 64


def admissible(L):
    """the widths the chooser may return: every width below 256, and the multiples of 256 from there on"""
    return [w for w in range(1, min(L, 255) + 1)] + list(range(256, L + 1, 256))


def py_plan(n, L, with_var, budget):
    fit = [w for w in admissible(L) if py_need(n, w, with_var) <= budget]
    return max(fit) if fit else 0


# ----------------------------------------------------------------------------- options
def test_usage_lists_the_options(tmp_path):
    r = run_build(["-h"], tmp_path)
    assert r.returncode == 0 and "--col-window" in r.stderr and "--mem" in r.stderr and "auto" in r.stderr


def test_refusals_of_window_options(hand_inputs):
    tmp, fa, tr = hand_inputs
    ok = [fa, tr, "--no-hmm", "-sm", sm("GTR"), "-n", "db"]
    for bad in ("0", "-3", "x", "7x", "1.5", ""):
        _refused(run_build(ok + ["--col-window", bad], tmp), tmp, "--col-window must be 'auto' or an integer >= 1")
    for bad in ("0", "-1", "x", "nan", "inf", "2GB"):
        _refused(run_build(ok + ["--col-window", "auto", "--mem", bad], tmp), tmp, "--mem must be a positive number")
    _refused(run_build(ok + ["--mem", "0"], tmp), tmp, "--mem must be a positive number")


# ----------------------------------------------------------------------------- the windowed writer on host messages
def _host_case():
    rng = np.random.default_rng(18)
    parent, blen, _ = synth.make_tree(20, rng)
    parent = np.asarray(parent, np.int32); blen = np.asarray(blen, np.float64)
    n, L = len(parent), 37
    up = rng.standard_normal((n, L, 4)) * 50 - 100; down = rng.standard_normal((n, L, 4)) * 50 - 100
    up[3, 5, 1] = -np.inf
    seq = rng.integers(0, 4, (n, L)).astype(np.int8); seq[rng.random((n, L)) < 0.1] = -2
    height = rng.random(n)
    db = get_db(60, 300, "GTR", dg_k=4)                         # for its model, rates and breaks
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    off, idx, rows, _, _ = _file_order(parent)
    names = ["node %d" % i if i % 3 else "" for i in range(n)]; annos = ["k__Bacteria;p__%d" % (i % 5) for i in range(n)]
    order = dict(child_off=off, child_idx=idx, msa_row_of_leaf=rows)
    kw = dict(names=names, annos=annos, anno_dist=rng.random(n))
    tail = dict(model_text=db.model.text, dg_alpha=db.dg_alpha, dg_breaks=db.dg_b)
    return parent, blen, seq, up, down, height, md, order, kw, tail


def _windows(L, W):
    return [(a, min(W, L - a)) for a in range(0, L, W)]


def _write_windowed(path, case, wins, on_close=True, **extra):
    parent, blen, seq, up, down, height, md, order, kw, tail = case
    w = E.PtuWriter(path, parent, blen, seq.shape[1], **kw, **order, **extra)
    for a, wl in wins:
        w.window(a, wl, up[:, a:a + wl], down[:, a:a + wl])
    if on_close:
        w.close(seq, height, md, **tail)
    return w


def test_windowed_writer_equals_the_stream_writer(tmp_path):
    case = _host_case()
    parent, blen, seq, up, down, height, md, order, kw, tail = case
    n, L = seq.shape
    assert n == 39 and L == 37
    ref = str(tmp_path / "ref.ptu")
    E.write_ptu_stream(ref, parent, blen, seq, up, down, height, md, **kw, **tail, **order)
    rng = np.random.default_rng(3)
    for W in (1, 5, 36, 37, 100):
        wins = _windows(L, W)
        assert sum(wl for _, wl in wins) == L
        for shuffled in (False, True):
            if shuffled:
                wins = [wins[i] for i in rng.permutation(len(wins))]
            p = str(tmp_path / ("w%d_%d.ptu" % (W, shuffled)))
            _write_windowed(p, case, wins)
            assert filecmp.cmp(ref, p, shallow=False), (W, shuffled)
    # the default child order and index block (NULL order, NULL rows, no names): hu_ptu_write's file
    plain, pw = str(tmp_path / "plain.ptu"), str(tmp_path / "plain_w.ptu")
    E.write_ptu(plain, parent, blen, seq, up, down, height, md, **tail)
    w = E.PtuWriter(pw, parent, blen, L)
    for a, wl in _windows(L, 16):
        w.window(a, wl, up[:, a:a + wl], down[:, a:a + wl])
    w.close(seq, height, md, **tail)
    assert filecmp.cmp(plain, pw, shallow=False)


def test_windowed_writer_refusals_leave_no_file(tmp_path):
    case = _host_case()
    parent, blen, seq, up, down, height, md, order, kw, tail = case
    L = seq.shape[1]
    p = str(tmp_path / "bad.ptu")
    wins = _windows(L, 5)
    for given, word in ((wins[:3] + wins[4:], "no window"), (wins + [wins[2]], "more than once"), ([(0, 20), (15, 22)], "more than once"), ([], "no window")):
        w = _write_windowed(p, case, given, on_close=False)
        assert os.path.exists(p)                                                  # sized and headed by open
        with pytest.raises(E.EngineError) as ei:
            w.close(seq, height, md, **tail)
        assert "error -5" in str(ei.value) and word in str(ei.value), str(ei.value)
        assert not os.path.exists(p)
    w = _write_windowed(p, case, wins, on_close=False)
    w.abort()
    assert not os.path.exists(p)
    w = _write_windowed(p, case, wins[:2], on_close=False)
    for a, wl in ((-1, 5), (35, 3), (0, 0), (0, L + 1)):                        # a window outside the columns: refused, the writer lives on
        with pytest.raises(E.EngineError):
            w.window(a, wl, np.zeros((len(parent), max(wl, 0), 4)), np.zeros((len(parent), max(wl, 0), 4)))
    for a, wl in wins[2:]:
        w.window(a, wl, up[:, a:a + wl], down[:, a:a + wl])
    w.close(seq, height, md, **tail)
    ref = str(tmp_path / "ref.ptu")
    E.write_ptu_stream(ref, parent, blen, seq, up, down, height, md, **kw, **tail, **order)
    assert filecmp.cmp(ref, p, shallow=False)
    del w
    assert os.path.exists(p)                                                      # a closed writer's file stays
    with pytest.raises(E.EngineError):                                            # a child order that is no permutation: refused before a file is made
        E.PtuWriter(str(tmp_path / "never.ptu"), parent, blen, L, child_off=order["child_off"], child_idx=order["child_idx"][::-1].copy())
    assert not os.path.exists(tmp_path / "never.ptu")
    with pytest.raises(E.EngineError):
        E.PtuWriter(str(tmp_path / "no_such_dir" / "x.ptu"), parent, blen, L)


# ----------------------------------------------------------------------------- the width chooser
def test_window_plan_against_the_documented_formula():
    cases = 0
    for n in (2, 9, 249, 99322, 399999):
        for L in (1, 37, 255, 256, 257, 1486, 7682, 65535):
            for with_var in (False, True):
                assert E.build_window_need(n, L, with_var) == py_need(n, L, with_var)
                lo, hi = py_need(n, 1, with_var), py_need(n, L, with_var)
                budgets = {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1, 2 * hi, (lo + hi) // 2, (3 * lo + hi) // 4, py_need(n, min(L, 256), with_var), py_need(n, min(L, 256), with_var) - 1,
                           py_need(n, min(L, 300), with_var), 288 * 10 ** 9}
                for budget in sorted(budgets):
                    want = py_plan(n, L, with_var, budget)
                    if want == 0:
                        with pytest.raises(E.EngineError) as ei:
                            E.build_window_plan(n, L, with_var, budget)
                        assert "error -4" in str(ei.value) and str(lo) in str(ei.value) and str(budget) in str(ei.value), str(ei.value)
                        continue
                    W, need = E.build_window_plan(n, L, with_var, budget)
                    assert 1 <= W <= L and need == py_need(n, W, with_var) and need <= budget, (n, L, with_var, budget, W)
                    adm = admissible(L)
                    nxt = adm.index(W) + 1                                      # W is admissible: below 256, or a multiple of 256
                    assert W < 256 or W % 256 == 0
                    assert nxt == len(adm) or py_need(n, adm[nxt], with_var) > budget, (n, L, with_var, budget, W)
                    assert W == want
                    cases += 1
    assert cases > 500


# ============================================================================= GPU
def _build(tmp, name, args):
    r = run_build(args + ["-n", name, "-v"], tmp)
    assert r.returncode == 0, r.stderr
    ll = [x for x in r.stderr.split("\n") if x.startswith("Final Tree log-liklihood: ")]
    assert len(ll) == 1, r.stderr
    return str(tmp / (name + ".ptu")), ll[0], r.stderr


@pytest.mark.gpu
def test_hand_tree_windows_equal_the_resident_build(hand_inputs):
    need_gpu()
    tmp, fa, tr = hand_inputs
    args = [fa, tr, "--no-hmm", "-sm", sm("GTR"), "-r", "other"]
    base, ll, err = _build(tmp, "res", args)
    assert "column windows" not in err
    L = E.parse_files(None, base)["L"]
    assert 280 <= L < 300
    for W in (1, 7, 257, L - 1, L + 5):
        p, l2, err = _build(tmp, "w%d" % W, args + ["--col-window", W])
        assert filecmp.cmp(base, p, shallow=False), W
        assert l2 == ll, (W, l2, ll)
        if W < L:
            assert "Building in %d column windows of %d columns" % (-(-L // W), W) in err, err
        else:
            assert "column windows" not in err                                    # W >= L: the resident path


@pytest.fixture(scope="module")
def resident70(tmp_path_factory):
    """the resident builds of 70_otus the windowed ones are compared with, one per set of options"""
    tmp = tmp_path_factory.mktemp("resident70")
    made = {}

    def get(model, *extra):
        key = (model,) + extra
        if key not in made:
            made[key] = _build(tmp, "res%d" % len(made), [FASTA70, TREE70, "--no-hmm", "-sm", sm(model), "-a", TAX70] + list(extra))
        return made[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("model,extra,W,n_win", [("JC69", (), 256, 6), ("GTR", ("-V", "-k", "4"), 743, 2)])
def test_70otus_windows_equal_the_resident_build(tmp_path, resident70, model, extra, W, n_win):
    need_gpu()
    base, ll, berr = resident70(model, *extra)
    p, l2, err = _build(tmp_path, "win", [FASTA70, TREE70, "--no-hmm", "-sm", sm(model), "-a", TAX70, "--col-window", W] + list(extra))
    assert "Building in %d column windows of %d columns" % (n_win, W) in err, err
    assert 1486 - (n_win - 1) * W in range(1, W + 1)
    assert filecmp.cmp(base, p, shallow=False)
    assert l2 == ll
    if extra:
        alpha = [x for x in err.split("\n") if x.startswith("Estimated alpha = ")]
        assert len(alpha) == 1 and alpha[0] in berr and "Re-evaluating Phylogenetic Tree at all 249 nodes" in err


@pytest.mark.gpu
def test_70otus_auto_width_under_mem(tmp_path, resident70):
    need_gpu()
    n, L = 249, 1486
    budget = py_need(n, 300, False) + 1000                    # room for 300 columns: the chooser rounds to 256, six windows
    W = py_plan(n, L, False, budget)
    n_win = -(-L // W)
    assert W == 256 and 3 <= n_win <= 8
    base, ll, _ = resident70("JC69")
    p, l2, err = _build(tmp_path, "auto", [FASTA70, TREE70, "--no-hmm", "-sm", sm("JC69"), "-a", TAX70, "--col-window", "auto", "--mem", "%.9f" % (budget / 1e9)])
    assert "Building in %d column windows of %d columns" % (n_win, W) in err, err
    assert filecmp.cmp(base, p, shallow=False) and l2 == ll
    # auto with room for everything: the resident path
    p, l2, err = _build(tmp_path, "roomy", [FASTA70, TREE70, "--no-hmm", "-sm", sm("JC69"), "-a", TAX70, "--col-window", "auto", "--mem", "1"])
    assert "column windows" not in err and filecmp.cmp(base, p, shallow=False) and l2 == ll
    # not even one column: one line, no file
    r = run_build([FASTA70, TREE70, "--no-hmm", "-sm", sm("JC69"), "-n", "tiny", "--col-window", "auto", "--mem", "%.9f" % ((py_need(n, 1, False) - 1000) / 1e9)], tmp_path)
    assert r.returncode != 0 and len(r.stderr.strip().split("\n")) == 1 and "one column of 249 nodes needs" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "tiny.ptu")
    # a given width beyond --mem
    r = run_build([FASTA70, TREE70, "--no-hmm", "-sm", sm("JC69"), "-n", "tiny", "--col-window", "512", "--mem", "%.9f" % (budget / 1e9)], tmp_path)
    assert r.returncode != 0 and len(r.stderr.strip().split("\n")) == 1 and "windows of 512 columns need" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "tiny.ptu")


@pytest.fixture(scope="module")
def swept70():
    """70_otus under GTR with 4 rate categories: one hu_tree_evaluate call, kept on the device for the tests below"""
    import torch
    db = synth.make_db_70otus("GTR")
    rates = E.dg_model(4, 1.66)[1]
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, rates)
    leaf_only = np.where(db.is_leaf[:, None], db.seq, 0).astype(np.int8)
    n, L = leaf_only.shape
    up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    seq, h = E.tree_evaluate(db.parent, db.blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()
    return db, md, leaf_only, up, down, seq, h


@pytest.mark.gpu
def test_sweep_windows_equal_tree_evaluate(swept70):
    need_gpu()
    import torch
    db, md, leaf_only, up, down, seq, h = swept70
    n, L = leaf_only.shape
    assert (n, L) == (249, 1486)
    wins = [(0, 700), (700, 786)]
    s = E.TreeSweep(db.parent, db.blen, L)
    assert np.array_equal(s.heights(), h)
    # both sweeps
    got = leaf_only.copy()
    for a, wl in wins:
        wu = torch.full((n, wl, 4), 7.0, dtype=torch.float64, device="cuda:0"); wd = torch.full_like(wu, 7.0)
        s.window(got, md, a, wl, wu.data_ptr(), wd.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(wu.view(torch.int64), up[:, a:a + wl].contiguous().view(torch.int64))             # bit-equal, -inf and signs included
        assert torch.equal(wd[1:].view(torch.int64), down[1:, a:a + wl].contiguous().view(torch.int64))       # down[root] is written by nobody
        assert bool((wd[0] == 7.0).all())
        assert np.array_equal(got[:, a:a + wl], seq[:, a:a + wl])
        if a == 0:
            assert np.array_equal(got[:, wl:], leaf_only[:, wl:])                                            # columns outside the window untouched
    assert np.array_equal(got, seq)
    # the post-order levels alone, and the mutation counts joined from the windows
    got = leaf_only.copy()
    cnt = np.zeros(L, np.int32)
    for a, wl in wins:
        wu = torch.full((n, wl, 4), 7.0, dtype=torch.float64, device="cuda:0")
        s.window(got, md, a, wl, wu.data_ptr(), None)
        torch.cuda.synchronize()
        assert torch.equal(wu.view(torch.int64), up[:, a:a + wl].contiguous().view(torch.int64))
        cnt[a:a + wl] = E.tree_count_mutations(db.parent, wl, wu.data_ptr())
    assert np.array_equal(got, seq)
    whole = E.tree_count_mutations(db.parent, L, up.data_ptr())
    assert np.array_equal(cnt, whole) and whole.sum() > 0
    with pytest.raises(E.EngineError):
        s.window(got, md, 1400, 100, up.data_ptr(), None)
    s.close()


@pytest.mark.gpu
def test_windowed_writer_with_device_buffers(tmp_path, swept70):
    need_gpu()
    import torch
    db, md, leaf_only, up, down, seq, h = swept70
    n, L = leaf_only.shape
    off, idx, rows, _, _ = _file_order(db.parent)
    order = dict(child_off=off, child_idx=idx, msa_row_of_leaf=rows)
    kw = dict(names=db.names, annos=db.annos, anno_dist=db.anno_dist)
    b, _ = E.dg_model(4, 1.66)
    tail = dict(model_text=db.model.text, dg_alpha=1.66, dg_breaks=b)
    ref = str(tmp_path / "ref.ptu")
    E.write_ptu_stream(ref, db.parent, db.blen, seq, up.data_ptr(), down.data_ptr(), h, md, msgs_on_device=True, **kw, **tail, **order)
    wins = [(700, 786), (0, 700)]
    # 2 n - 1 = 497 records a window: staging for 100 pieces of the narrower window -> 5 runs there, 6 at the wider one (89 pieces each)
    for k, staging in enumerate((100 * 32 * 700, 1, 0)):
        p = str(tmp_path / ("dev%d.ptu" % k))
        w = E.PtuWriter(p, db.parent, db.blen, L, staging_bytes=staging, **kw, **order)
        for a, wl in wins:
            wu = up[:, a:a + wl].contiguous(); wd = down[:, a:a + wl].contiguous()
            torch.cuda.synchronize()
            w.window(a, wl, wu.data_ptr(), wd.data_ptr(), on_device=True)
        w.close(seq, h, md, **tail)
        assert filecmp.cmp(ref, p, shallow=False), staging
