"""hmmufotu-amd-otu-cs / hu_otucs_* / Database.otu_consensus(): the OTU consensus sequences of hmmufotu-sum -c
(src/hmmufotu-sum.cpp:337-458, PTUnrooted::inferPostCS src/PhyloTreeUnrooted.cpp:1111-1125).

CPU: the program's option checks (they run before the device is touched) and the description string of a FASTA record.
GPU: the column counts against the restated loop of the reference (tests/tsv_consumers.sum_otus, and the same loop in numpy on
generated rows), and the consensus symbols against a numpy restatement of inferPostCS written here from db.up, the raw log
messages of the synthetic database — nothing the library computed.  Where the restatement's two largest posterior values agree
to 1e-12 relative the arithmetic decides (a tie, as in oracle/parity.py): there the device's symbol must be one of the two, the
cells so excused are counted, and more than 0.5 % of the called cells fails the test."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsv_consumers as C  # noqa: E402
from conftest import get_db  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
FA, FB = os.path.join(GOLD, "cli_sampleA.tsv"), os.path.join(GOLD, "cli_sampleB.tsv")
TIE_REL = 1e-12
EXCUSE_CAP = 0.005


def _bin(name):
    p = os.path.join(HERE, "..", "hmmufotu_amd", "bin", name)
    assert os.path.exists(p), name + " missing: run __graft_entry__.build()"
    return os.path.abspath(p)


def _run(args, **kw):
    return subprocess.run(args, capture_output=True, text=True, timeout=300, **kw)


# ------------------------------------------------------------------------------------------------ restatements
def _enc_table():
    """step 2 of the reference's loop: b = encode(toupper(c)) of IUPACNucl, from the table tests/tsv_consumers.py restates; bytes
    above 127 are no symbols"""
    t = np.full(256, -1, np.int64)
    for c in range(128):
        t[c] = C._ENC.get(chr(c).upper(), -1)
    return t


def _count_rows(nodes, rows):
    """{node: (freq [4][L], gap [L])} of uint8 rows [n][L]: the loop of src/hmmufotu-sum.cpp:391-397 in numpy"""
    enc = _enc_table()[rows]
    out = {}
    for u in np.unique(nodes):
        e = enc[nodes == u]
        out[int(u)] = (np.stack([(e == b).sum(0) for b in range(4)]), (e < 0).sum(0))
    return out


def _restate_infer(db, node, freq, gap, eff_n):
    """inferPostCS for one node from the raw log message db.up[node]: (symbols [L] of 'ACGT-', post [L][4] sorted descending, called [L])"""
    M = np.asarray(db.up[node], np.float64)
    p = np.exp(M - M.max(1, keepdims=True))
    pri = p / p.sum(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        post = eff_n * pri + freq.T.astype(np.float64)
        post = post / post.sum(1, keepdims=True)
    best = np.where(np.isnan(post).any(1), 0, np.argmax(np.nan_to_num(post, nan=-1.0), 1))       # maxCoeff: the first maximum
    called = ~(freq.sum(0) < gap)
    sym = np.where(called, np.frombuffer(b"ACGT", np.uint8)[best], ord("-")).astype(np.uint8)
    return sym, post, called


def _check_consensus(db, got, node, freq, gap, eff_n, tally):
    """got: the device's string for the node.  Adds (called, excused) to tally."""
    sym, post, called = _restate_infer(db, node, freq, gap, eff_n)
    g = np.frombuffer(got.encode(), np.uint8)
    assert len(g) == db.cs_len
    assert ((g == ord("-")) == ~called).all(), "gap rule differs at node %d" % node
    diff = np.nonzero((g != sym) & called)[0]
    if eff_n == 0:
        assert len(diff) == 0, "effN = 0 is integer arithmetic: node %d differs at columns %s" % (node, diff[:10])
    for j in diff:
        order = np.argsort(-post[j], kind="stable")
        a, b = post[j][order[0]], post[j][order[1]]
        assert abs(a - b) <= TIE_REL * abs(a), "node %d column %d: %r vs %r, post %s" % (node, j, chr(g[j]), chr(sym[j]), post[j])
        assert chr(g[j]) in ("ACGT"[order[0]], "ACGT"[order[1]]), "node %d column %d: %r is neither of the tying symbols" % (node, j, chr(g[j]))
    tally[0] += int(called.sum()); tally[1] += len(diff)


def _assert_tally(tally, what):
    print("%s: %d called cells, %d excused as ties of the arithmetic" % (what, tally[0], tally[1]))
    assert tally[0] > 0 and tally[1] <= EXCUSE_CAP * tally[0], "%s: %d of %d called cells excused" % (what, tally[1], tally[0])


def _accepted(texts, min_q=0.0):
    """(nodes, rows as uint8 [n][L], sample of row) of the records hmmufotu-sum accepts (identity filters off)"""
    nodes, rows, smp = [], [], []
    for s, t in enumerate(texts):
        for r in C.scan(t)[1]:
            if C.c_atol(r["taxon_id"]) >= 0 and C.c_atof(r["Q_taxon"]) >= min_q:
                nodes.append(C.c_atol(r["taxon_id"])); rows.append(r["alignment"].encode("latin1")); smp.append(s)
    return np.array(nodes, np.int32), np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1), np.array(smp)


def _retarget(text, targets, tag):
    """a third sample: the records of an assignment file with their taxon_id rewritten to the given nodes in turn (Q_taxon kept)"""
    lines = text.split("\n")
    out, k, hdr = [], 0, None
    for ln in lines:
        if hdr is None or ln == "":
            out.append(ln)
            if ln and not ln.startswith("#"):
                hdr = ln.split("\t")
            continue
        f = ln.split("\t")
        if C.c_atol(f[hdr.index("taxon_id")]) >= 0:
            f[hdr.index("taxon_id")] = str(targets[k % len(targets)]); k += 1
        f[hdr.index("id")] = tag + f[hdr.index("id")]
        out.append("\t".join(f))
    return "\n".join(out)


def _golden_db(tmp_path):
    from hmmufotu_amd import synth
    db = get_db(120, 700, "GTR", dg_k=4)
    pre = str(tmp_path / "db")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    return db, pre


def _special_nodes(db):
    leaf = int(np.nonzero(db.is_leaf)[0][3])
    inner = int(np.nonzero(~np.asarray(db.is_leaf))[0][5])
    assert inner != 0
    return [0, leaf, inner]


# ------------------------------------------------------------------------------------------------ CPU
def test_cli_option_checks_run_without_a_device(tmp_path):
    exe = _bin("hmmufotu-amd-otu-cs")
    out = str(tmp_path / "cs.fasta")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")          # no device, wherever this runs
    p = _run([exe, "--help"], env=env)
    assert p.returncode == 0 and "-c  FILE" in p.stderr and "--no-gap" in p.stderr
    for args, msg in (
            (["db", FA], "-c must be specified"),
            (["db", FA, "-c", out, "-e", "-1"], "-e|--effN must be non-negative"),
            (["db", FA, "-c", out, "--effN", "nan"], "-e|--effN must be non-negative"),
            (["db", FA, "-c", out, "-n", "-1"], "-n must be non-negative integer"),
            (["db", FA, "-c", out, "-s", "-2"], "-s must be non-negative integer"),
            (["db", FA, "-c", out, "--frobnicate"], "unknown option --frobnicate"),
            (["db", str(tmp_path / "absent.tsv"), "-c", out], "Unable to open assignment input file"),
            (["db", "-c", out], "Usage:")):
        p = _run([exe] + args, env=env)
        assert p.returncode != 0 and msg in p.stderr, (args, p.returncode, p.stderr)
    bad = str(tmp_path / "bad.tsv"); open(bad, "w").write("# hmmufotu_amd v0.1.0 x\nid\ttaxon_id\n")
    p = _run([exe, "db", bad, "-c", out], env=env)
    assert p.returncode != 0 and "Not an valid input file" in p.stderr


def test_description_of_a_record():
    from hmmufotu_amd import engine as E
    d = E.otucs_description("gg_97", "k__Bacteria;p__Firmicutes", 0.0, 12, 2)
    assert d == 'DBName=gg_97;Taxonomy="k__Bacteria;p__Firmicutes";AnnoDist=0;ReadCount=12;SampleHits=2'
    for v, txt in ((0.0, "0"), (0.1, "0.10000000000000001"), (1e-5, "1.0000000000000001e-05"), (3.0, "3")):
        assert txt == "%.17g" % v
        assert E.otucs_description("d", "t", v, 1, 1) == 'DBName=d;Taxonomy="t";AnnoDist=%s;ReadCount=1;SampleHits=1' % txt
    tax = "k__Bacteria; p__ Candidatus X; s__a b;Other"
    d = E.otucs_description("/data/my db", tax, 0.25, 1048576, 31)
    assert d == 'DBName=/data/my db;Taxonomy="%s";AnnoDist=0.25;ReadCount=1048576;SampleHits=31' % tax
    assert E.otucs_description("d", "", 1.0, 0, 0) == 'DBName=d;Taxonomy="";AnnoDist=1;ReadCount=0;SampleHits=0'


# ------------------------------------------------------------------------------------------------ GPU
def _rng_rows(rng, n, L, alphabet):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), size=(n, L))]


def _amplicon_rows(rng, n, L, alphabet):
    """rows of '-' with a stretch of symbols, as an aligned read looks"""
    rows = np.full((n, L), ord("-"), np.uint8)
    for i in range(n):
        a = int(rng.integers(0, L - 40)); b = int(min(L, a + rng.integers(20, 400)))
        rows[i, a:b] = _rng_rows(rng, 1, b - a, alphabet)[0]
    return rows


def _assert_counts(cs, want, L):
    for u, (f, g) in want.items():
        gf, gg = cs.counts(u)
        assert gf.shape == (4, L) and gg.shape == (L,)
        assert (gf == f).all() and (gg == g).all(), "counts of node %d differ" % u


@pytest.mark.gpu
def test_counts_of_the_committed_assignment_files():
    from hmmufotu_amd import engine as E
    db = get_db(120, 700, "GTR", dg_k=4)
    texts = [open(FA).read(), open(FB).read()]
    want = C.sum_otus(texts, db.cs_len)
    assert len(want) == 34
    D = E.Database.from_synth(db)
    cs = D.otu_consensus()
    nodes, rows, _ = _accepted(texts)
    cs.add(nodes, rows)
    for u, o in want.items():
        f, g = cs.counts(u)
        assert (f == np.array(o["freq"])).all() and (g == np.array(o["gap"])).all(), u
    f, g = cs.counts(int(max(want)) + 1 if int(max(want)) + 1 not in want else 1)
    assert not f.any() and not g.any()                                                     # a node no row has named
    cs.close(); D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L", [700, 1333])
def test_counts_of_generated_rows(L):
    """a heavy OTU beside hundreds of single-row OTUs; lower case, IUPAC, '.', '_' and invalid bytes; bases at both ends of a row, an
    all-gap row, a row of '.', a row of invalid bytes; L no multiple of 64 (nor of 16); and the same rows in uneven pieces"""
    from hmmufotu_amd import engine as E
    db = get_db(200, L, "GTR", dg_k=4)
    assert db.n_nodes >= 320 and L % 16 != 0
    rng = np.random.default_rng(L)
    alpha = b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn-._?*0 \x00\x7f\x80\xc1\xe1\xff"
    heavy = 17
    nodes = np.concatenate([np.full(5000, heavy), np.arange(20, 320), np.full(6, 7)]).astype(np.int32)
    rows = np.concatenate([_amplicon_rows(rng, 5000, L, b"ACGTacgtNRY-."), _amplicon_rows(rng, 150, L, alpha), _rng_rows(rng, 150, L, alpha),
                           np.full((6, L), ord("-"), np.uint8)])
    sp = rows[-6:]
    sp[0, 0] = ord("A"); sp[0, L - 1] = ord("t")                 # bases at both ends: outside any nominal region
    sp[1, L - 1] = ord("G")                                      # the last column alone
    # sp[2] stays all '-'
    sp[3, :] = ord(".")
    sp[4, :] = np.frombuffer(b"?\xff", np.uint8)[np.arange(L) % 2]
    sp[5, L // 2] = ord("_")                                     # a lone gap symbol that is not '-'
    perm = rng.permutation(len(nodes))
    nodes, rows = nodes[perm], np.ascontiguousarray(rows[perm])
    want = _count_rows(nodes, rows)
    assert want[heavy][0].sum() + want[heavy][1].sum() == 5000 * L
    D = E.Database.from_synth(db)
    one = D.otu_consensus(); one.add(nodes, rows)
    _assert_counts(one, want, L)
    many = D.otu_consensus()                                     # a second handle on the same database, fed in uneven pieces
    cuts = [0, 1, 2, 66, 67, 1500, 1501, 4000, len(nodes)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        many.add(nodes[a:b], rows[a:b])
    many.add(np.zeros(0, np.int32), np.zeros((0, L), np.uint8))
    _assert_counts(many, want, L)
    _assert_counts(one, want, L)                                 # untouched by the other handle
    one.close(); many.close(); D.close()


def _consensus_inputs(db):
    """the committed files' records, and the same records once more spread over node 0, a leaf and an inner node"""
    texts = [open(FA).read(), open(FB).read()]
    texts.append(_retarget(texts[0], _special_nodes(db), "x_"))
    return texts


@pytest.mark.gpu
def test_consensus_against_the_restatement():
    from hmmufotu_amd import engine as E
    db = get_db(120, 700, "GTR", dg_k=4)
    nodes, rows, _ = _accepted(_consensus_inputs(db))
    want = _count_rows(nodes, rows)
    otus = sorted(want)
    assert set(_special_nodes(db)) <= set(otus) and len(otus) >= 34
    D = E.Database.from_synth(db)
    cs = D.otu_consensus(); cs.add(nodes, rows)
    for eff_n in (0.0, 0.5, 2.0, 50.0):
        got = cs.infer(otus, eff_n)
        tally = [0, 0]
        for u, s in zip(otus, got):
            _check_consensus(db, s, u, want[u][0], want[u][1], eff_n, tally)
        _assert_tally(tally, "effN %g" % eff_n)
        if eff_n == 0:
            assert tally[1] == 0
    # an OTU without rows: no counts, so the prior alone decides and nothing is a gap
    free = next(u for u in range(1, db.n_nodes) if u not in want)
    tally = [0, 0]
    _check_consensus(db, cs.infer([free], 2.0)[0], free, np.zeros((4, db.cs_len), np.int64), np.zeros(db.cs_len, np.int64), 2.0, tally)
    _assert_tally(tally, "an OTU without rows")
    assert cs.infer([], 2.0) == []
    cs.close(); D.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["JC69", "GTR"])
def test_consensus_on_the_70_otus_database(model, tmp_path):
    """a second database (the reference's fixture, tests/golden/ref_data): reads assigned by hmmufotu-amd here, their consensus against
    the restatement.  Under JC69 an all-gap subtree gives four equal prior weights: the first-maximum rule."""
    from hmmufotu_amd import engine as E, synth
    db = synth.make_db_70otus(model)
    pre = str(tmp_path / "otus70")
    synth.write_hmm(db.hmm, pre + ".hmm"); synth.write_ptu(db, pre + ".ptu")
    rng = np.random.default_rng(5)
    reads = synth.simulate_reads(db, 300, 150, rng, mean_cols=500, sd_cols=30)
    fa = str(tmp_path / "reads.fasta")
    with open(fa, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r.seq))
    p = _run([_bin("hmmufotu-amd"), pre, fa, "-s", "1"])
    assert p.returncode == 0, p.stderr
    nodes, rows, _ = _accepted([p.stdout])
    assert len(nodes) >= 200 and rows.shape[1] == db.cs_len
    want = _count_rows(nodes, rows)
    otus = sorted(want)
    D = E.Database.load(pre + ".hmm", pre + ".ptu")
    cs = D.otu_consensus(); cs.add(nodes, rows)
    _assert_counts(cs, want, db.cs_len)
    for eff_n in (0.0, 2.0):
        tally = [0, 0]
        for u, s in zip(otus, cs.infer(otus, eff_n)):
            _check_consensus(db, s, u, want[u][0], want[u][1], eff_n, tally)
        _assert_tally(tally, "70_otus %s effN %g" % (model, eff_n))
    if model == "JC69":                                          # columns where the whole subtree of a node is gaps: equal weights, 'A' first
        M = np.asarray(db.up)
        flat = [(u, j) for u in range(db.n_nodes) for j in np.nonzero((M[u] == M[u][:, :1]).all(1))[0][:3]][:200]
        assert flat, "the fixture has all-gap subtrees"
        us = sorted(set(u for u, _ in flat) - set(otus))
        zero4, zero = np.zeros((4, db.cs_len), np.int64), np.zeros(db.cs_len, np.int64)
        tally = [0, 0]
        for u, s in zip(us, cs.infer(us, 2.0)):
            _check_consensus(db, s, u, zero4, zero, 2.0, tally)
        _assert_tally(tally, "70_otus JC69 prior alone")
    cs.close(); D.close()


def _read_fasta(path):
    recs, lines = [], open(path).read().split("\n")
    assert lines[-1] == ""
    for ln in lines[:-1]:
        if ln.startswith(">"):
            head, _, desc = ln[1:].partition(" ")
            recs.append([head, desc, []])
        else:
            assert recs and 0 < len(ln) <= 60
            recs[-1][2].append(ln)
    for r in recs:
        assert all(len(x) == 60 for x in r[2][:-1])              # every line but the last is full
    return [(h, d, "".join(s)) for h, d, s in recs]


@pytest.mark.gpu
def test_cli_end_to_end(tmp_path):
    import re
    from hmmufotu_amd import engine as E
    db, pre = _golden_db(tmp_path)
    texts = _consensus_inputs(db)
    fz = str(tmp_path / "a.tsv.gz")
    with gzip.open(fz, "wb") as fo:
        fo.write(texts[0].encode())
    fx = str(tmp_path / "x.tsv"); open(fx, "w").write(texts[2])
    lst = str(tmp_path / "samples.txt")
    open(lst, "w").write("gut\t%s\nskin\t%s\nsoil\t%s\n" % (fz, FB, fx))
    D = E.Database.load(pre + ".hmm", pre + ".ptu")
    for flt, min_q, min_n, min_s in ((["-q", "3", "-n", "2", "-s", "2"], 3.0, 2, 2), ([], 0.0, 0, 0)):
        common = [pre, fz, FB, fx, "-l", lst, "--use-dbname"] + flt
        tab = str(tmp_path / "otu.txt")
        p = _run([_bin("hmmufotu-amd-sum")] + common + ["-o", tab])
        assert p.returncode == 0, p.stderr
        table = [l.split("\t") for l in open(tab).read().split("\n")[2:] if l]
        out, out_ng = str(tmp_path / "cs.fasta"), str(tmp_path / "cs_nogap.fasta")
        p = _run([_bin("hmmufotu-amd-otu-cs")] + common + ["-c", out, "--batch", "7"])
        assert p.returncode == 0, p.stderr
        p = _run([_bin("hmmufotu-amd-otu-cs")] + common + ["-c", out_ng, "--no-gap", "-v"])
        assert p.returncode == 0, p.stderr
        recs, recs_ng = _read_fasta(out), _read_fasta(out_ng)
        assert [r[0] for r in recs] == [t[0] for t in table] and len(recs) > 0          # the table's rows, in its order
        nodes, rows, smp = _accepted(texts, min_q)
        cs = D.otu_consensus(); cs.add(nodes, rows)
        kept = [int(t[0][len(pre) + 1:]) for t in table]
        if not flt:                                              # unfiltered: node 0, the leaf and the inner node of the third sample are OTUs
            assert set(_special_nodes(db)) <= set(kept)
        seqs = cs.infer(kept, 2.0)
        for (head, desc, seq), (h2, d2, s2), t, u, want in zip(recs, recs_ng, table, kept, seqs):
            m = re.fullmatch(r'DBName=(.*);Taxonomy="(.*)";AnnoDist=([^;]*);ReadCount=(\d+);SampleHits=(\d+)', desc)
            assert m, desc
            cnt = [int(x) for x in t[1:4]]
            assert m.group(1) == pre and m.group(2) == db.annos[u] == t[4] and m.group(3) == "%.17g" % db.anno_dist[u]
            assert int(m.group(4)) == sum(cnt) and int(m.group(5)) == sum(c > 0 for c in cnt)
            assert sum(cnt) >= min_n and int(m.group(5)) >= min_s
            assert seq == want and len(seq) == db.cs_len and set(seq) <= set("ACGT-")
            assert (h2, d2) == (head, desc) and s2 == seq.replace("-", "")
        cs.close()
    # -e reaches the inference
    out0 = str(tmp_path / "cs0.fasta")
    p = _run([_bin("hmmufotu-amd-otu-cs"), pre, FA, FB, "-c", out0, "-e", "0"])
    assert p.returncode == 0, p.stderr
    nodes, rows, _ = _accepted(texts[:2])
    cs = D.otu_consensus(); cs.add(nodes, rows)
    r0 = _read_fasta(out0)
    assert [int(r[0]) for r in r0] == sorted(set(nodes.tolist())) and [r[2] for r in r0] == cs.infer(sorted(set(nodes.tolist())), 0.0)
    cs.close()
    # a record that cannot be counted names its read and ends the program with an error
    lines = texts[0].split("\n")
    hdr = next(l for l in lines if l and not l.startswith("#")).split("\t")
    k = next(i for i, l in enumerate(lines) if l and not l.startswith("#") and l.split("\t") != hdr and C.c_atol(l.split("\t")[hdr.index("taxon_id")]) >= 0)
    f = lines[k].split("\t")
    short = list(f); short[hdr.index("alignment")] = short[hdr.index("alignment")][:-1]
    far = list(f); far[hdr.index("taxon_id")] = str(db.n_nodes)
    for rec, msg in ((short, "columns"), (far, "is not a node of")):
        fbad = str(tmp_path / "bad.tsv"); open(fbad, "w").write("\n".join(lines[:k] + ["\t".join(rec)] + lines[k + 1:]))
        p = _run([_bin("hmmufotu-amd-otu-cs"), pre, fbad, "-c", str(tmp_path / "none.fasta")])
        assert p.returncode not in (0, -6, -11) and p.returncode > 0 and msg in p.stderr and f[hdr.index("id")] in p.stderr, (p.returncode, p.stderr)
    D.close()


@pytest.mark.gpu
def test_refusals_leave_the_process_and_the_counts_intact():
    from hmmufotu_amd import engine as E
    db = get_db(120, 700, "GTR", dg_k=4)
    L = db.cs_len
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    W = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, db.up[:, 100:400], db.down[:, 100:400], db.height, md, db.anno_id, db.anno_dist,
                               win_start=100, win_len=300)
    with pytest.raises(E.EngineError, match="column window"):
        W.otu_consensus()
    W.close()
    D = E.Database.from_synth(db)
    cs = D.otu_consensus()
    rows = np.full((3, L), ord("-"), np.uint8); rows[:, 10:200] = ord("C")
    cs.add([4, 4, 9], rows)
    for bad in (db.n_nodes, -1, 1 << 30):
        with pytest.raises(E.EngineError, match="names node"):
            cs.add([4, bad, 9], rows)
        with pytest.raises(E.EngineError, match="names node"):
            cs.infer([0, bad], 2.0)
        with pytest.raises(E.EngineError, match="node"):
            cs.counts(bad)
    with pytest.raises(E.EngineError, match="columns"):
        cs.add([4], [b"-" * (L - 1)])
    with pytest.raises(E.EngineError, match="rows must be"):
        cs.add([4], np.zeros((1, L + 1), np.uint8))
    with pytest.raises(E.EngineError, match="eff_n"):
        cs.infer([4], -1.0)
    # a refused call changed nothing, not even the slot of a node it would have seen first
    with pytest.raises(E.EngineError):
        cs.add([11, db.n_nodes], rows[:2])
    f, g = cs.counts(11)
    assert not f.any() and not g.any()
    f, g = cs.counts(4)
    assert (f[1, 10:200] == 2).all() and f.sum() == 2 * 190 and (g[:10] == 2).all() and g.sum() == 2 * (L - 190)
    cs.add([11], rows[:1])
    assert cs.counts(11)[0].sum() == 190 and cs.counts(9)[0].sum() == 190
    assert len(cs.infer([4, 9, 11, 0], 2.0)) == 4
    cs.close(); D.close()
