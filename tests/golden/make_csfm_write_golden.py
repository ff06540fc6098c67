#!/usr/bin/env python3
"""Golden `.csfm` files of four small alignments for the writer's tests (tests/test_csfm_write.py): tests/golden/csfm_write_{a,b,c,d}.fa and
the bytes oracle/_ref/csfm_ref writes for each, csfm_write_{a,b,c,d}.csfm.gz.  csfm_ref (`make -C oracle ref`) is the reference's vendored
libcds and libdivsufsort under a restated CSFMIndex::build / save (oracle/csfm_ref.cpp); it writes no saveProgInfo head and takes csSeq from
unweighted counts.  The 70_otus alignment's file is tests/golden/70_otus.csfm.gz (make_csfm_golden.py).
  a  7 rows x 42 columns: no T anywhere (a padding symbol in the wavelet tree), three identical rows back to back, an all-gap row (two
     adjacent separators), a row with an inner gap run, lower case and N
  b  one row, ACGT-ACGTTTGA (concatLen 13)
  c  40 identical random rows of 300 bases (N = 12,041): common prefixes run across the separators for thousands of symbols
  d  three rows of one column: A, -, C (N = 6)
  70otus_pruned  the 70_otus alignment without the columns that hold no residue (MSA::prune), as hmmufotu-amd-build --csfm indexes it:
     125 rows x 1,486 of the 7,682 columns; only the .csfm.gz is kept, the test prunes the fixture itself
Needs the reference's sources for csfm_ref; the tests read only the committed files."""
import gzip, os, random, subprocess, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, "tests", "golden")

random.seed(23)
same = "".join(random.choice("ACG") for _ in range(42))
a = [same, same, same,
     "-" * 42,
     "".join(random.choice("ACG") for _ in range(12)) + "-" * 17 + "".join(random.choice("ACG") for _ in range(13)),
     "".join(random.choice("acgN") for _ in range(42)),
     "--" + "".join(random.choice("ACGacg-.") for _ in range(38)) + "..", ]
c_row = "".join(random.choice("ACGT") for _ in range(300))
cases = {"a": a, "b": ["ACGT-ACGTTTGA"], "c": [c_row] * 40, "d": ["A", "-", "C"]}
assert all("T" not in r.upper() and "U" not in r.upper() for r in a)
rows70 = []
for l in gzip.open(os.path.join(G, "ref_data", "70_otus.fasta.gz"), "rt"):
    l = l.strip()
    if l.startswith(">"):
        rows70.append("")
    elif rows70:
        rows70[-1] += l
keep = [j for j in range(len(rows70[0])) if any(r[j].upper() in "ACGTUMRWSYKVHDBN" for r in rows70)]
cases["70otus_pruned"] = ["".join(r[j] for j in keep) for r in rows70]
for name, rows in cases.items():
    with tempfile.TemporaryDirectory() as t:
        fa = os.path.join(t, "x.fa") if name == "70otus_pruned" else os.path.join(G, "csfm_write_%s.fa" % name)
        with open(fa, "w") as f:
            for i, r in enumerate(rows):
                f.write(">s%d\n%s\n" % (i, r))
        out = os.path.join(t, "x.csfm")
        subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "csfm_ref"), fa, out])
        raw = open(out, "rb").read()
    with gzip.GzipFile(os.path.join(G, "csfm_write_%s.csfm.gz" % name), "wb", mtime=0) as g:
        g.write(raw)
    print(name, len(rows), "rows x", len(rows[0]), "columns:", len(raw), "bytes")
