#!/usr/bin/env python3
"""The reference code's answers for tests/test_ref_seq.py and the `.csfm` of the CLI test's database (tests/test_gpu_parity.py::
test_cli_end_to_end).  Made by oracle/_ref/libref_seq.so and oracle/_ref/csfm_ref (`make -C oracle ref`): the reference's alphabet,
DigitalSeq, PrimarySeq, SeqUtils, ProgEnv and SeqIO behind a C shim (oracle/ref_seq_shim.cpp), and its vendored libcds +
libdivsufsort under a restated CSFMIndex build / save (oracle/csfm_ref.cpp), all compiled from the reference tree where it lies.
The inputs are built by the tests' own functions, so the tests rebuild exactly what the reference code was run on.
Outputs: tests/golden/ref_seq.npz, tests/golden/cli_db.csfm.gz.
Run where the reference tree is; every other machine only reads the committed files."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ref_seq as T          # noqa: E402
import test_gpu_parity as P       # noqa: E402

L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_seq.so"))
L.ref_pdist.restype = C.c_double
L.ref_ptu_head_write.restype = C.c_long
L.ref_ptu_head_write.argtypes = [C.c_long, C.c_int, C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_long]
L.ref_ptu_head_read.restype = C.c_long
L.ref_ptu_head_read.argtypes = [C.c_char_p, C.POINTER(C.c_long), C.POINTER(C.c_int), C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long,
                                C.c_void_p, C.c_void_p]
L.ref_seqio_read.restype = C.c_long
p8 = C.POINTER(C.c_int8)
out = {}


def ragged(name, rows):
    out[name] = np.concatenate([np.asarray(r, np.int8) for r in rows]) if rows else np.zeros(0, np.int8)
    out[name + "_offs"] = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)


# DigitalSeq
ins = T.digitize_inputs()
rows = []
for s in ins:
    buf = np.zeros(len(s) + 1, np.int8)
    n = L.ref_digitize(s.encode(), buf.ctypes.data_as(p8), len(buf))
    rows.append(buf[:n].copy())
out["digitize_in"] = np.array(ins); ragged("digitize", rows)

# SeqUtils::pDist on every node of a tree
db, cases = T.pdist_cases()
out["pdist_q"] = np.stack([q for q, _, _ in cases]); out["pdist_se"] = np.array([(s, e) for _, s, e in cases], np.int32)
out["pdist"] = np.array([[L.ref_pdist(q.ctypes.data_as(p8), np.ascontiguousarray(db.seq[u], np.int8).ctypes.data_as(p8), db.cs_len, s, e)
                          for u in range(db.n_nodes)] for q, s, e in cases])

# PrimarySeq::revcom
def revcom(s):
    buf = C.create_string_buffer(len(s) + 8)
    assert L.ref_revcom(s.encode(), buf, len(buf)) == len(s)
    return buf.value.decode()


ins = T.revcom_inputs(); out["revcom_in"] = np.array(ins); out["revcom"] = np.array([revcom(s) for s in ins])
ins = T.cli_revcom_inputs(); out["cli_revcom_in"] = np.array(ins); out["cli_revcom"] = np.array([revcom(s) for s in ins])

# pDist on the oracle's alignments of the engine test's reads (the engine's alignments are these, bit for bit)
from oracle import oracle_py as O          # noqa: E402
from conftest import oracle_objects        # noqa: E402
db, reads, vps = T.engine_pdist_case()
_, H, _ = oracle_objects(db)
codes, se, pd = [], [], []
for i, r in enumerate(reads):
    a = H.align(r.seq, vps[i])
    q = np.full(db.cs_len, -2, np.int8); dq = O.digitize(a["align"]); q[:len(dq)] = dq
    assert len(dq) == db.cs_len
    s, e = a["csStart"] - 1, a["csEnd"] - 1
    codes.append(q); se.append((s, e))
    pd.append([L.ref_pdist(q.ctypes.data_as(p8), np.ascontiguousarray(db.seq[u], np.int8).ctypes.data_as(p8), db.cs_len, s, e) for u in range(db.n_nodes)])
out["engine_codes"] = np.stack(codes); out["engine_se"] = np.array(se, np.int32); out["engine_pdist"] = np.array(pd)

# the head of a .ptu, both directions
db = T.small_db()
n, cs = db.n_nodes, db.cs_len
with tempfile.TemporaryDirectory() as t:
    p = os.path.join(t, "product.ptu")
    T.write_product_ptu(db, p)
    nn, cl = C.c_long(0), C.c_int(0)
    cd = np.full((n, cs), 99, np.int8); ad = np.zeros(n); sl = np.zeros(n, np.int64)
    names = C.create_string_buffer(1 << 16); annos = C.create_string_buffer(1 << 16)
    off = L.ref_ptu_head_read(p.encode(), C.byref(nn), C.byref(cl), cd.ctypes.data, cd.size, names, len(names), annos, len(annos),
                              ad.ctypes.data, sl.ctypes.data)
    assert off > 0, off
    out["ptu_read_off"] = np.int64(off); out["ptu_read_head"] = np.frombuffer(open(p, "rb").read()[:off], np.uint8)
    out["ptu_read_dims"] = np.array([nn.value, cl.value], np.int64); out["ptu_read_seqlen"] = sl; out["ptu_read_codes"] = cd
    out["ptu_read_anno_dist"] = ad; out["ptu_read_names"] = np.array(names.value.decode()); out["ptu_read_annos"] = np.array(annos.value.decode())
cap = 1 << 20
buf = C.create_string_buffer(cap)
nm = (C.c_char_p * n)(*[s.encode() for s in db.names]); an = (C.c_char_p * n)(*[s.encode() for s in db.annos])
seq = np.ascontiguousarray(db.seq, np.int8); ad = np.ascontiguousarray(db.anno_dist, np.float64)
k = L.ref_ptu_head_write(n, cs, seq.ctypes.data, nm, an, ad.ctypes.data, buf, cap); assert k > 0
out["ptu_written_head"] = np.frombuffer(buf.raw[:k], np.uint8).copy()
seq2 = seq.copy(); seq2[4, :] = -128
k2 = L.ref_ptu_head_write(n, cs, seq2.ctypes.data, nm, an, ad.ctypes.data, buf, cap); assert k2 > 0
out["ptu_written_head_noseq4"] = np.frombuffer(buf.raw[:k2], np.uint8).copy()

# readProgInfo / writeProgInfo
ins = T.prog_info_lines()
out["prog_info_in"] = np.array(ins); out["prog_info"] = np.array([L.ref_read_prog_info(s.encode()) for s in ins], np.int32)
buf = C.create_string_buffer(4096)
assert L.ref_write_prog_info(T.PROG_INFO_WRITTEN.encode(), buf, len(buf)) > 0
out["prog_info_written"] = np.array(buf.value.decode())

# SeqIO
with tempfile.TemporaryDirectory() as t:
    files, _, _ = T.seqio_files(t)
    res = {}
    for name, (fmt, path) in files.items():
        buf = C.create_string_buffer(1 << 20)
        k = L.ref_seqio_read(path.encode(), fmt.encode(), buf, len(buf))
        assert k >= -1, (name, k)
        res[name] = k if k < 0 else [l.split("\x1f") for l in buf.value.decode().split("\n")[:-1]]
    out["seqio"] = np.array(json.dumps(res))

# the .csfm of the CLI test's database: written by the reference's libcds + libdivsufsort from its leaf rows
msa = P.cli_msa_text()
out["cli_msa_sha256"] = np.array(hashlib.sha256(msa.encode()).hexdigest())
with tempfile.TemporaryDirectory() as t:
    fa = os.path.join(t, "msa.fasta"); open(fa, "w").write(msa)
    subprocess.check_call([os.path.join(ROOT, "oracle", "_ref", "csfm_ref"), fa, os.path.join(t, "x.csfm")])
    with open(os.path.join(t, "x.csfm"), "rb") as f, gzip.GzipFile(os.path.join(G, "cli_db.csfm.gz"), "wb", mtime=0) as g:
        g.write(f.read())

np.savez_compressed(os.path.join(G, "ref_seq.npz"), **out)
print("wrote ref_seq.npz (%d bytes) and cli_db.csfm.gz (%d bytes)" % (os.path.getsize(os.path.join(G, "ref_seq.npz")), os.path.getsize(os.path.join(G, "cli_db.csfm.gz"))))
