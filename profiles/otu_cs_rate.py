"""OTU consensus rates at gg_97 scale: 7,682 CS columns, 1,048,576 accepted rows in batches of 8,192 over about 20,000 OTUs
with a Zipf share (a few OTUs hold most reads), on a synthetic database of 10,001 leaves (20,001 nodes: every node can be an OTU).
Reports ms per hu_otucs_add (rows cut to their spans, and the same rows with a symbol at both ends so that whole rows cross the bus), the
bytes staged, hu_otucs_infer over 4,096 OTUs, and the reference's loop restated in C++ on one host core (profiles/otu_cs_baseline.cpp).
The split of a call into copy and kernel comes from a run of this script under rocprofv3 --kernel-trace --memory-copy-trace --stats with --quick
(64 batches, no host baseline).  --out=DIR: where the JSON goes (default profiles/)."""
import ctypes as C, json, os, subprocess, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth_gpu
quick = "--quick" in sys.argv
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
L, BATCH, N_ROWS, N_OTU, POOL = 7682, 8192, (1 << 19) if quick else (1 << 20), 20000, 8
out = {}
t0 = time.time()
db, up, down = synth_gpu.make_db_gpu(10001, L, "GTR", dg_k=0, seed=97, device="cuda:0", log=lambda *a: None)
md = E.model_desc(db.model.type_id, db.model.pi, db.model.par)
D = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, up.data_ptr(), down.data_ptr(), db.height, md, msgs_on_device=True)
out["db"] = dict(nodes=D.n_nodes, cs_len=D.cs_len, build_s=round(time.time() - t0, 1))
rng = np.random.default_rng(5)
# rows as an aligned 250-base amplicon read looks: '-' everywhere but a stretch of ~1,400 columns, a base in the profile's match columns
p2cs = np.asarray(db.hmm.p2cs)[1:] - 1
pool = np.full((POOL * BATCH, L), ord("-"), np.uint8)
k0 = rng.integers(300, 340, size=len(pool))
for i in range(len(pool)):
    cols = p2cs[k0[i]:k0[i] + 250]
    pool[i, cols] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=len(cols))]
span = np.array([np.nonzero(r != ord("-"))[0][[0, -1]] for r in pool[:BATCH]])
out["rows"] = dict(batch=BATCH, rows=N_ROWS, otus=N_OTU, span_columns_mean=float((span[:, 1] - span[:, 0] + 1).mean()))
w = 1.0 / np.arange(1, N_OTU + 1); w /= w.sum()
otu_nodes = rng.permutation(D.n_nodes)[:N_OTU].astype(np.int32)
nodes = otu_nodes[rng.choice(N_OTU, size=N_ROWS, p=w)]
out["rows"]["share_of_top_10_otus"] = round(float(np.sort(np.bincount(nodes))[::-1][:10].sum() / N_ROWS), 3)


def run(rows_pool, label):
    cs = D.otu_consensus()
    cs.add(nodes[:BATCH], rows_pool[:BATCH])                       # warm-up: buffers, first slots
    cs.close(); cs = D.otu_consensus()
    ts = []
    for b in range(N_ROWS // BATCH):
        r = rows_pool[(b % POOL) * BATCH:(b % POOL + 1) * BATCH]
        t1 = time.perf_counter(); cs.add(nodes[b * BATCH:(b + 1) * BATCH], r); ts.append(time.perf_counter() - t1)
    ts = np.array(ts) * 1e3
    out[label] = dict(calls=len(ts), ms_per_add_median=round(float(np.median(ts)), 3), ms_per_add_mean=round(float(ts.mean()), 3),
                      ms_first_16_mean=round(float(ts[:16].mean()), 3), total_s=round(float(ts.sum()) / 1e3, 3),
                      rows_per_s=round(N_ROWS / (ts.sum() / 1e3), 1))
    return cs


cs = run(pool, "add_spans")
full = pool.copy(); full[:, 0] = ord("."); full[:, L - 1] = ord(".")     # a gap symbol that is not '-': the span is the whole row
cs_full = run(full, "add_whole_rows")
out["add_spans"]["staged_bytes_per_add"] = int(((span[:, 1] | 15) + 1 - (span[:, 0] & ~15)).sum())
out["add_whole_rows"]["staged_bytes_per_add"] = BATCH * ((L + 15) // 16 * 16)
# the counts of the heaviest OTU agree between the two (but for the two end columns) and with a numpy count of its rows
top = int(np.bincount(nodes).argmax())
f1, g1 = cs.counts(top); f2, g2 = cs_full.counts(top)
assert (f1 == f2).all() and (g1[1:-1] == g2[1:-1]).all() and int(f1[:, 5].sum() + g1[5]) == int((nodes == top).sum())
cs_full.close()
kept = np.sort(np.unique(nodes))[:4096].astype(np.int32)
cs.infer(kept[:64])
reps = 5
t1 = time.perf_counter()
for _ in range(reps): seqs = cs.infer(kept, 2.0)
t2 = time.perf_counter()
cells = len(kept) * L
out["infer_call"] = dict(otus=len(kept), ms=round((t2 - t1) / reps * 1e3, 3), bytes_must_move=cells * (32 + 20 + 1),
                         note="the call includes the copy of the symbols to the host and their conversion to str; kernel time: rocprofv3 run")
if not quick:
    so = os.path.join(OUT if os.access(OUT, os.W_OK) else "/tmp", "otu_cs_baseline.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "profiles", "otu_cs_baseline.cpp")])
    lib = C.CDLL(so)
    nb = 4 * BATCH
    uniq, slot = np.unique(nodes[:nb], return_inverse=True)
    slot = slot.astype(np.int32)
    freq = np.zeros((len(uniq), L, 4)); gap = np.zeros((len(uniq), L))
    enc = E.msa_encode_table()
    rows = np.ascontiguousarray(pool[:nb])
    t1 = time.perf_counter()
    lib.otu_cs_baseline(C.c_int64(nb), C.c_int64(L), slot.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), enc.ctypes.data_as(C.c_void_p),
                        freq.ctypes.data_as(C.c_void_p), gap.ctypes.data_as(C.c_void_p))
    t2 = time.perf_counter()
    out["host_loop_one_core"] = dict(rows=nb, s=round(t2 - t1, 3), ms_per_8192_rows=round((t2 - t1) / 4 * 1e3, 2), rows_per_s=round(nb / (t2 - t1), 1))
    cs2 = D.otu_consensus(); cs2.add(nodes[:nb], rows)
    bad = 0
    for k in range(0, len(uniq), max(1, len(uniq) // 50)):
        f, g = cs2.counts(int(uniq[k]))
        bad += int(not ((f.T == freq[k]).all() and (g == gap[k]).all()))
    out["host_loop_one_core"]["otus_differing_from_device"] = bad
    cs2.close()
cs.close()
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "otu_cs_rate%s.json" % ("_quick" if quick else "")), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
sys.exit(1 if out.get("host_loop_one_core", {}).get("otus_differing_from_device") else 0)
