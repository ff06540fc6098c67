"""hmmufotu-anneal primer scan rate on a gg_97-scale synthetic database (99,322 leaves, 7,682 CS columns): 4,096 primers, -s 3, -i 0.9.
--quick: no CPU restatement (for the kernel trace run); --out=DIR: where the JSON goes (default profiles/)."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from hmmufotu_amd import engine as E, synth_gpu, synth
quick = "--quick" in sys.argv
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
out = {}
t0 = time.time()
db, up, down = synth_gpu.make_db_gpu(99322, 7682, "GTR", dg_k=0, seed=97, win=(0, 64), device="cuda:0", log=lambda *a: None)
del up, down
n, L = db.seq.shape
up = torch.zeros((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
md = E.model_desc(db.model.type_id, db.model.pi, db.model.par)
D = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, up.data_ptr(), down.data_ptr(), db.height, md, msgs_on_device=True)
out["db"] = dict(nodes=D.n_nodes, leaves=D.num_leaves(), cs_len=D.cs_len, K=D.K, build_s=round(time.time() - t0, 1))
from test_anneal import make_primers, restate_anneal
db.is_leaf = None
primers = make_primers(db, 4096, np.random.default_rng(3))
D.anneal(primers[:64])
torch.cuda.synchronize()
t1 = time.time(); res = D.anneal(primers, identity=0.9, strand=3); t2 = time.time()
out["end_to_end"] = dict(primers=len(primers), s=round(t2 - t1, 4), primers_per_s=round(len(primers) / (t2 - t1), 1),
                         no_alignment=sum(r is None for r in res))
# the scan alone: one aligned batch, hu_anneal_batch timed over repeats
b = E.Batch(D, len(primers)); b.set_reads(primers, None); b.align(E.default_opts(align_mode="global"))
rows = np.arange(len(primers), dtype=np.int32)
rows[[i for i, r in enumerate(b.alignments(want_align=False)["recs"]) if r["status"] != 1]] = -1
b.anneal(rows, 0.1)
reps = 10
t3 = time.time()
for _ in range(reps): b.anneal(rows, 1 - 0.9)
t4 = time.time()
out["scan_call"] = dict(primers=len(primers), ms=round((t4 - t3) / reps * 1e3, 3), primers_per_s=round(len(primers) * reps / (t4 - t3), 1))
b.close()
if not quick:
    from oracle import oracle_py as O
    h = db.hmm
    H = O.Hmm(h.K, h.L, h.EM, h.EI, h.T, h.p2cs, 0)
    idx = list(range(0, 4096, 128))          # 32 primers: oracle alignment + numpy restatement over every node
    t5 = time.time(); want = restate_anneal(H, [primers[i] for i in idx], db.seq, db.parent, 0.9, 3); t6 = time.time()
    out["cpu_restatement"] = dict(primers=len(idx), s=round(t6 - t5, 3), primers_per_s=round(len(idx) / (t6 - t5), 2))
    bad = [i for i, w in zip(idx, want) if res[i] != w]
    out["parity_at_scale"] = dict(checked=len(idx), mismatched=bad)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "anneal_rate%s.json" % ("_quick" if quick else "")), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
sys.exit(1 if out.get("parity_at_scale", {}).get("mismatched") else 0)
