"""Seconds per phase of hmmufotu-amd-tree --support on one device: a random binary tree of n = 4,096 leaves
(--n=..., comma separated; 2 n - 1 nodes), rows evolved by `synth` down it (JC69, mean branch 0.05, 5 % of the cells turned into gaps),
7,682 columns as gg_97 has them, the HKY85 model of the golden files, the true lengths, B = 1,000 replicates (--replicates).  The phases
are those of hu_support_timing, host clock around calls that end in a synchronise: the sweep up and down (with a sweep handle of its
own, which also sends the rows), the scoring (k_nni_score and the copies of its results), the weights (the table's allocation, its
zeroing and k_support_weights) and the supports (k_nni_support, the copies of its results).  Phase B of the support kernel reads the
table once per edge, 2 bytes per edge, column and replicate; that count is held against the whole phase.  The second call is the one
recorded: the first pays for loading the code objects.  --host=1 runs the same call on the library's host path for scale, one thread.
--out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
NS = [int(x) for x in arg("n", "4096").split(",")]
L, B, HOST = int(arg("columns", 7682)), int(arg("replicates", 1000)), int(arg("host", 1))
if E.device_count() < 1:
    sys.exit("support_rate: no gfx950 device")
m = synth.load_model("HKY85")
md = E.model_desc(m.type_id, m.pi, m.par)
out = {"columns": L, "replicates": B, "pairs_in_lds": L <= E.SUPPORT_LDS_COLS}


def write():
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "support_rate.json"), "w") as f:
        json.dump(out, f, indent=1)


def record(r, call):
    s = r["seconds"]
    edges = len(r["edge_node"])
    table = 2 * edges * L * B
    return dict(call_s=round(call, 3), eligible_edges=edges, skipped=r["skipped"], sweep_s=round(s["sweep"], 4), score_s=round(s["score"], 4),
                weights_s=round(s["weights"], 4), support_s=round(s["support"], 4), table_bytes_read=table,
                table_bytes_per_s_of_the_support_phase=table / s["support"] if s["support"] > 0 else None,
                mean_support=float(np.mean(r["support"])) if edges else None, edges_with_full_support=int(np.sum(r["count"] == B)),
                edges_without_support=int(np.sum(r["count"] == 0)))


for n in NS:
    rng = np.random.default_rng(97 + n)
    parent, blen, is_leaf = synth.make_tree(n, rng)
    seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
    seq[rng.random(seq.shape) < 0.05] = -2
    seq[~is_leaf] = -2
    nodes = len(parent)
    bl = np.where(parent >= 0, blen, 0.0)
    rec = dict(nodes=nodes, need_bytes=E.support_need(nodes, L, B), table_bytes=2 * ((B + 3) // 4 * 4) * L)
    dev = None
    for _ in range(2):
        t0 = time.perf_counter()
        dev = E.tree_nni_support(parent, bl, seq, md, replicates=B)
        call = time.perf_counter() - t0
    rec["device"] = record(dev, call)
    out["n_%d" % n] = rec
    print(n, rec, flush=True)
    write()
    if HOST:
        t0 = time.perf_counter()
        host = E.tree_nni_support(parent, bl, seq, md, replicates=B, host=True)
        rec["host_path"] = record(host, time.perf_counter() - t0)
        rec["edges_whose_count_differs_between_the_two"] = int(np.sum(host["count"] != dev["count"]))
        print(n, rec["host_path"], flush=True)
        write()
    del seq
