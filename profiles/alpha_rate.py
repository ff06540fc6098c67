"""Time of hu_alpha on one device.  The workload is one planted table (fixed seed): 256 samples x 4,096 OTUs, 45,000
to 55,000 reads and 300 to 1,500 nonzero cells per sample, 20 depths (i x the largest sample / 20) x 10 repeats, on a tree of 8,001 nodes.
One warm-up call on two samples (the first call loads the code object), then three timed calls: the host clock around the whole call
(it checks the table, walks the tree and builds the plan on the host) and hu_alpha_timing's phases.
The baseline, in the same run, is the only way to the same numbers before hu_alpha: one device hu_otu_subset call per (depth, repeat),
200 calls, the whole table copied back by each, timed twice by the host clock around the loop.  It runs no code of hu_alpha and does
not include the metrics, which a user then had to compute on the host from the 200 tables.
Context: the host path on the first 8 samples, and that its integers and PD bits equal the device's.
--out=FILE: where the JSON goes as well."""
import json, os, sys, time
import numpy as np
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from hmmufotu_amd import engine as E, synth

rng = np.random.default_rng(7)
S, M, N, R = 256, 4096, 50000, 10
parent, blen, is_leaf = synth.make_tree(4001, rng)
n = len(parent)
nodes = rng.choice(n, M, replace=False).astype(np.int32)
counts = np.zeros((M, S))
for j in range(S):
    k = int(rng.integers(300, 1500))
    rows = rng.choice(M, k, replace=False)
    counts[rows, j] = rng.multinomial(int(rng.integers(45000, 55000)), rng.dirichlet(np.full(k, 0.2)))
tot = counts.sum(0)
depths = [int(i * tot.max() / 20) for i in range(1, 21)]
out = dict(samples=S, otus=M, nodes=n, reads_min=int(tot.min()), reads_max=int(tot.max()), nonzero_cells=int((counts > 0).sum()), depths=len(depths), reps=R)
kw = dict(otu_node=nodes, parent=parent, blen=blen, depths=depths, reps=R, seed=1)
E.alpha_diversity(counts[:, :2], otu_node=nodes, parent=parent, blen=blen, depths=depths[:2], reps=1)      # the first call loads the code object
runs = []
for _ in range(3):
    t0 = time.perf_counter(); dev = E.alpha_diversity(counts, **kw); wall = time.perf_counter() - t0
    runs.append(dict(wall=wall, **{k: float(v) for k, v in E.alpha_timing().items()}))
out["alpha_runs"] = runs
out["draws"] = int((dev["draws"]["reads"] > 0).sum())
out["sizes"] = E.alpha_sizes(counts, nodes, parent, blen, depths=depths, reps=R)
# the baseline: one device otu_subset per (depth, repeat), the table copied back each time; the metrics on the host not included
E.otu_subset(counts[:, :2], 10, seed=1, device=0)
base = []
for _ in range(2):
    t0 = time.perf_counter()
    for m in depths:
        for r in range(R):
            sub = E.otu_subset(counts, m, seed=1 + r, device=0)
    base.append(time.perf_counter() - t0)
out["baseline_subset_calls_wall"] = base
# the last baseline call against the corresponding draws
m = depths[-1]; j = int(np.argmax(tot))
out["check_observed"] = [int((sub[:, j] > 0).sum()), int(dev["draws"]["S"][j, len(depths) - 1, R - 1])]
t0 = time.perf_counter(); host = E.alpha_diversity(counts[:, :8], host=True, **kw); out["host_path_8_samples_wall"] = time.perf_counter() - t0
out["host_equal_ints"] = bool(all((host["draws"][f] == dev["draws"][f][:8]).all() for f in ("S", "F1", "F2", "Q")))
out["host_equal_pd_bits"] = bool(host["draws"]["PD"].tobytes() == np.ascontiguousarray(dev["draws"]["PD"][:8]).tobytes())
dest = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), None)
if dest:
    json.dump(out, open(dest, "w"), indent=1)
print(json.dumps(out))
