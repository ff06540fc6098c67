"""Time of hu_unifrac_rarefied on one device.  The workload is section 30's planted table (fixed seed): 256 samples x
4,096 OTUs, 45,000 to 55,000 reads and 300 to 1,500 nonzero cells per sample, on a tree of 8,001 nodes; `weighted`, one depth (45,000
reads, which keeps every sample) and R = 100 draws.  One warm-up call on two repeats (the first call loads the code object), then three
timed calls: the host clock around the whole call (it checks the table, walks the tree and builds the plan on the host) and
hu_unifrac_rarefied_timing's phases; the best of the three by the whole call is reported beside all three.
The comparison, in the same process, is the only route to these numbers before hu_unifrac_rarefied: a loop of R x (engine.otu_subset on the
device, then engine.unifrac of the kept columns on the device), timed by the host clock around the loop.  It uploads, checks, plans and
copies back the whole table per draw, and it does not include the mean and the deviation, which a script then took on the host.
Also: the pair kernels' terms per second per draw (a term is one (pair, branch)) beside hu_unifrac's own pair kernel on one draw's table
(the same S' and B), and that the loop's last distances are the entry's last draw bit for bit.
--out=PREFIX: where the JSON (PREFIX.json) and the short table (PREFIX.md) go; default profiles/unifrac_rarefied_rate."""
import json, os, sys, time
import numpy as np
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from hmmufotu_amd import engine as E, synth

rng = np.random.default_rng(7)
S, M, R, DEPTH = 256, 4096, 100, 45000
parent, blen, is_leaf = synth.make_tree(4001, rng)
n = len(parent)
nodes = rng.choice(n, M, replace=False).astype(np.int32)
counts = np.zeros((M, S))
for j in range(S):
    k = int(rng.integers(300, 1500))
    rows = rng.choice(M, k, replace=False)
    counts[rows, j] = rng.multinomial(int(rng.integers(45000, 55000)), rng.dirichlet(np.full(k, 0.2)))
tot = counts.sum(0)
kw = dict(otu_node=nodes, parent=parent, blen=blen)
sizes = E.unifrac_rarefied_sizes(counts, depth=DEPTH, reps=R, **kw)
K, B, L = sizes["n_kept"], sizes["n_branch"], sizes["slab"]
terms = K * (K - 1) // 2 * B
out = dict(method="weighted", samples=S, kept=K, otus=M, nodes=n, reads_min=int(tot.min()), reads_max=int(tot.max()), nonzero_cells=int((counts > 0).sum()),
           depth=DEPTH, reps=R, seed=1, branches=B, slab=L, terms_per_draw=terms, sizes=sizes)
E.unifrac_rarefied(counts, depth=DEPTH, reps=2, seed=1, **kw)                    # the first call loads the code object
runs = []
for _ in range(3):
    t0 = time.perf_counter(); lean = E.unifrac_rarefied(counts, depth=DEPTH, reps=R, seed=1, **kw); wall = time.perf_counter() - t0
    runs.append(dict(wall=wall, **{k: float(v) for k, v in E.unifrac_rarefied_timing().items()}))
got = E.unifrac_rarefied(counts, depth=DEPTH, reps=R, seed=1, draws=True, **kw)  # not timed: with every D_r, for the check below
out["mean_same_with_and_without_draws"] = bool(got["mean"].tobytes() == lean["mean"].tobytes())
best = min(runs, key=lambda r: r["wall"])
out["rarefied_runs"] = runs; out["rarefied_best"] = best
out["pairs_terms_per_s_per_draw"] = terms * R / best["pairs"]
# the route of the parent commit: R x (subset on the device, distances on the device); the mean and sd on the host are not included
keep = tot >= DEPTH
E.otu_subset(counts[:, :2], 10, seed=1, device=0)
E.unifrac(np.ascontiguousarray(counts[:, :2]), slab=L, **kw)
base = []
for _ in range(2):
    t0 = time.perf_counter()
    for r in range(R):
        sub = E.otu_subset(counts, DEPTH, seed=1 + r, device=0)
        d = E.unifrac(np.ascontiguousarray(sub[:, keep]), slab=L, **kw)
    base.append(time.perf_counter() - t0)
out["baseline_loop_wall"] = base
out["baseline_last_equals_last_draw"] = bool(d.tobytes() == got["draws"][R - 1].tobytes())
ut = E.unifrac_timing()
out["unifrac_one_draw_timing"] = {k: float(v) for k, v in ut.items()}
out["unifrac_pairs_terms_per_s"] = terms / ut["pairs"]
out["ratio_baseline_over_whole_call"] = min(base) / best["wall"]
prefix = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(os.path.dirname(os.path.abspath(__file__)), "unifrac_rarefied_rate"))
json.dump(out, open(prefix + ".json", "w"), indent=1)
with open(prefix + ".md", "w") as f:
    f.write("hu_unifrac_rarefied, weighted, %d kept samples x %d OTUs, B = %d, L = %d, depth %d, R = %d, %d draws resident (one MI355X; seconds)\n\n" % (K, M, B, L, DEPTH, R, best["resident_draws"]))
    f.write("| | copies up | draws | embedding | pair kernels | accumulate | copy back | whole call |\n|---|---|---|---|---|---|---|---|\n")
    f.write("| best of three | " + " | ".join("%.4f" % best[k] for k in ("to_device", "draws", "embed", "pairs", "accumulate", "to_host", "wall")) + " |\n\n")
    f.write("Loop of R x (otu_subset, unifrac) on the device, two runs: %.3f and %.3f s; over the whole call: %.1f.\n" % (base[0], base[1], out["ratio_baseline_over_whole_call"]))
    f.write("Pair kernels: %.3g terms/s per draw batched; hu_unifrac's pair kernel on one draw's table: %.3g terms/s.\n" % (out["pairs_terms_per_s_per_draw"], out["unifrac_pairs_terms_per_s"]))
print(json.dumps(out))
