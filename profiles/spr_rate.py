"""Seconds per phase of one round of hmmufotu-amd-tree --ml-lengths --spr on one device, at radius 3 and at
radius 5 (--radius=..., comma separated): a random binary tree of n = 4,096 leaves (--n=...; 2 n - 1 nodes), rows evolved by `synth`
down it (JC69, mean branch 0.05, 5 % of the cells turned into gaps), 7,682 columns as gg_97 has them.  The leaf rows are then permuted
among 2 % of the leaves, so that the topology is no optimum, and the search runs --rounds rounds (1) with one round of the fit each
(--ml-rounds) under the HKY85 model of the golden files, from the true lengths.  The phases are those of hu_spr_timing, host clock
around calls that end in a synchronise: the fits (hu_tree_optimize_lengths), the scoring (a full sweep up and down with a sweep handle
of its own, which also sends the rows, the walks laid out on the host, k_spr_score slab by slab and the copies of its records and
results) and the trials (an up sweep and hu_tree_loglik each).  A target reads two messages of the level sweeps or of the stack and
up[v], and writes one message to the stack: 128 bytes per target and column; that count is held against the whole scoring phase, so it
is a floor below the kernel's own rate.  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
N, RADII = int(arg("n", 4096)), [int(x) for x in arg("radius", "3,5").split(",")]
L, ROUNDS, ML_ROUNDS = int(arg("columns", 7682)), int(arg("rounds", 1)), int(arg("ml-rounds", 1))
if E.device_count() < 1:
    sys.exit("spr_rate: no gfx950 device")
m = synth.load_model("HKY85")
md = E.model_desc(m.type_id, m.pi, m.par)
rng = np.random.default_rng(97 + N)
parent, blen, is_leaf = synth.make_tree(N, rng)
seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
seq[rng.random(seq.shape) < 0.05] = -2
seq[~is_leaf] = -2
leaves = np.nonzero(is_leaf)[0]
moved = rng.choice(leaves, size=max(2, N // 50), replace=False)
seq[moved] = seq[rng.permutation(moved)]
nodes = len(parent)
out = {"leaves": N, "nodes": nodes, "columns": L, "spr_rounds_asked": ROUNDS, "ml_rounds_per_fit": ML_ROUNDS, "ratios_in_lds": L <= E.BLEN_LDS_COLS}
for radius in RADII:
    t0 = time.perf_counter()
    r = E.tree_spr_search(parent, np.where(parent >= 0, blen, 0.0), seq, md, radius=radius, spr_rounds=ROUNDS, max_rounds=ML_ROUNDS)
    call = time.perf_counter() - t0
    s = r["seconds"]
    passes = len(r["rounds"]) + (0 if r["stop"] == "max rounds" else 1)
    targets = r["rounds"][0]["targets"] if r["rounds"] else 0
    msg = 128 * targets * L
    rec = dict(need_bytes=E.spr_need(nodes, L, radius), call_s=round(call, 3), stop=r["stop"], rounds=r["rounds"], moves=len(r["moves"]),
               move_distances=sorted(x[4] for x in r["moves"]), skipped=r["skipped"], ll_start=r["ll_start"], ll_final=r["ll_final"], fit_s=round(s["fit"], 4),
               score_s=round(s["score"], 4), trial_s=round(s["trial"], 4), other_s=round(s["other"], 4), scoring_passes=passes,
               seconds_per_scoring_pass=s["score"] / max(passes, 1), targets=targets, score_message_bytes=msg,
               score_message_bytes_per_s_of_the_phase=msg * max(passes, 1) / s["score"] if s["score"] > 0 else None)
    out["radius_%d" % radius] = rec
    print(radius, rec, flush=True)
if "radius_3" in out and "radius_5" in out:
    out["round_at_5_over_round_at_3"] = out["radius_5"]["seconds_per_scoring_pass"] / out["radius_3"]["seconds_per_scoring_pass"]
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "spr_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
