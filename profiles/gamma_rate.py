"""Seconds of the phases of hmmufotu-amd-tree --ml-lengths --gamma K on one device, next to the fixed-rate
figures of profiles/blen_rate.py from the same session: the same trees (a random binary tree of n = 4,096 and 16,384 leaves, --n=...,
comma separated; rows evolved by `synth` down it under JC69, mean branch 0.05, 5 % of the cells turned into gaps), 7,682 columns, the
HKY85 model of the golden files, K = 4 at alpha = 0.5.  hu_gamma_profile runs a full sweep (up and down, all categories), a step
(k_gamma_step and the copies of its 44 n bytes of results) and a trial (the up sweep, hu_tree_loglik per category and its copies)
--reps times each (6) by the host clock around calls that end in a synchronise, once with the sweeps over all categories in one launch
per level and once with K runs of the fixed-rate level kernels; the medians leave the first repetition, which also sends the rows, out.
A round is a full sweep, a step and a trial.  The shape search is the `shape` phase of a fit of one pass and one round:
HU_GAMMA_SHAPE_EVALS trials with the rates set anew.  A step reads the two messages of every non-root branch in every category once,
64 K bytes per branch and column: that count, held against the whole step phase, is a floor for the kernel's own rate; beyond LDS the
4 K values of a column also go through the global scratch, written once and read once per evaluation of f', which the count leaves
out.  --out=DIR: where gamma_rate.json and the table for DESIGN.md (gamma_rate.md) go."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
NS = [int(x) for x in arg("n", "4096,16384").split(",")]
L, K, REPS, ROUNDS, ALPHA = int(arg("columns", 7682)), int(arg("k", 4)), int(arg("reps", 6)), int(arg("rounds", 3)), float(arg("alpha", 0.5))
if E.device_count() < 1:
    sys.exit("gamma_rate: no gfx950 device")
if REPS < 6:
    sys.exit("gamma_rate: at least 6 repetitions, the first is the warm-up")
m = synth.load_model("HKY85")
md = E.model_desc(m.type_id, m.pi, m.par)
out = {"columns": L, "k": K, "alpha": ALPHA, "reps": REPS, "values_in_lds": L <= E.gamma_lds_cols(K), "hbm_peak_TBps": 8.0, "hbm_copy_TBps": 6.29}
rows = []
for n in NS:
    rng = np.random.default_rng(97 + n)
    parent, blen, is_leaf = synth.make_tree(n, rng)
    seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
    seq[rng.random(seq.shape) < 0.05] = -2
    seq[~is_leaf] = -2
    nodes = len(parent)
    start = np.where(parent >= 0, blen * rng.uniform(0.5, 1.5, nodes), 0.0)
    # the fixed-rate fit, as blen_rate.py measures it
    r = E.tree_optimize_lengths(parent, start, seq, md, max_rounds=ROUNDS)
    s = r["seconds"]
    steps = len(r["rounds"]) + (0 if r["stop"] == "max rounds" else 1)
    sweeps = 1 + max(steps - 1, 0)
    trials = sum(1 + int(round(-np.log2(x["s"]))) for x in r["rounds"])
    fixed = dict(full_sweep_s=s["sweep"] / sweeps, step_s=s["step"] / max(steps, 1), trial_s=s["trial"] / max(trials, 1))
    fixed["round_s"] = fixed["full_sweep_s"] + fixed["step_s"] + fixed["trial_s"]
    fixed["step_message_bytes_per_s"] = 64 * (nodes - 1) * L / fixed["step_s"]
    med = {}
    for name, reruns in (("batched", False), ("reruns", True)):
        t = E.gamma_profile(parent, start, seq, md, k=K, alpha=ALPHA, reps=REPS, sweep_reruns=reruns)
        med[name] = dict(zip(("full_sweep_s", "step_s", "trial_s"), np.median(t[1:], axis=0).tolist()), all=t.tolist())
    t0 = time.perf_counter()
    f = E.tree_gamma_fit(parent, start, seq, md, k=K, max_outer=1, max_rounds=1)
    fit_call = time.perf_counter() - t0
    b = med["batched"]
    msg = 64 * K * (nodes - 1) * L
    rec = dict(nodes=nodes, need_bytes=E.gamma_need(nodes, L, K), fixed_rate=fixed, batched=b, reruns=med["reruns"],
               round_s=b["full_sweep_s"] + b["step_s"] + b["trial_s"], shape_search_s=f["seconds"]["shape"], fit_of_one_pass_one_round_s=fit_call,
               alpha_after_one_search=f["alpha"], step_message_bytes=msg, step_message_bytes_per_s=msg / b["step_s"], share_of_hbm_peak=msg / b["step_s"] / 8e12,
               batched_over_reruns_full_sweep=b["full_sweep_s"] / med["reruns"]["full_sweep_s"], batched_over_reruns_trial=b["trial_s"] / med["reruns"]["trial_s"])
    out["n_%d" % n] = rec
    print(n, {k: v for k, v in rec.items() if k not in ("batched", "reruns")}, {k: v for k, v in b.items() if k != "all"},
          {k: v for k, v in med["reruns"].items() if k != "all"}, flush=True)
    rows.append("| %d | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.2f | %.2f | %.4f / %.4f / %.4f / %.4f | %.2f |" % (
        nodes, b["full_sweep_s"], med["reruns"]["full_sweep_s"], b["trial_s"], med["reruns"]["trial_s"], b["step_s"], rec["round_s"], rec["shape_search_s"],
        rec["step_message_bytes_per_s"] / 1e12, fixed["full_sweep_s"], fixed["step_s"], fixed["trial_s"], fixed["round_s"], fixed["step_message_bytes_per_s"] / 1e12))
    del seq
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "gamma_rate.json"), "w") as fh:
    json.dump(out, fh, indent=1)
with open(os.path.join(OUT, "gamma_rate.md"), "w") as fh:
    fh.write("| nodes | full sweep, one launch per level (s) | full sweep, K reruns (s) | trial, one launch (s) | trial, K reruns (s) | step (s) | round (s) | shape search (s) "
             "| step TB/s of messages | fixed rate: full sweep / step / trial / round (s) | fixed-rate step TB/s |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
    fh.write("\n".join(rows) + "\n")
