"""Seconds per round of hmmufotu-amd-tree --ml-lengths on one device: a random binary tree of n = 4,096 and 16,384
leaves (--n=..., comma separated; 2 n - 1 nodes), rows evolved by `synth` down it (JC69, mean branch 0.05, 5 % of the cells turned
into gaps), 7,682 columns as gg_97 has them.  The fit starts from the true lengths scaled by a factor drawn from [0.5, 1.5] per
branch and runs --rounds rounds (3) under the HKY85 model of the golden files; the phases are those of hu_blen_timing, host clock
around calls that end in a synchronise: the full sweeps (up and down; the first one also sends the rows), the steps (k_blen_step and
the copies of its 44 n bytes of results), the trial sweeps (up only, with hu_tree_loglik and its copy of 8 x columns bytes).  A step
reads the two messages of every non-root branch once, 64 bytes per branch and column: that count, held against the whole step phase,
is a floor for the kernel's own rate; above HU_BLEN_LDS_COLS columns the ratios also go through global memory, 24 bytes per branch
and column written once and read once per evaluation of f', which the count leaves out.  Against the device's peaks (MI355X: 8 TB/s
HBM, 6.29 TB/s measured for a copy).  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
NS = [int(x) for x in arg("n", "4096,16384").split(",")]
L, ROUNDS = int(arg("columns", 7682)), int(arg("rounds", 3))
if E.device_count() < 1:
    sys.exit("blen_rate: no gfx950 device")
m = synth.load_model("HKY85")
md = E.model_desc(m.type_id, m.pi, m.par)
out = {"columns": L, "rounds_asked": ROUNDS, "ratios_in_lds": L <= E.BLEN_LDS_COLS, "hbm_peak_TBps": 8.0, "hbm_copy_TBps": 6.29}
for n in NS:
    rng = np.random.default_rng(97 + n)
    parent, blen, is_leaf = synth.make_tree(n, rng)
    seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
    seq[rng.random(seq.shape) < 0.05] = -2
    seq[~is_leaf] = -2
    nodes = len(parent)
    start = np.where(parent >= 0, blen * rng.uniform(0.5, 1.5, nodes), 0.0)
    t0 = time.perf_counter()
    r = E.tree_optimize_lengths(parent, start, seq, md, max_rounds=ROUNDS)
    call = time.perf_counter() - t0
    s = r["seconds"]
    steps = len(r["rounds"]) + (0 if r["stop"] == "max rounds" else 1)
    sweeps = 1 + max(steps - 1, 0)
    trials = sum(1 + int(round(-np.log2(x["s"]))) for x in r["rounds"])
    msg = 64 * (nodes - 1) * L
    rec = dict(nodes=nodes, need_bytes=E.blen_need(nodes, L), call_s=round(call, 3), stop=r["stop"], rounds=r["rounds"], ll_start=r["ll_start"], ll_final=r["ll_final"],
               full_sweeps=sweeps, steps=steps, trial_sweeps=trials, sweep_s=round(s["sweep"], 4), step_s=round(s["step"], 4), trial_s=round(s["trial"], 4),
               other_s=round(s["other"], 4), seconds_per_full_sweep=s["sweep"] / sweeps, seconds_per_step=s["step"] / max(steps, 1),
               seconds_per_trial_sweep=s["trial"] / max(trials, 1), seconds_per_round=(s["sweep"] + s["step"] + s["trial"]) / max(steps, 1),
               step_message_bytes=msg, step_message_bytes_per_s=msg * max(steps, 1) / s["step"], share_of_hbm_peak=msg * max(steps, 1) / s["step"] / 8e12)
    out["n_%d" % n] = rec
    print(n, rec, flush=True)
    del seq
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "blen_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
