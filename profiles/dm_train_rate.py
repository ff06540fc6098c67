"""Rate of the prior training's device work at gg_97 scale on one device.  hu_dm_training_data on a random
99,322 x 7,682 alignment (about 1,400 columns with few gaps, the others mostly gaps; some lower-case and IUPAC letters): the call is
timed end to end three times after one warm-up, the kernels and the copies come from hu_dm_training_data_timing of the best call, the
device memory the call held from the same entry.  hu_dm_train on the sets it returns, as the program batches them: n match-emission
mixtures (qM = 5, each from its own shuffle) and the four densities, n = 1, 8 and 32, capped at 500 iterations; one warm-up and three
timed runs each, seconds to the cap and per iteration, and the ratio of 32 seeds to one.  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
N_SEQ, L, K_WANT, CAP = 99322, 7682, 1400, 500
rng = np.random.default_rng(97)
out = {"device": torch.cuda.get_device_name(0)}

dense = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTacgtNR--", np.uint8)
sparse = np.frombuffer(b"ACGTacNR------------------------", np.uint8)
match = np.zeros(L, bool)
match[rng.choice(L, K_WANT, replace=False)] = True
pick = rng.integers(0, 32, size=(N_SEQ, L), dtype=np.uint8)
msa = np.where(match[None, :], dense[pick], sparse[pick])
del pick
weight = rng.random(N_SEQ) + 0.5
weight *= N_SEQ / weight.sum()

best, phases = None, None
E.dm_training_data(msa, weight)                                                          # warm-up
ts = []
for _ in range(3):
    t0 = time.perf_counter(); td = E.dm_training_data(msa, weight); ts.append(time.perf_counter() - t0)
    if best is None or ts[-1] < best:
        best, phases = ts[-1], E.dm_training_data_timing()
out["dm_training_data"] = dict(n_seq=N_SEQ, cs_len=L, bytes=int(msa.nbytes), columns={k: int(td[k].shape[1]) for k in ("me", "ie", "mt", "it", "dt")},
                               s=[round(t, 4) for t in ts], best_s=round(best, 4), to_device_s=round(phases["to_device"], 4),
                               wcounts_and_mask_s=round(phases["wcounts_and_mask"], 4), states_kernels_s=round(phases["states_kernels"], 4),
                               counts_kernel_s=round(phases["counts_kernel"], 4), device_held_gb=round(phases["peak_bytes"] / 1e9, 3))
del msa

dens = [dict(data=td[k], alpha0=E.dm_moment_init(td[k])) for k in ("ie", "mt", "it", "dt")]
M = td["me"].shape[1]
out["dm_train"] = {}
for n in (1, 8, 32):
    probs = [dict(data=td["me"], alpha0=E.dm_moment_init(td["me"], 5, E.dm_shuffle(M, 1 if s == 0 else None))) for s in range(n)] + dens
    E.dm_train(probs, max_iter=CAP)                                                      # warm-up
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); res = E.dm_train(probs, max_iter=CAP); ts.append(time.perf_counter() - t0)
    its = max(r["iterations"] for r in res)
    out["dm_train"]["n%d" % n] = dict(problems=len(probs), me_columns=M, s=[round(t, 4) for t in ts], best_s=round(min(ts), 4), iterations=its,
                                     s_per_iteration=round(min(ts) / its, 6), statuses=sorted({r["status"] for r in res}))
out["dm_train"]["ratio_32_to_1"] = round(out["dm_train"]["n32"]["best_s"] / out["dm_train"]["n1"]["best_s"], 3)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "dm_train_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
