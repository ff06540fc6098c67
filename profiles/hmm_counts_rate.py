"""Rate of the profile training's device counts at gg_97 scale on one device: hu_hmm_counts on a random
99,322 x 7,682 alignment (random letters, ~30 % gaps, some lower-case and IUPAC) with about 1,400 match columns, and the host's
hu_hmm_estimate on the counts it returns.  The call is timed end to end (host <-> device copies and the host's sums included) three
times after one warm-up; the two kernels and the copies come from hu_hmm_counts_timing of the best call, the device memory the call
held from the same entry (hipMemGetInfo before and after its allocations).  --out=DIR: where the JSON goes; --prior=FILE: the .dm file
(default: the test fixture)."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
PRIOR = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--prior=")), os.path.join(ROOT, "tests", "golden", "ref_data", "gg_97_otus.dm"))
N_SEQ, L, K_WANT = 99322, 7682, 1400
rng = np.random.default_rng(97)
out = {"device": torch.cuda.get_device_name(0)}

letters = np.frombuffer(b"ACGTACGTACGTACGTacgtNR----------", np.uint8)
msa = letters[rng.integers(0, len(letters), size=(N_SEQ, L), dtype=np.uint8)]
res = E.msa_encode_table()[msa] >= 0
start = res.argmax(1).astype(np.int32)
end = (L - 1 - res[:, ::-1].argmax(1)).astype(np.int32)
del res
weight = rng.random(N_SEQ) + 0.5
weight *= N_SEQ / weight.sum()
mask = np.zeros(L, bool)
mask[rng.choice(L, K_WANT, replace=False)] = True

best, phases = None, None
E.hmm_counts(msa, weight, start, end, mask)                                              # warm-up
ts = []
for _ in range(3):
    t0 = time.perf_counter(); c = E.hmm_counts(msa, weight, start, end, mask); ts.append(time.perf_counter() - t0)
    if best is None or ts[-1] < best:
        best, phases = ts[-1], E.hmm_counts_timing()
out["hmm_counts"] = dict(n_seq=N_SEQ, cs_len=L, K=int(mask.sum()), bytes=int(msa.nbytes), s=[round(t, 4) for t in ts], best_s=round(best, 4),
                         to_device_s=round(phases["to_device"], 4), states_kernel_s=round(phases["states_kernel"], 4),
                         counts_kernel_s=round(phases["counts_kernel"], 4), to_host_s=round(phases["to_host"], 4),
                         device_held_gb=round(phases["peak_bytes"] / 1e9, 3), compo_sum=float(c["e_m"][0].sum()))
del msa

prior = E.hmm_prior_read(PRIOR)
ts = []
for _ in range(3):
    t0 = time.perf_counter(); est = E.hmm_estimate(c["e_m"], c["e_i"], c["t"], N_SEQ, prior); ts.append(time.perf_counter() - t0)
out["hmm_estimate"] = dict(K=int(mask.sum()), s=[round(t, 4) for t in ts], best_s=round(min(ts), 4), eff_n=est["eff_n"], passes=est["passes"])
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "hmm_counts_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
