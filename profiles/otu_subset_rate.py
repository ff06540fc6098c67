"""Time of hu_otu_subset on one device and on the library's host path.  The table: 1,024 samples of 10^6 reads
over 50,000 OTUs (log-normal abundances, about 70 % of the cells zero), size 10^5, both methods.  Device: one warm-up and three timed
calls of the whole table, wall time of the call (it ends in a device synchronise and the copy back) and the phases of the best call
from hu_otu_subset_timing.  Host path: one call on the first HOST_SAMPLES samples of the same table (single-threaded; the whole table
would take minutes), whose result must equal the device's columns.  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
N_OTU, N_SAMPLE, READS, SIZE, HOST_SAMPLES = 50000, 1024, 10 ** 6, 10 ** 5, 64
rng = np.random.default_rng(17)
out = {"device": torch.cuda.get_device_name(0), "n_otu": N_OTU, "n_sample": N_SAMPLE, "reads_per_sample": READS, "size": SIZE}

base = rng.lognormal(0.0, 2.0, N_OTU)
counts = np.zeros((N_OTU, N_SAMPLE))
for j in range(N_SAMPLE):
    p = base * rng.lognormal(0.0, 1.0, N_OTU) * (rng.random(N_OTU) >= 0.7)
    counts[:, j] = rng.multinomial(READS, p / p.sum())
out["zero_cells"] = round(float((counts == 0).mean()), 3)

for method in ("uniform", "multinomial"):
    got = E.otu_subset(counts, SIZE, method, seed=1)                                      # warm-up
    best, phases, ts = None, None, []
    for _ in range(3):
        t0 = time.perf_counter(); got = E.otu_subset(counts, SIZE, method, seed=1); ts.append(time.perf_counter() - t0)
        if best is None or ts[-1] < best:
            best, phases = ts[-1], E.otu_subset_timing()
    assert (got.sum(0) == SIZE).all()
    t0 = time.perf_counter(); host = E.otu_subset(counts[:, :HOST_SAMPLES], SIZE, method, seed=1, device=-1); th = time.perf_counter() - t0
    assert (host == got[:, :HOST_SAMPLES]).all()
    out[method] = dict(device_call_s=[round(t, 4) for t in ts], best_s=round(best, 4), to_device_s=round(phases["to_device"], 4), kernels_s=round(phases["kernels"], 4),
                       to_host_s=round(phases["to_host"], 4), host_path_samples=HOST_SAMPLES, host_path_s=round(th, 3), host_path_s_per_sample=round(th / HOST_SAMPLES, 4),
                       equal_on_host_samples=True)
    print(method, out[method], flush=True)
os.makedirs(OUT, exist_ok=True)
json.dump(out, open(os.path.join(OUT, "otu_subset_rate.json"), "w"), indent=1)
print(json.dumps(out))
