"""Rate of the build's device statistics at gg_97 scale on one device:
hu_msa_stats on a 99,322 x 7,682 alignment (random letters, ~30 % gaps, some lower-case and IUPAC), and hu_tree_count_mutations over a
198,643-node x 7,682-column up buffer (48.8 GB of float64; random values, the same traffic as the fixed-rate messages of hu_tree_evaluate).
Each call is timed end to end (host <-> device copies included) three times after one warm-up.  Peak device memory is the device's
used memory (hipMemGetInfo, via torch.cuda.mem_get_info) polled from a second thread during one more call: it includes the engine's own
hipMalloc scratch, which torch's allocator statistics do not see.  --out=DIR: where the JSON goes."""
import json, os, sys, threading, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
N_LEAVES, L = 99322, 7682
rng = np.random.default_rng(97)
out = {"device": torch.cuda.get_device_name(0)}


def timed(f, reps=3):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return ts


def peak_used_gb(f):
    """the largest device memory in use while f() runs, and before it (GB), from hipMemGetInfo polled every ~50 us"""
    free0, total = torch.cuda.mem_get_info(0)
    low = [free0]
    done = threading.Event()

    def poll():
        while not done.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
            time.sleep(5e-5)
    t = threading.Thread(target=poll); t.start()
    try:
        f()
    finally:
        done.set(); t.join()
    return round((total - low[0]) / 1e9, 2), round((total - free0) / 1e9, 2)


letters = np.frombuffer(b"ACGTACGTACGTACGTacgtNR----------", np.uint8)
msa = letters[rng.integers(0, len(letters), size=(N_LEAVES, L), dtype=np.uint8)]
ts = timed(lambda: E.msa_stats(msa))
st = E.msa_stats(msa)
peak, before = peak_used_gb(lambda: E.msa_stats(msa))
out["msa_stats"] = dict(n_seq=N_LEAVES, cs_len=L, bytes=int(msa.nbytes), s=[round(t, 4) for t in ts], best_s=round(min(ts), 4),
                        weight_sum=float(st["seq_weight"].sum()), device_used_gb_before=before, device_used_gb_peak=peak)
del msa, st

parent, blen, is_leaf = synth.make_tree(N_LEAVES, rng)
n = len(parent)
torch.manual_seed(0)
up = torch.randn((n, L, 4), dtype=torch.float64, device="cuda:0")
torch.cuda.synchronize()
ts = timed(lambda: E.tree_count_mutations(parent, L, up.data_ptr()))
cnt = E.tree_count_mutations(parent, L, up.data_ptr())
peak, before = peak_used_gb(lambda: E.tree_count_mutations(parent, L, up.data_ptr()))
gb = n * L * 32 / 1e9
out["count_mutations"] = dict(n_nodes=n, cs_len=L, up_gb=round(gb, 2), s=[round(t, 4) for t in ts], best_s=round(min(ts), 4),
                              up_gb_per_s=round(gb / min(ts), 1), mean_count=float(cnt.mean()),
                              scratch_gb=round((n * L + n * 4 + L * 4) / 1e9, 2), device_used_gb_before=before, device_used_gb_peak=peak)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "build_stats_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
