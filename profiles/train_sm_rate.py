"""Rate of hu_sm_counts at gg_97 scale on one device: 99,322 encoded rows x 7,682 columns (random bases, ~30 %
gaps, a few invalid codes) under a random binary tree of as many leaves, with the Gojobori training set of that tree from
hu_sm_training_set: one triple per internal node with two children of which one is a tip.  Reported: the wall time of E.sm_counts
(median of five calls after one warm-up, copies included), the phases the entry times itself (allocation and host-to-device copy, kernel,
copies back), the peak device memory while it runs (hipMemGetInfo polled from a second thread, as build_stats_rate.py does), and the
time of the same counts in numpy on a sample of the items, SCALED to the whole item set.  --out=DIR: where the JSON goes."""
import json, os, sys, threading, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
N_LEAVES, L, SAMPLE = 99322, 7682, 64
rng = np.random.default_rng(97)
out = {"device": torch.cuda.get_device_name(0)}


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


def numpy_counts(rows, items):
    """calcTransFreq3Seq and the two pDist of every triple, restated (src/DNASubModel.cpp:75-104, src/SeqUtils.cpp:37-54)"""
    counts, dn = np.zeros((len(items), 4, 4), np.int32), np.zeros((len(items), 4), np.int32)
    for i, (r0, r1, r2) in enumerate(items):
        b0, b1, b2 = rows[r0].astype(int), rows[r1].astype(int), rows[r2].astype(int)
        anc = np.where((b0 == b1) | (b0 == b2), b0, np.where(b1 == b2, b1, -1))
        ok = (b0 >= 0) & (b1 >= 0) & (b2 >= 0) & (anc >= 0)
        for b in (b0, b1, b2):
            np.add.at(counts[i], (anc[ok], b[ok]), 1)
        v1, v2 = (b0 >= 0) & (b1 >= 0), (b0 >= 0) & (b2 >= 0)
        dn[i] = ((v1 & (b0 != b1)).sum(), v1.sum(), (v2 & (b0 != b2)).sum(), v2.sum())
    return counts, dn


parent, blen, is_leaf = synth.make_tree(N_LEAVES, rng)
n = len(parent)
order = np.argsort(parent[1:], kind="stable") + 1                  # children grouped by parent, in id order
child_off = np.zeros(n + 1, np.int32)
np.add.at(child_off, parent[1:] + 1, 1)
child_off = np.cumsum(child_off).astype(np.int32)
row_of = np.full(n, -1, np.int32)
row_of[is_leaf] = np.arange(N_LEAVES)
items = E.sm_training_set(parent, child_off, order.astype(np.int32), row_of, "Gojobori")
codes = np.array([0, 1, 2, 3] * 4 + [-2] * 7 + [-1], np.int8)
rows = codes[rng.integers(0, len(codes), size=(N_LEAVES, L), dtype=np.uint8)]

E.sm_counts(rows, items)                                           # warm-up
ts, phases = [], []
for _ in range(5):
    t0 = time.perf_counter(); got = E.sm_counts(rows, items); ts.append(time.perf_counter() - t0)
    phases.append(E.sm_counts_timing())
peak, before = peak_used_gb(lambda: E.sm_counts(rows, items))
sample = items[np.linspace(0, len(items) - 1, SAMPLE).astype(int)]
t0 = time.perf_counter(); ref_counts, ref_dn = numpy_counts(rows, sample); t_np = time.perf_counter() - t0
pick = np.linspace(0, len(items) - 1, SAMPLE).astype(int)
med = lambda k: round(float(np.median([p[k] for p in phases])), 4)
out["sm_counts"] = dict(n_rows=N_LEAVES, cs_len=L, n_items=int(len(items)), rows_bytes=int(rows.nbytes), calls_s=[round(t, 4) for t in ts],
                        median_s=round(float(np.median(ts)), 4), to_device_s=med("to_device"), kernel_s=med("kernel"), to_host_s=med("to_host"),
                        device_used_gb_before=before, device_used_gb_peak=peak,
                        numpy_sample_items=SAMPLE, numpy_sample_s=round(t_np, 4), numpy_scaled_to_all_items_s=round(t_np * len(items) / SAMPLE, 1),
                        sample_equal=bool(np.array_equal(got["counts"][pick], ref_counts) and np.array_equal(got["dn"][pick], ref_dn)),
                        items_passed=int(got["pass"].sum()))
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "train_sm_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
