"""Rate of the .csfm writer on the synthetic 99,322 x 7,682 alignment of profiles/measure_seed_index.py, one device.
Medians of --reps (3) runs after one warm-up:
  suffix_array    device time of hu_suffix_array alone (no copies), and the doubling rounds it took
  csfm_write      wall time of hu_csfm_write, split into text, device (with copies) and encode + write
  peak device memory while hu_csfm_write runs: hipMemGetInfo (torch.cuda.mem_get_info) polled from a second thread, as build_stats_rate.py
  csfm_ref        wall time of oracle/_ref/csfm_ref (the reference's own libcds + libdivsufsort, single-threaded) on the same alignment,
                  and whether the two files agree byte for byte behind the 20-byte head (csSeq aside: csfm_ref's comes from unweighted counts,
                  which is what this script passes too)
  load / create   wall times of hu_seed_index_load_csfm on the written file and of hu_seed_index_create from the rows (16 host threads)
Usage: python profiles/csfm_write_rate.py [--leaves=N] [--reps=R] [--no-ref] [--out=DIR]  -> profiles/csfm_write_rate.json"""
import json, os, statistics, subprocess, sys, tempfile, threading, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E


def opt(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT, leaves, reps = opt("out", os.path.join(ROOT, "profiles")), int(opt("leaves", 99322)), int(opt("reps", 3))
L, K = 7682, 1400
rng = np.random.default_rng(97)
match = np.zeros(L, bool); match[np.sort(rng.choice(L, K, replace=False))] = True
base = np.empty((leaves, K), np.int8)
base[0] = rng.integers(0, 4, K)
for i in range(1, leaves):                       # every row: a copy of an earlier row with 3 % substitutions
    row = base[int(rng.integers(max(0, i - 64), i))].copy()
    m = rng.random(K) < 0.03
    row[m] = (row[m] + rng.integers(1, 4, int(m.sum()))) % 4
    base[i] = row
seq = np.full((leaves, L), -2, np.int8)
seq[:, match] = np.where(rng.random((leaves, K)) < 0.02, -2, base)
rows = np.frombuffer(b"ACGT", np.uint8)[np.maximum(seq, 0)]
rows[seq < 0] = ord("-")
cnt = np.stack([(seq == b).sum(0) for b in range(4)])
gap = (seq < 0).sum(0)
cs = "".join("ACGT"[int(c.argmax())] if c.max() >= g else "-" for c, g in zip(cnt.T, gap))
ident = cnt.max(0) / leaves
text = np.concatenate([np.where(seq >= 0, seq + 1, -1).astype(np.int8), np.zeros((leaves, 1), np.int8)], 1).ravel()
text = np.concatenate([text[text >= 0].astype(np.uint8), np.zeros(1, np.uint8)])
out = {"device": torch.cuda.get_device_name(0), "leaves": leaves, "cs_len": L, "symbols": int(len(text)), "reps": reps, "host_threads": min(16, os.cpu_count())}


def timed(f):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = f(); ts.append((time.perf_counter() - t0, r))
    return ts


def med(v):
    return round(statistics.median(v), 4)


def peak_used_gb(f):
    free0, total = torch.cuda.mem_get_info(0)
    low, done = [free0], threading.Event()

    def poll():
        while not done.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0]); time.sleep(5e-5)
    t = threading.Thread(target=poll); t.start()
    try:
        f()
    finally:
        done.set(); t.join()
    return round((total - low[0]) / 1e9, 2), round((total - free0) / 1e9, 2)


with tempfile.TemporaryDirectory() as tmp:
    ts = timed(lambda: E.suffix_array(text, info=True)[1:])
    out["suffix_array"] = dict(device_s=med([r[1] for _, r in ts]), wall_s=med([t for t, _ in ts]), rounds=ts[0][1][0], symbols_per_s=round(len(text) / statistics.median([r[1] for _, r in ts])))
    mine = os.path.join(tmp, "mine.csfm")
    ts = timed(lambda: (E.csfm_write(mine, rows, cs, ident), E.csfm_write_timing())[1])
    out["csfm_write"] = dict(wall_s=med([t for t, _ in ts]), text_s=med([r["text"] for _, r in ts]), device_s=med([r["device"] for _, r in ts]),
                             encode_write_s=med([r["encode_write"] for _, r in ts]), suffix_array_s=med([r["suffix_array"] for _, r in ts]),
                             rounds=ts[0][1]["rounds"], file_bytes=os.path.getsize(mine))
    peak, before = peak_used_gb(lambda: E.csfm_write(mine, rows, cs, ident))
    out["csfm_write"].update(device_used_gb_before=before, device_used_gb_peak=peak, device_bytes_per_symbol=round((peak - before) * 1e9 / len(text), 1))
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "csfm_ref")
    if "--no-ref" not in sys.argv and os.path.exists(ref_bin):
        fa, theirs = os.path.join(tmp, "msa.fa"), os.path.join(tmp, "ref.csfm")
        with open(fa, "wb") as f:
            for i in range(leaves):
                f.write(b">s%d\n" % i); f.write(rows[i].tobytes()); f.write(b"\n")
        ts = timed(lambda: subprocess.run([ref_bin, fa, theirs], check=True, capture_output=True))
        a, b = open(mine, "rb").read(), open(theirs, "rb").read()
        out["csfm_ref"] = dict(wall_s=med([t for t, _ in ts]), same_bytes_behind_the_head=a[20:] == b)
        out["csfm_write"]["speedup_over_csfm_ref"] = round(out["csfm_ref"]["wall_s"] / out["csfm_write"]["wall_s"], 2)
        del a, b

    class H:
        pass
    h = H(); h.K = K; h.p2cs = np.concatenate([[0], np.nonzero(match)[0] + 1]).astype(np.int32)
    ts = timed(lambda: E.SeedIndex(None, None, h, 20, csfm=mine).positions)
    out["seed_index_load_csfm"] = dict(wall_s=med([t for t, _ in ts]), positions=ts[0][1])
    parent = np.zeros(leaves + 1, np.int32); parent[0] = -1          # a star: node 0 is the root, every other node a leaf
    allseq = np.vstack([np.zeros((1, L), np.int8), seq])
    ts = timed(lambda: E.SeedIndex(parent, allseq, h, 20).positions)
    out["seed_index_create"] = dict(wall_s=med([t for t, _ in ts]), positions=ts[0][1])
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "csfm_write_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
