"""Rate of hmmufotu-amd-tree's two steps on one device: rows evolved by `synth` down a random tree (JC69, mean
branch 0.05, 5 % of the cells turned into gaps), 7,682 columns as gg_97 has them, n = 4,096, 16,384 and 32,768 rows (--n=..., comma separated).
Distances (JC69): one warm-up, then the best of three calls of msa_distances, the phase `distances` of hu_nj_timing (host clock
around a synchronise: k_dist_pairs, k_dist_scan and, with saturated pairs, k_dist_fix).  A pair-word is one pair of rows and one
64-column word: n (n - 1) / 2 x ceil(7682 / 64) of them, the diagonal tiles' wasted half and the padding words not counted.
Neighbour joining: one call of nj on that matrix, the phase `joins` (all launches of all joins, the copy of the records included).
The argmin reads (r^2 - r) / 2 cells of 8 bytes at the join with r active slots: summed over the joins, the matrix bytes of the
argmin, held against the whole phase, so the rate is a floor for the kernel's own.  Against the device's peaks (MI355X: 8 TB/s HBM,
6.29 TB/s measured for a copy).  The host path runs the first --host-n rows once for a measured ratio against code that is not the
kernels.  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
NS = [int(x) for x in arg("n", "4096,16384,32768").split(",")]
L, N_HOST = int(arg("columns", 7682)), int(arg("host-n", 256))
if E.device_count() < 1:
    sys.exit("tree_rate: no gfx950 device")
rng = np.random.default_rng(97)
nmax = max(NS)
parent, blen, is_leaf = synth.make_tree(nmax, rng)
seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
rows_all = np.ascontiguousarray(seq[is_leaf])
del seq
rows_all[rng.random(rows_all.shape) < 0.05] = -2
out = {"columns": L, "words": -(-L // 64), "hbm_peak_TBps": 8.0, "hbm_copy_TBps": 6.29}
for n in NS:
    rows = np.ascontiguousarray(rows_all[:n])
    r = {}
    ds = []
    for it in range(4):
        t0 = time.perf_counter(); D, ns = E.msa_distances(rows, "JC69"); dt = time.perf_counter() - t0
        if it:
            ds.append((E.nj_timing()["distances"], dt))
        else:
            first = D.tobytes()
        assert D.tobytes() == first
    pw = n * (n - 1) // 2 * (-(-L // 64))
    best = min(ds)
    r.update(saturated=ns, pair_words=pw, distances_s=[round(a, 4) for a, _ in ds], distances_call_s=[round(b, 3) for _, b in ds],
             pair_words_per_s=pw / best[0], columns_compared_per_s=pw * 64 / best[0])
    t0 = time.perf_counter(); tr = E.nj(D); dt = time.perf_counter() - t0
    tm = E.nj_timing()
    cells = sum((k * k - k) // 2 for k in range(4, n + 1))
    r.update(nj_call_s=round(dt, 3), nj_to_device_s=round(tm["to_device"], 4), nj_joins_s=round(tm["joins"], 4), joins=n - 3, launches=5 * (n - 3) + 2,
             argmin_matrix_bytes=cells * 8, argmin_matrix_bytes_per_s=cells * 8 / tm["joins"], share_of_hbm_peak=cells * 8 / tm["joins"] / 8e12,
             seconds_per_join=tm["joins"] / (n - 3))
    if n == min(NS):
        sub = np.ascontiguousarray(rows[:N_HOST])
        t0 = time.perf_counter(); Dh, _ = E.msa_distances(sub, "JC69", host=True); th = time.perf_counter() - t0
        t0 = time.perf_counter(); trh = E.nj(Dh, host=True); tn = time.perf_counter() - t0
        trd = E.nj(Dh)
        r.update(host_n=N_HOST, host_distances_s=round(th, 3), host_pair_words_per_s=N_HOST * (N_HOST - 1) // 2 * (-(-L // 64)) / th, host_nj_s=round(tn, 3),
                 host_nj_equals_device_bits=bool(all(trh[k].tobytes() == trd[k].tobytes() for k in trh)))
    out["n_%d" % n] = r
    print(n, r, flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "tree_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
