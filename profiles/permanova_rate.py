"""Rate of hu_permanova on one device: matrices of the Euclidean distances of n random points in 8 dimensions
(fixed seed), 8 groups of equal size dealt round-robin, n = 4,096 and 16,384 with 9,999 permutations.  One warm-up and three timed calls
each, timed end to end by the host clock (a call checks the matrix on the host, computes SS_T there, and ends in a device synchronise
and the copy back) and split by hu_permanova_timing into copies up, shuffles, pair kernel (k_permanova_pairs of every chunk and of the
observed labelling, host clock around a synchronise) and finish with the copy back.  A term is one (permutation, pair): P x n (n-1) / 2
of them; the diagonal tiles' wasted half and the observed labelling's launch are not counted.  The host path (one thread) runs the same
permutations at n = 512 once, so the ratio is a measured one against code that is not the kernel.  The first size also runs with 512
groups, whose labels the pair kernel keeps as halfwords in LDS (one workgroup on a CU instead of two).
--out=DIR: where the JSON goes; --sizes=A,B, --perms=P, --host-n=N: smaller sizes for a rehearsal."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


def matrix(n, seed):
    x = np.random.default_rng(seed).normal(size=(n, 8))
    sq = (x * x).sum(1)
    d = np.empty((n, n))
    for i0 in range(0, n, 1024):
        b = sq[i0:i0 + 1024, None] + sq[None, :] - 2.0 * (x[i0:i0 + 1024] @ x.T)
        d[i0:i0 + 1024] = np.sqrt(np.maximum(b, 0.0))
    d = np.triu(d, 1)
    return d + d.T


OUT = arg("out", os.path.join(ROOT, "profiles"))
SIZES = [int(v) for v in arg("sizes", "4096,16384").split(",")]
P, N_HOST, A = int(arg("perms", 9999)), int(arg("host-n", 512)), 8
if E.device_count() < 1:
    sys.exit("permanova_rate: no gfx950 device")
out = {"perms": P, "groups": A, "dims": 8}
for n, a in [(n, A) for n in SIZES] + [(SIZES[0], 512)]:
    d = matrix(n, 27); g = np.arange(n) % a
    ts = []; phases = []
    for it in range(4):
        t0 = time.perf_counter(); r = E.permanova(d, g, perms=P, seed=1); dt = time.perf_counter() - t0
        if it:
            ts.append(dt); phases.append(E.permanova_timing())
        else:
            first = r
        assert r["ssw_perm"].tobytes() == first["ssw_perm"].tobytes() and r["p"] == first["p"]
    terms = P * n * (n - 1) // 2
    best = min(phases, key=lambda p: p["pairs"])
    nt = -(-n // 64)
    res = dict(n=n, tiles=nt * (nt + 1) // 2, terms=terms, F=r["F"], p=r["p"], groups=a, need_bytes=E.permanova_need(n, a, min(P, 16384)), call_s=[round(t, 4) for t in ts],
               to_device_s=[round(p["to_device"], 4) for p in phases], shuffle_s=[round(p["shuffle"], 4) for p in phases],
               pairs_s=[round(p["pairs"], 4) for p in phases], finish_s=[round(p["finish"], 4) for p in phases],
               terms_per_s_pairs=terms / best["pairs"], terms_per_s_call=terms / min(ts))
    out["n_%d" % n if a == A else "n_%d_groups_%d" % (n, a)] = res
    print(res, flush=True)
d = matrix(N_HOST, 27); g = np.arange(N_HOST) % A
t0 = time.perf_counter(); h = E.permanova(d, g, perms=P, seed=1, host=True); th = time.perf_counter() - t0
dev = E.permanova(d, g, perms=P, seed=1)
hterms = P * N_HOST * (N_HOST - 1) // 2
big = out["n_%d" % SIZES[-1]]
out["host"] = dict(n=N_HOST, host_s=round(th, 3), host_terms_per_s=hterms / th, host_equals_device_bits=bool(h["ssw_perm"].tobytes() == dev["ssw_perm"].tobytes() and h["F"] == dev["F"]),
                   pairs_rate_over_host_rate=big["terms_per_s_pairs"] / (hterms / th), call_rate_over_host_rate=big["terms_per_s_call"] / (hterms / th))
print(out["host"], flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "permanova_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
