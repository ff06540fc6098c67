"""Rate of hu_diffabund on one device: tables of Poisson-like counts from a fixed seed with about 5 % of the cells
nonzero, samples dealt round-robin to groups of equal size, 9,999 permutations: 100,000 OTUs by 1,024 samples with 2 and with 8 groups
(the register and the LDS instance of k_da_sums), and 10,000 OTUs by 256 samples with 2.  One warm-up and three timed calls each, timed
end to end by the host clock (a call checks and ranks the table on the host, and ends in a device synchronise and the copy back) and
split by hu_diffabund_timing into copies up, shuffles, sums (k_da_sums of every chunk and of the observed labelling, host clock around a
synchronise) and finish with the copy back.  A term is one (cell above 0 of a tested OTU, permutation); the observed labelling's launch
and the padding of a row to eight cells are not counted.  The host path (one thread) runs the same permutations on a table it finishes
in about a second, so the ratio is a measured one against code that is not the kernel.
--out=DIR: where the JSON goes; --shapes=MxNxA,..., --perms=P, --host-shape=MxNxA: smaller sizes for a rehearsal."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


def table(n_otu, n, seed, density=0.05):
    rng = np.random.default_rng(seed)
    c = np.zeros((n_otu, n))
    for i0 in range(0, n_otu, 8192):
        m = min(8192, n_otu - i0)
        c[i0:i0 + m] = (rng.random((m, n)) < density) * rng.geometric(0.2, (m, n))
    c[0] += 1.0                                                                  # no sample without reads
    return c


def shape(s):
    return tuple(int(v) for v in s.split("x"))


OUT = arg("out", os.path.join(ROOT, "profiles"))
SHAPES = [shape(s) for s in arg("shapes", "100000x1024x2,100000x1024x8,10000x256x2").split(",")]
P = int(arg("perms", 9999))
HOST = shape(arg("host-shape", "2000x256x2"))
if E.device_count() < 1:
    sys.exit("diffabund_rate: no gfx950 device")
out = {"perms": P, "density": 0.05}
for n_otu, n, a in SHAPES:
    c = table(n_otu, n, 31); g = np.arange(n) % a
    ts = []; phases = []
    for it in range(4):
        t0 = time.perf_counter(); r = E.diffabund(c, g, perms=P, seed=1); dt = time.perf_counter() - t0
        if it:
            ts.append(dt); phases.append(E.diffabund_timing())
        else:
            first = r
        assert r["rec"].tobytes() == first["rec"].tobytes() and r["max_H"].tobytes() == first["max_H"].tobytes()
    tested = r["rec"]["tested"] == 1
    cells = int((c[tested] > 0).sum())
    terms = cells * P
    best = min(phases, key=lambda p: p["sums"])
    res = dict(n_otu=n_otu, n_sample=n, groups=a, tested=int(tested.sum()), cells=cells, terms=terms, smallest_p_maxT=float(np.nanmin(r["rec"]["p_maxT"])),
               need_bytes=E.diffabund_need(n, a, int(tested.sum()), cells, min(P, 16384)), call_s=[round(t, 4) for t in ts],
               to_device_s=[round(p["to_device"], 4) for p in phases], shuffle_s=[round(p["shuffle"], 4) for p in phases],
               sums_s=[round(p["sums"], 4) for p in phases], finish_s=[round(p["finish"], 4) for p in phases],
               terms_per_s_sums=terms / best["sums"], terms_per_s_call=terms / min(ts))
    out["%dx%dx%d" % (n_otu, n, a)] = res
    print(res, flush=True)
    del c
n_otu, n, a = HOST
c = table(n_otu, n, 31); g = np.arange(n) % a
t0 = time.perf_counter(); h = E.diffabund(c, g, perms=P, seed=1, host=True); th = time.perf_counter() - t0
dev = E.diffabund(c, g, perms=P, seed=1)
hterms = int((c[h["rec"]["tested"] == 1] > 0).sum()) * P
big = out["%dx%dx%d" % SHAPES[0]]
out["host"] = dict(n_otu=n_otu, n_sample=n, groups=a, terms=hterms, host_s=round(th, 3), host_terms_per_s=hterms / th,
                   host_equals_device_bytes=bool(h["rec"].tobytes() == dev["rec"].tobytes() and h["max_H"].tobytes() == dev["max_H"].tobytes()),
                   sums_rate_over_host_rate=big["terms_per_s_sums"] / (hterms / th), call_rate_over_host_rate=big["terms_per_s_call"] / (hterms / th))
print(out["host"], flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "diffabund_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
