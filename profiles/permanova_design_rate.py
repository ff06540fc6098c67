"""Rate of hu_permanova_design on one device: section 27's fixture (the Euclidean distances of n random points in 8
dimensions, fixed seed) at n = 4,096 and 16,384 with 9,999 permutations and three designs: one factor of 8 levels (q = 7); that factor,
a covariate and their interaction (q = 15); a factor of 100 levels (q = 99).  One warm-up and three timed calls each, timed end to end by
the host clock and split by hu_permanova_design_timing into copies up (with the squares), shuffles, the quadratic-form kernel
(k_pmd_quad of every chunk and of the identity, host clock around a synchronise) and finish with the copy back.  The kernel's work is
counted as 2 n^2 q P flop; the epilogue, the padding of the column blocks and the identity's launch are not counted.  As context, not as
a bar: the host path (one thread) at n = 512 on the first design with --host-perms permutations, and hu_permanova's pair kernel on the
first design's labels, which answers the same question for one factor without a matrix product.
--out=DIR: where the JSON goes; --sizes=A,B, --perms=P, --host-n=N, --host-perms=P: smaller sizes for a rehearsal."""
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


def designs(n):
    g = (np.arange(n) % 8).tolist(); c = np.random.default_rng(28).normal(size=n).tolist(); h = (np.arange(n) % 100).tolist()
    return [("factor8", dict(g=g), ["g"], ("g",)), ("factor8*covariate", dict(g=g, c=c), ["g", "c", "g:c"], ("g",)), ("factor100", dict(h=h), ["h"], ("h",))]


OUT = arg("out", os.path.join(ROOT, "profiles"))
SIZES = [int(v) for v in arg("sizes", "4096,16384").split(",")]
P, N_HOST, P_HOST = int(arg("perms", 9999)), int(arg("host-n", 512)), int(arg("host-perms", 999))
if E.device_count() < 1:
    sys.exit("permanova_design_rate: no gfx950 device")
out = {"perms": P, "dims": 8}
for n in SIZES:
    d = matrix(n, 27)
    for name, variables, terms, factors in designs(n):
        t0 = time.perf_counter(); D = E.design_build(variables, terms, factors=factors); tb = time.perf_counter() - t0
        ts = []; phases = []
        for it in range(4):
            t0 = time.perf_counter(); r = E.permanova_design(d, D["Q"], D["term_start"], perms=P, seed=1); dt = time.perf_counter() - t0
            if it:
                ts.append(dt); phases.append(E.permanova_design_timing())
            else:
                first = r
            assert r["ss_perm"].tobytes() == first["ss_perm"].tobytes() and r["terms"] == first["terms"]
        flop = 2.0 * n * n * D["q"] * P
        quad = [p["quad"] for p in phases]
        res = dict(n=n, design=name, q=D["q"], T=len(terms), flop=flop, slabs=E.pcoa_slabs(n), build_s=round(tb, 4), F=[t["F"] for t in r["terms"]], p=[t["p"] for t in r["terms"]],
                   need_bytes=E.permanova_design_need(n, D["q"], len(terms), min(P, 16384)), call_s=[round(t, 4) for t in ts],
                   to_device_s=[round(p["to_device"], 4) for p in phases], shuffle_s=[round(p["shuffle"], 4) for p in phases], quad_s=[round(t, 4) for t in quad],
                   finish_s=[round(p["finish"], 4) for p in phases], flops_quad_best=flop / min(quad), flops_quad_worst=flop / max(quad), flops_call_best=flop / min(ts))
        if name == "factor8":                                            # the same question through hu_permanova's pair kernel
            g = np.asarray(variables["g"])
            pk = []
            for it in range(4):
                t0 = time.perf_counter(); o = E.permanova(d, g, perms=P, seed=1); dt = time.perf_counter() - t0
                if it:
                    pk.append((dt, E.permanova_timing()["pairs"]))
            res.update(pairs_call_s=[round(a, 4) for a, _ in pk], pairs_kernel_s=[round(b, 4) for _, b in pk], pairs_p=o["p"], quad_over_pairs_kernel=min(quad) / min(b for _, b in pk))
        out["n_%d_%s" % (n, name)] = res
        print(res, flush=True)
d = matrix(N_HOST, 27)
name, variables, terms, factors = designs(N_HOST)[0]
D = E.design_build(variables, terms, factors=factors)
t0 = time.perf_counter(); h = E.permanova_design(d, D["Q"], D["term_start"], perms=P_HOST, seed=1, host=True); th = time.perf_counter() - t0
t0 = time.perf_counter(); dev = E.permanova_design(d, D["Q"], D["term_start"], perms=P_HOST, seed=1); td = time.perf_counter() - t0
hflop = 2.0 * N_HOST * N_HOST * D["q"] * P_HOST
bar = N_HOST ** 3 * 2.0 ** -50 * float(np.max(d * d)) * D["q"]
out["host"] = dict(n=N_HOST, perms=P_HOST, q=D["q"], host_s=round(th, 3), device_call_s=round(td, 4), host_flops=hflop / th,
                   host_device_gap_in_bars=float(np.max(np.abs(h["ss_perm"] - dev["ss_perm"])) / bar), same_p=bool(h["terms"][0]["p"] == dev["terms"][0]["p"]))
print(out["host"], flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "permanova_design_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
