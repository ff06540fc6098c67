"""Rate of hu_pcoa on one device.  The fixture is permanova's: the Euclidean distances of n random points in 8
dimensions (fixed seed), n = 4,096 and 16,384, k = 3 with the default oversampling.  Such a matrix has 8 positive axes, so k = 10 runs on
points in 16 dimensions.  Both converge in two iterations (the block is wider than the matrix's rank), which is three launches of the
product kernel: too short a window for a rate.  So a third case per size times the product kernel over dozens of launches: points in 8
dimensions whose axes are scaled 2^(-j/2), k = 3 and no oversampling, where the block of 3 columns converges like 2^-it.
One warm-up and three timed calls each, timed end to end by the host clock (a call checks the matrix and computes the trace on the host,
and ends in the copy back) and split by hu_pcoa_timing.  The product kernel's time is a host clock around a synchronise, summed over
its launches: iterations + 1 (the certificate).  Its bytes are the squares alone, 8 n^2 per launch; its flop 2 n^2 mp per launch.
Context, not a bar (they are other algorithms or other hardware): the host path (one thread) and a full numpy.linalg.eigh at the first size.
--out=DIR: where the JSON goes; --sizes=A,B: smaller sizes for a rehearsal; --context=0: without the host path and eigh; --name=X: the file's name."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E

HBM_PEAK = 8.0e12      # bytes per second, MI355X


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


def matrix(n, seed, dims=8, decay=0.0):
    x = np.random.default_rng(seed).normal(size=(n, dims)) * 2.0 ** (-decay * np.arange(dims))
    sq = (x * x).sum(1)
    d = np.empty((n, n))
    for i0 in range(0, n, 1024):
        b = sq[i0:i0 + 1024, None] + sq[None, :] - 2.0 * (x[i0:i0 + 1024] @ x.T)
        d[i0:i0 + 1024] = np.sqrt(np.maximum(b, 0.0))
    d = np.triu(d, 1)
    return d + d.T


OUT = arg("out", os.path.join(ROOT, "profiles"))
SIZES = [int(v) for v in arg("sizes", "4096,16384").split(",")]
CONTEXT = int(arg("context", 1))
if E.device_count() < 1:
    sys.exit("pcoa_rate: no gfx950 device")
out = {"hbm_peak_bytes_per_s": HBM_PEAK}
for n in SIZES:
    for name, k, over, dims, decay in (("k3", 3, 8, 8, 0.0), ("k10", 10, 8, 16, 0.0), ("window", 3, 0, 8, 0.5), ("wide", 3, 61, 128, 0.0625)):
        d = matrix(n, 27, dims, decay)
        ts = []; phases = []
        for it in range(4):
            t0 = time.perf_counter(); r = E.pcoa(d, k=k, oversample=over); dt = time.perf_counter() - t0
            if it:
                ts.append(dt); phases.append(E.pcoa_timing())
            else:
                first = r
            assert r["coords"].tobytes() == first["coords"].tobytes() and r["iterations"] == first["iterations"]
        launches = r["iterations"] + 1
        mp = -(-r["m_final"] // 16) * 16
        prod = [p["product"] / launches for p in phases]
        res = dict(n=n, k=k, oversample=over, dims=dims, m=r["m_final"], mp=mp, slabs=E.pcoa_slabs(n), iterations=r["iterations"], product_launches=launches,
                   worst_resid_over_lambda1=float(r["resid"].max() / r["eigval"][0]), need_bytes=E.pcoa_need(n, k, over), call_s=[round(t, 4) for t in ts],
                   **{f + "_s": [round(float(p[f]), 5) for p in phases] for f in ("to_device", "square", "product", "small", "host_mxm", "to_host")},
                   product_s_per_launch=[round(float(t), 7) for t in prod], product_bytes_per_s=float(8.0 * n * n / min(prod)), product_share_of_hbm_peak=float(8.0 * n * n / min(prod) / HBM_PEAK),
                   product_flop_per_s=float(2.0 * n * n * mp / min(prod)))
        out["n_%d_%s" % (n, name)] = res
        print(res, flush=True)
if CONTEXT:
    n = SIZES[0]
    d = matrix(n, 27)
    t0 = time.perf_counter(); h = E.pcoa(d, k=3, host=True); th = time.perf_counter() - t0
    J = np.eye(n) - 1.0 / n
    t0 = time.perf_counter(); w = np.linalg.eigh(-0.5 * J @ (d * d) @ J)[0]; te = time.perf_counter() - t0
    dev = E.pcoa(d, k=3)
    out["context"] = dict(n=n, host_path_s=round(th, 3), host_iterations=h["iterations"], numpy_eigh_s=round(te, 3), numpy_threads=os.environ.get("OMP_NUM_THREADS"),
                          host_equals_device_bits=bool(h["coords"].tobytes() == dev["coords"].tobytes()),
                          eigenvalues_off_eigh_over_lambda1=float(np.abs(dev["eigval"] - w[::-1][:3]).max() / w[-1]))
    print(out["context"], flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, arg("name", "pcoa_rate.json")), "w") as f:
    json.dump(out, f, indent=1)
