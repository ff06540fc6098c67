"""Rate of hu_unifrac at gg_97 scale on one device: a synth tree of 198,643 nodes (parents and lengths only, handed
to the library as arrays), 2,048 samples of 2,000 reads each, every read on a node drawn uniformly from the whole tree (leaves and inner
nodes) with a fixed seed, so a sample holds a little under 2,000 OTUs.  `weighted` and `unweighted`: one warm-up and three timed calls
each, timed end to end by the host clock (every call ends in a device synchronise and the copy back) and split by hu_unifrac_timing
into copies up, embedding, pair kernels (k_unifrac_pairs + k_unifrac_finish, host clock around a synchronise) and copy back.  A term is one
(pair, branch): S (S - 1) / 2 x B of them, the diagonal tiles' wasted half not counted.  The same table cut to its first 256 samples
goes through the host path (one thread) once per method, so the ratio is a measured one against code that is not the kernel.
--out=DIR: where the JSON goes; --samples=N, --host-samples=N, --leaves=N: smaller sizes for a rehearsal."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
N_LEAVES, S, S_HOST, READS = int(arg("leaves", 99322)), int(arg("samples", 2048)), int(arg("host-samples", 256)), 2000
if E.device_count() < 1:
    sys.exit("unifrac_rate: no gfx950 device")
rng = np.random.default_rng(97)
parent, blen, _ = synth.make_tree(N_LEAVES, rng)
n = len(parent)
counts = np.zeros((n, S))
for j in range(S):
    np.add.at(counts[:, j], rng.integers(0, n, READS), 1.0)
rows = np.nonzero(counts.sum(1))[0]
counts = np.ascontiguousarray(counts[rows]); nodes = rows.astype(np.int32)
out = {"n_nodes": n, "samples": S, "reads_per_sample": READS, "otus": len(rows), "otus_per_sample_mean": float((counts > 0).sum(0).mean())}
print(out, flush=True)
for method in ("weighted", "unweighted"):
    r = {}
    ts = []; phases = []
    for it in range(4):
        t0 = time.perf_counter(); d = E.unifrac(counts, nodes, parent, blen, method=method); dt = time.perf_counter() - t0
        if it:
            ts.append(dt); phases.append(E.unifrac_timing())
        else:
            first = d.copy()
        assert d.tobytes() == first.tobytes()
    B = len(E.unifrac_embed(counts[:, :1], nodes, parent, blen, host=True)["node"])
    terms = S * (S - 1) // 2 * B
    best = min(phases, key=lambda p: p["pairs"])
    r.update(B=B, L=E.unifrac_default_slab(S, B), tiles=(-(-S // 64)) * (-(-S // 64) + 1) // 2, terms=terms, call_s=[round(t, 4) for t in ts],
             to_device_s=[round(p["to_device"], 4) for p in phases], embed_s=[round(p["embed"], 4) for p in phases],
             pairs_s=[round(p["pairs"], 4) for p in phases], to_host_s=[round(p["to_host"], 4) for p in phases],
             terms_per_s_pairs=terms / best["pairs"], terms_per_s_call=terms / min(ts))
    sub = np.ascontiguousarray(counts[:, :S_HOST])
    t0 = time.perf_counter(); h = E.unifrac(sub, nodes, parent, blen, method=method, host=True, slab=r["L"]); th = time.perf_counter() - t0
    hterms = S_HOST * (S_HOST - 1) // 2 * B
    dsub = E.unifrac(sub, nodes, parent, blen, method=method, slab=r["L"])
    r.update(host_samples=S_HOST, host_s=round(th, 3), host_terms_per_s=hterms / th, host_equals_device_bits=bool(h.tobytes() == dsub.tobytes()),
             pairs_rate_over_host_rate=(terms / best["pairs"]) / (hterms / th))
    out[method] = r
    print(method, r, flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "unifrac_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
