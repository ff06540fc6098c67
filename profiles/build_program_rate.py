"""hmmufotu-amd-build at scale on one device, and the writer A/B.

Input: the tree and leaf rows of synth_gpu.make_db_gpu written out as FASTA and Newick.  Default: gg_97 scale (99,322 leaves x 7,682
columns as read, ~1,400 of them dense; the .ptu is then ~99 GB, so --tmp must name a file system with that much room).  --quick: 20,000
leaves x 1,486 columns (a 3.8 GB .ptu).

1. The program with -V -vv: its own wall time per phase (read, join, stats, first sweep, mutation count, second sweep, log-likelihood,
   write) from the "[phase]" lines, and the device's peak used memory (hipMemGetInfo through torch.cuda.mem_get_info, polled from a
   thread while the program runs: it sees the program's own allocations, which no allocator statistic of this process would).
2. The writer A/B on the same device buffers and the same target file system: hu_ptu_write (one blocking copy per directed edge) against
   hu_ptu_write_stream (k_ptu_gather + two staging buffers), three alternating runs each, file removed between runs.  Decision rule: the
   pipeline stays only if its median is below the plain loop's by more than the spread (max - min) of the three runs.
   --writer-only --once runs each writer once and nothing else: the form to put behind
   `rocprofv3 --kernel-trace --memory-copy-trace --stats --` for the split into gather, copy and host write.

--out=DIR: where build_program_rate.json goes (default profiles/).  --tmp=DIR: where the inputs and the .ptu files are written."""
import json, os, subprocess, sys, tempfile, threading, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth, synth_gpu
arg = lambda k, d=None: next((a.split("=", 1)[1] for a in sys.argv if a.startswith(k + "=")), d)
OUT = arg("--out", os.path.join(ROOT, "profiles"))
QUICK, WRITER_ONLY, ONCE = "--quick" in sys.argv, "--writer-only" in sys.argv, "--once" in sys.argv
N_LEAVES, L = (20000, 1486) if QUICK else (99322, 7682)
TMP = arg("--tmp") or tempfile.mkdtemp(prefix="hu_build_rate_")
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-build")
SM = os.path.join(ROOT, "tests", "golden", "ref_data", "gg_97_otus_GTR.sm")
out = {"device": torch.cuda.get_device_name(0), "quick": QUICK, "n_leaves": N_LEAVES, "cs_len_as_read": L, "target_dir": TMP}


def newick_of(parent, blen, names):
    """Newick text of a parent array, written without recursion"""
    n = len(parent)
    kids = [[] for _ in range(n)]
    for u in range(1, n):
        kids[parent[u]].append(u)
    parts, stack = [], [(0, 0)]
    while stack:
        u, k = stack.pop()
        if k == 0 and kids[u]:
            parts.append("(")
        if k < len(kids[u]):
            if k:
                parts.append(",")
            stack.append((u, k + 1)); stack.append((kids[u][k], 0))
            continue
        if kids[u]:
            parts.append(")")
        parts.append(names[u] if not kids[u] else "")
        if u:
            parts.append(":%.6g" % blen[u])
    return "".join(parts) + ";\n"


def peak_used_gb(f):
    free0, total = torch.cuda.mem_get_info(0)
    low, done = [free0], threading.Event()

    def poll():
        while not done.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info(0)[0]); time.sleep(2e-3)
    t = threading.Thread(target=poll); t.start()
    try:
        r = f()
    finally:
        done.set(); t.join()
    return r, round((total - low[0]) / 1e9, 2), round((total - free0) / 1e9, 2)


db, up, down = synth_gpu.make_db_gpu(N_LEAVES, L, "GTR", dg_k=0)
n = db.n_nodes
parent, blen, seq, height = db.parent, db.blen, db.seq, db.height
md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, None)
out.update(n_nodes=n, message_gb=round(2 * n * L * 32 / 1e9, 2))

if not WRITER_ONLY:
    del up, down
    torch.cuda.empty_cache()
    names = ["s%d" % u for u in range(n)]
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(os.path.join(TMP, "in.fasta"), "wb") as f:
        for u in np.nonzero(db.is_leaf)[0]:
            row = np.where(seq[u] >= 0, lut[np.maximum(seq[u], 0)], ord("-")).astype(np.uint8)
            f.write(b">" + names[u].encode() + b"\n" + row.tobytes() + b"\n")
    with open(os.path.join(TMP, "in.tree"), "w") as f:
        f.write(newick_of(parent, blen, names))
    cmd = [BIN, "in.fasta", "in.tree", "--no-hmm", "-sm", SM, "-V", "-n", "built", "-vv"]
    t0 = time.perf_counter()
    r, peak, before = peak_used_gb(lambda: subprocess.run(cmd, cwd=TMP, capture_output=True, text=True))
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("hmmufotu-amd-build failed: " + r.stderr[-2000:])
    phases = {ln.split("] ", 1)[1].rsplit(":", 1)[0]: float(ln.rsplit(":", 1)[1].split()[0]) for ln in r.stderr.split("\n") if ln.startswith("[phase] ")}
    out["program"] = dict(wall_s=round(wall, 2), phase_s=phases, ptu_gb=round(os.path.getsize(os.path.join(TMP, "built.ptu")) / 1e9, 2),
                          device_used_gb_before=before, device_used_gb_peak=peak,
                          loglik_line=next((ln for ln in r.stderr.split("\n") if ln.startswith("Final Tree")), ""),
                          alpha_line=next((ln for ln in r.stderr.split("\n") if ln.startswith("Estimated alpha")), ""))
    for fn in ("built.ptu", "in.fasta"):
        os.remove(os.path.join(TMP, fn))
    up = torch.empty((n, L, 4), dtype=torch.float64, device="cuda:0"); down = torch.zeros_like(up)
    leaf_only = np.where(db.is_leaf[:, None], seq, 0).astype(np.int8)
    seq, height = E.tree_evaluate(parent, blen, leaf_only, md, up.data_ptr(), down.data_ptr())
    torch.cuda.synchronize()

# ---- writer A/B: the same buffers, the same file system, alternating
path = os.path.join(TMP, "ab.ptu")
kw = dict(model_text=db.model.text, msgs_on_device=True)
writers = {"ptu_write": lambda: E.write_ptu(path, parent, blen, seq, up.data_ptr(), down.data_ptr(), height, md, **kw),
           "ptu_write_stream": lambda: E.write_ptu_stream(path, parent, blen, seq, up.data_ptr(), down.data_ptr(), height, md, **kw)}
times = {k: [] for k in writers}
for rep in range(1 if ONCE else 3):
    for k, f in writers.items():
        t0 = time.perf_counter(); f(); times[k].append(round(time.perf_counter() - t0, 3))
        size = os.path.getsize(path); os.remove(path)
med = {k: float(np.median(v)) for k, v in times.items()}
spread = max(max(v) - min(v) for v in times.values())
out["writer_ab"] = dict(file_gb=round(size / 1e9, 2), s=times, median_s=med, spread_s=round(spread, 3),
                        pipeline_stays=bool(med["ptu_write_stream"] < med["ptu_write"] - spread))
if not ONCE:
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "build_program_rate.json"), "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
