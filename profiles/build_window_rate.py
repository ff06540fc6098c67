"""hmmufotu-amd-build --col-window against the resident build at scale on one device.

Input: the tree and leaf rows of synth_gpu.make_db_gpu written out as FASTA and Newick, as profiles/build_program_rate.py makes them.
Default: gg_97 scale (99,322 leaves x 7,682 columns as read; the .ptu is ~99 GB, so --tmp must name a file system with that much
room).  --quick: 20,000 leaves x 1,486 columns (a 3.8 GB .ptu).

Four configurations of the same command (-V -vv): resident, and --col-window L/2, L/4, L/8 with L the column count after pruning
(taken from the resident build's file).  Three rounds, each running the four in turn, so that every configuration meets the same drift
of a shared host and file system; the file is removed after each run.  Per run: the program's own wall time per phase (its "[phase]"
lines), the whole wall time, the device's peak used memory (hipMemGetInfo through torch.cuda.mem_get_info, polled from a thread while
the program runs), and whether the .ptu equals the resident one byte for byte (compared once per configuration, in the first round).
Reported: medians, the spread (max - min) of each configuration, and the ratio of every windowed median to the resident median; a
ratio inside the spread is no difference.  A measurement path that finds no device fails.

--out=DIR: where build_window_rate.json goes (default profiles/).  --tmp=DIR: where the inputs and the .ptu files are written."""
import filecmp, json, os, subprocess, sys, tempfile, threading, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth_gpu
arg = lambda k, d=None: next((a.split("=", 1)[1] for a in sys.argv if a.startswith(k + "=")), d)
OUT = arg("--out", os.path.join(ROOT, "profiles"))
QUICK = "--quick" in sys.argv
N_LEAVES, L_READ = (20000, 1486) if QUICK else (99322, 7682)
TMP = arg("--tmp") or tempfile.mkdtemp(prefix="hu_build_window_")
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-build")
SM = os.path.join(ROOT, "tests", "golden", "ref_data", "gg_97_otus_GTR.sm")
if not torch.cuda.is_available():
    sys.exit("build_window_rate.py needs a gfx950 device")
out = {"device": torch.cuda.get_device_name(0), "quick": QUICK, "n_leaves": N_LEAVES, "cs_len_as_read": L_READ}


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


db, up, down = synth_gpu.make_db_gpu(N_LEAVES, L_READ, "GTR", dg_k=0)
n = db.n_nodes
del up, down
torch.cuda.empty_cache()
names = ["s%d" % u for u in range(n)]
lut = np.frombuffer(b"ACGT", np.uint8)
with open(os.path.join(TMP, "in.fasta"), "wb") as f:
    for u in np.nonzero(db.is_leaf)[0]:
        row = np.where(db.seq[u] >= 0, lut[np.maximum(db.seq[u], 0)], ord("-")).astype(np.uint8)
        f.write(b">" + names[u].encode() + b"\n" + row.tobytes() + b"\n")
with open(os.path.join(TMP, "in.tree"), "w") as f:
    f.write(newick_of(db.parent, db.blen, names))
out["n_nodes"] = n


def run(name, extra):
    cmd = [BIN, "in.fasta", "in.tree", "--no-hmm", "-sm", SM, "-V", "-n", name, "-vv"] + extra
    t0 = time.perf_counter()
    r, peak, before = peak_used_gb(lambda: subprocess.run(cmd, cwd=TMP, capture_output=True, text=True))
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        sys.exit("hmmufotu-amd-build %s failed: %s" % (" ".join(extra), r.stderr[-2000:]))
    lines = r.stderr.split("\n")
    phases = {ln.split("] ", 1)[1].rsplit(":", 1)[0]: float(ln.rsplit(":", 1)[1].split()[0]) for ln in lines if ln.startswith("[phase] ")}
    return dict(wall_s=round(wall, 2), phase_s=phases, device_used_gb_before=before, device_used_gb_peak=peak,
                windows_line=next((ln for ln in lines if ln.startswith("Building in ")), ""),
                loglik_line=next((ln for ln in lines if ln.startswith("Final Tree")), ""),
                alpha_line=next((ln for ln in lines if ln.startswith("Estimated alpha")), ""))


ptu = lambda name: os.path.join(TMP, name + ".ptu")
first = run("resident", [])                                  # kept through the first round: the file the windowed ones are compared with
L = E.tree_info(ptu("resident"))["cs_len"]
configs = [("resident", [])] + [("window_L/%d" % d, ["--col-window", str(-(-L // d))]) for d in (2, 4, 8)]
out.update(cs_len=L, message_gb=round(2 * n * L * 32 / 1e9, 2), ptu_gb=round(os.path.getsize(ptu("resident")) / 1e9, 2),
           need_gb={k: round(E.build_window_need(n, int(x[1]), True) / 1e9, 2) for k, x in configs[1:]})
runs = {k: [] for k, _ in configs}
same = {}
for rnd in range(3):
    for k, extra in configs:
        if rnd == 0 and k == "resident":
            runs[k].append(first)
            continue
        r = run("cur", extra)
        if rnd == 0:
            same[k] = filecmp.cmp(ptu("resident"), ptu("cur"), shallow=False) and r["loglik_line"] == first["loglik_line"]
        os.remove(ptu("cur"))
        runs[k].append(r)
    if rnd == 0:
        os.remove(ptu("resident"))
med = {k: float(np.median([r["wall_s"] for r in v])) for k, v in runs.items()}
spread = {k: round(max(r["wall_s"] for r in v) - min(r["wall_s"] for r in v), 2) for k, v in runs.items()}
out.update(runs=runs, equal_to_resident=same, median_wall_s=med, spread_wall_s=spread,
           peak_gb={k: max(r["device_used_gb_peak"] for r in v) for k, v in runs.items()},
           ratio_to_resident={k: round(med[k] / med["resident"], 3) for k in med if k != "resident"})
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "build_window_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
