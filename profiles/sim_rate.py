"""Rates of the read simulation on one device.

Library: a gg_97-scale synthetic database (99,322 leaves, 198,643 nodes x 7,682 columns, GTR; --leaves=N for another size), the gap
fractions from its own leaf rows (hu_sim_gap_frac), a plan of 65,536 reads of about 500 columns (hu_sim_plan, host), then hu_sim_reads:
one warm-up call, five timed calls with mates.  Reported per call: the wall time around the call (copies and the conversion to Python
strings included), the phases the entry times itself (hu_sim_timing: allocation and copies to the device, the kernel up to its
synchronise, the copies back), reads/s and sites/s of the kernel phase and of the whole entry, and the kernel's bytes per second two ways:
64 B for every site (what it must read if no site were a gap) and 64 B for every site that was not drawn as a gap (what it does load:
a gap site reads its 8-byte gap fraction alone).  Most columns of the synthetic alignment are 99.9 % gaps, as in gg_97.

Program: a database of 2,001 leaves written to a temporary directory (the whole-size one is 98 GB of messages), hmmufotu-amd-sim
with -N 1 (start-up and database load) and with -N 262144, single-end and paired: the difference is planning, simulation and FASTA.
--out=DIR: where sim_rate.json goes (default profiles/).  --quick: 2,001 leaves for the library part too."""
import json, os, subprocess, sys, tempfile, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth, synth_gpu
OUT = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--out=")), os.path.join(ROOT, "profiles"))
quick = "--quick" in sys.argv
N_LEAVES = int(next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--leaves=")), 2001 if quick else 99322))
L, R, N_PROG, SMALL = 7682, 65536, 262144, 2001
BIN = os.path.join(ROOT, "hmmufotu_amd", "bin", "hmmufotu-amd-sim")
out = {"device": torch.cuda.get_device_name(0)}

# ---- the program, on a database small enough to write
with tempfile.TemporaryDirectory() as tmp:
    db, up, down = synth_gpu.make_db_gpu(SMALL, L, "GTR", dg_k=0, seed=97, device="cuda:0", log=lambda *a: None)
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par)
    pre = os.path.join(tmp, "db")
    synth.write_hmm(db.hmm, pre + ".hmm")
    E.write_ptu_stream(pre + ".ptu", db.parent, db.blen, db.seq, up.data_ptr(), down.data_ptr(), db.height, md, model_text=db.model.text, msgs_on_device=True)
    del up, down
    torch.cuda.empty_cache()
    prog = dict(nodes=int(db.n_nodes), cs_len=L, ptu_bytes=os.path.getsize(pre + ".ptu"), reads=N_PROG)

    def timed(args):
        t0 = time.perf_counter()
        r = subprocess.run(["timeout", "-k", "10", "600", BIN, pre] + args + ["-S", "7"], cwd=tmp, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("hmmufotu-amd-sim failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        return time.perf_counter() - t0
    t1 = timed(["one.fa", "-N", "1"])
    ts = timed(["se.fa", "-N", str(N_PROG)]); tp = timed(["p1.fa", "p2.fa", "-N", str(N_PROG), "-r", "250"])
    prog.update(start_and_load_s=round(t1, 3), single_end_s=round(ts, 3), paired_s=round(tp, 3), fasta_bytes_single_end=os.path.getsize(os.path.join(tmp, "se.fa")),
                single_end_reads_per_s_after_load=round(N_PROG / max(ts - t1, 1e-9), 1), paired_pairs_per_s_after_load=round(N_PROG / max(tp - t1, 1e-9), 1))
    out["program"] = prog

# ---- the library at scale
t0 = time.time()
db, up, down = synth_gpu.make_db_gpu(N_LEAVES, L, "GTR", dg_k=0, seed=97, device="cuda:0", log=lambda *a: None)
md = E.model_desc(db.model.type_id, db.model.pi, db.model.par)
D = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, up.data_ptr(), down.data_ptr(), db.height, md, msgs_on_device=True)
out["db"] = dict(nodes=D.n_nodes, cs_len=D.cs_len, message_bytes=2 * D.n_nodes * D.cs_len * 32, build_s=round(time.time() - t0, 1))
t1 = time.perf_counter(); gf = D.sim_gap_frac(); t2 = time.perf_counter()
plan = D.sim_plan(R, 7); t3 = time.perf_counter()
cols = (plan["end"] - plan["start"] + 1).astype(np.int64)
out["gap_frac_s"] = round(t2 - t1, 3); out["gap_frac_mean"] = round(float(gf.mean()), 4)
out["plan"] = dict(reads=R, s=round(t3 - t2, 4), reads_per_s=round(R / (t3 - t2), 1), columns_mean=round(float(cols.mean()), 1))
D.sim_reads({k: v[:1024] for k, v in plan.items()}, gf, 7, mate=True)                 # warm-up: the code object, first allocations
calls = []
for i in range(5):
    t1 = time.perf_counter(); got = D.sim_reads(plan, gf, 7, read0=i * R, mate=True); w = time.perf_counter() - t1
    ph = E.sim_timing()
    calls.append(dict(wall_s=round(w, 4), to_device_s=round(ph["to_device"], 5), kernel_s=round(ph["kernel"], 6), to_host_s=round(ph["to_host"], 5),
                      residues=int(got["seq_len"].sum())))
k = float(np.median([c["kernel_s"] for c in calls])); entry = float(np.median([c["to_device_s"] + c["kernel_s"] + c["to_host_s"] for c in calls]))
sites = int(cols.sum()); res = int(np.median([c["residues"] for c in calls]))
out["sim_reads"] = dict(reads=R, sites=sites, residues_median=res, calls=calls, kernel_s_median=k, entry_s_median=round(entry, 5),
                        wall_s_median=round(float(np.median([c["wall_s"] for c in calls])), 4),
                        kernel_reads_per_s=round(R / k, 1), kernel_sites_per_s=round(sites / k, 1), entry_reads_per_s=round(R / entry, 1), entry_sites_per_s=round(sites / entry, 1),
                        kernel_gb_per_s_at_64B_per_site=round(64 * sites / k / 1e9, 1), kernel_gb_per_s_at_64B_per_residue=round(64 * res / k / 1e9, 1),
                        note="kernel_s is a host clock from the launch to the end of hipDeviceSynchronize: launch latency included")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "sim_rate%s.json" % ("_quick" if quick else "")), "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
