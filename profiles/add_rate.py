"""Seconds per round of hmmufotu-amd-tree --add on one device: a random binary tree of 4,096 leaves (8,191 nodes),
rows evolved by `synth` down it (JC69, mean branch 0.05, 5 % of the cells turned into gaps), 7,682 columns as gg_97 has them, under
the HKY85 model of the golden files.  The queries are rows of the same tree's leaves with one base in ten changed (--queries=64,1024).
Two things are timed by the host clock around calls that end in a synchronise: hu_tree_add_scores, whose time less the sweep's is the
scoring of every (edge, query) with its copies (the sweep alone is timed by a call with one query), and, for the smaller number of
queries, hu_tree_add_search with the phases of hu_add_timing (the sweeps, the scoring, the fits) over its rounds.  The rate of the
scoring is given as (edge, query, column) triples per second and as the bytes of the edges' messages per second (64 bytes per edge and
column, read once per tile of HU_ADD_TILE queries).  --out=DIR: where the JSON goes."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


OUT = arg("out", os.path.join(ROOT, "profiles"))
N, L = int(arg("n", 4096)), int(arg("columns", 7682))
QS = [int(x) for x in arg("queries", "64,1024").split(",")]
SEARCH_Q = int(arg("search", QS[0]))
FIT_ROUNDS = int(arg("rounds", 3))
if E.device_count() < 1:
    sys.exit("add_rate: no gfx950 device")
m = synth.load_model("HKY85")
md = E.model_desc(m.type_id, m.pi, m.par)
rng = np.random.default_rng(97 + N)
parent, blen, is_leaf = synth.make_tree(N, rng)
seq = synth.evolve_sequences(parent, blen, L, synth.load_model("JC69"), np.ones(L), rng)
seq[rng.random(seq.shape) < 0.05] = -2
seq[~is_leaf] = -2
nodes = len(parent)
leaves = np.nonzero(is_leaf)[0]


def queries(q):
    rows = np.array(seq[rng.choice(leaves, q)])
    hit = rng.random(rows.shape) < 0.1
    rows[hit] = rng.integers(0, 4, rows.shape)[hit]
    return np.ascontiguousarray(rows, np.int8)


out = {"leaves": N, "nodes": nodes, "columns": L, "tile": E.ADD_TILE, "ratios_in_lds": L <= E.BLEN_LDS_COLS}
E.tree_add_scores(parent, blen, seq, queries(1), md)                       # warm-up: the code objects, the first allocations
t0 = time.perf_counter()
E.tree_add_scores(parent, blen, seq, queries(1), md)
one = time.perf_counter() - t0
out["sweep_and_one_query_s"] = round(one, 4)
for q in QS:
    qs = queries(q)
    t0 = time.perf_counter()
    r = E.tree_add_scores(parent, blen, seq, qs, md)
    call = time.perf_counter() - t0
    score = call - one
    triples = (nodes - 1) * q * L
    tiles = -(-q // E.ADD_TILE)
    rec = dict(queries=q, need_bytes=E.add_need(nodes, L, q), call_s=round(call, 4), scoring_s=round(score, 4), triples=triples, triples_per_s=triples / score,
               message_bytes=64 * (nodes - 1) * L * tiles, message_bytes_per_s=64 * (nodes - 1) * L * tiles / score,
               optima_at_min=int((r["best_t"] == 0).sum()), optima_at_max=int((r["best_t"] == 10).sum()))
    out["scores_q_%d" % q] = rec
    print(q, rec, flush=True)
    del r
if SEARCH_Q > 0:
    qs = queries(SEARCH_Q)
    t0 = time.perf_counter()
    r = E.tree_add_search(parent, blen, seq, qs, md, max_rounds=FIT_ROUNDS)
    call = time.perf_counter() - t0
    s = r["seconds"]; k = max(len(r["rounds"]), 1)
    out["search_q_%d" % SEARCH_Q] = dict(call_s=round(call, 3), rounds=r["rounds"], fit_rounds_asked=FIT_ROUNDS, ll_start=r["ll_start"], ll_final=r["ll_final"],
                                         sweep_s=round(s["sweep"], 4), score_s=round(s["score"], 4), fit_s=round(s["fit"], 4), other_s=round(s["other"], 4),
                                         sweep_s_per_round=s["sweep"] / k, score_s_per_round=s["score"] / k, fit_s_per_fit=s["fit"] / (k + 1))
    print("search", out["search_q_%d" % SEARCH_Q], flush=True)
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "add_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
