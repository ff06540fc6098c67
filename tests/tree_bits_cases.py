"""The cases of tests/test_tree_bits_gpu.py and of its generator (tests/make_tree_bits_golden.py): the smallest shapes at which the tree
family's device tests run every kernel instance, made by the generators of tests/test_tree_*.py, and the run that gives every result as
raw integers (a float as its 64 bits).

Per mode: the branch step and the NNI scores at 6 leaves x 63, 64 and 65 columns and at 12 leaves on either side of their switch from
ratios in LDS to ratios in global memory; the supports on either side of theirs, with replicate counts that are no multiple of a
thread's four; the SPR scores at four of their shapes, the far radius among them; the insertion scores on either side of the switch
with one query more than a tile, once with a slab and a tile of their own; and the small search of each of the three search tests."""
import os

import numpy as np

import test_tree_add as TA
import test_tree_blen as TB
import test_tree_nni as TN
import test_tree_spr as TS
import test_tree_support as TU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_bits")
SPR_SEARCH_RADIUS = 4


def _cases():
    E = TN.E
    out = []
    for n, L in ((6, 63), (6, 64), (6, 65), (12, E.BLEN_LDS_COLS), (12, E.BLEN_LDS_COLS + 1)):
        out.append(("step_%d_%d" % (n, L), "step", (n, L)))
    for n, L in ((6, 63), (6, 64), (6, 65), (12, E.NNI_LDS_COLS), (12, E.NNI_LDS_COLS + 1)):
        out.append(("nni_%d_%d" % (n, L), "nni", (n, L)))
    for n, L, B in ((5, E.SUPPORT_LDS_COLS, 33), (5, E.SUPPORT_LDS_COLS + 1, 257)):
        out.append(("support_%d_%d_%d" % (n, L, B), "support", (n, L, B)))
    for n, L, r in ((6, 64, 2), (9, 65, 3), (12, E.BLEN_LDS_COLS + 1, 2), (33, 255, 32)):
        out.append(("spr_%d_%d_%d" % (n, L, r), "spr", (n, L, r)))
    for n, L, nq, kw in ((5, E.BLEN_LDS_COLS, TA.TILE + 1, {}), (5, E.BLEN_LDS_COLS + 1, TA.TILE + 1, {}),
                         (5, E.BLEN_LDS_COLS + 1, TA.TILE + 1, dict(slab=5, tile=3))):
        out.append(("add_%d_%d_%d%s" % (n, L, nq, "_slab5_tile3" if kw else ""), "add", (n, L, nq, kw)))
    out += [("nni_search", "nni_search", ()), ("spr_search", "spr_search", ()), ("add_search", "add_search", ())]
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
SEARCHES = ("nni_search", "spr_search", "add_search")


def golden_path(name, root=None):
    return os.path.join(root or GOLDEN, name + ".npz")


def _bits(x):
    """floats as their 64 bits, everything else as the integers it is"""
    a = np.ascontiguousarray(np.atleast_1d(x))
    return a.view(np.int64) if a.dtype == np.float64 else a


def _search_out(r, stop, moves):
    return dict(parent=r["parent"], blen=r["blen"], ll_final=np.float64(r["ll_final"]), stop=np.int32(stop),
                moves=np.array(moves, np.int32).reshape(len(moves), -1), n_rounds=np.int32(len(r["rounds"])))


def run_case(E, name, host):
    """the results of case `name` as {field: integer array}, by the device or by the library's host path"""
    _, mode, arg = CASES[CASE_IDS.index(name)]
    if mode == "step":
        c = TB.device_case(*arg)
        got = E.tree_branch_step(c.parent, c.start, c.seq, c.md, min_len=c.min_len, max_len=c.max_len, host=host)
        got = {k: got[k] for k in ("t_star", "f", "d1", "d2", "capped")}
    elif mode == "nni":
        got = TN.scores(TN.device_case(*arg), host=host)
        got = {k: got[k] for k in ("edge_node", "t_star", "f", "f0_at_blen")}
    elif mode == "support":
        got = TU.support(TN.device_case(*arg[:2]), host=host, B=arg[2])
        got = {k: got[k] for k in ("edge_node", "t_star", "f", "count", "sums")}
    elif mode == "spr":
        got = TS.scores(TS.device_case(*arg[:2]), host, arg[2])
        got = {k: got[k] for k in ("prune_node", "v_off", "base_t", "base_f", "f_at_blen", "target_node", "dist", "t_star", "f")}
    elif mode == "add":
        got = TA.scores(TA.device_case(*arg[:3]), host, **arg[3])
    elif mode == "nni_search":
        c = TN.search_case()
        r = E.tree_nni_search(c.parent, c.start, c.seq, c.md, host=host)
        got = _search_out(r, E.NNI_STOP.index(r["stop"]), r["swaps"])
    elif mode == "spr_search":
        c = TS.spr_search_case()
        r = E.tree_spr_search(c.parent, c.start, c.seq, c.md, radius=SPR_SEARCH_RADIUS, host=host)
        got = _search_out(r, E.SPR_STOP.index(r["stop"]), r["moves"])
    else:
        c = TA.search_case()
        r = E.tree_add_search(c.parent, c.start, c.seq, c.q, c.md, host=host)
        got = _search_out(r, 0, [(i["round"], i["query"], i["v"], i["w"]) for i in r["inserts"]])
        got.update(insert_t=np.array([i["t"] for i in r["inserts"]]), insert_f=np.array([i["f"] for i in r["inserts"]]),
                   query_node=r["query_node"])
    return {k: _bits(v) for k, v in got.items()}


def reaches(name, got):
    """why the results `got` of case `name` do not reach the code the case is there for, or None: a score case needs a t_star that left
    its start and one that lies inside the bounds (a Newton loop that iterated and ended on its own), a search an accepted round"""
    _, mode, arg = CASES[CASE_IDS.index(name)]
    if mode in SEARCHES:
        if int(got["n_rounds"][0]) < 1 or len(got["moves"]) < 1:
            return "no accepted round"
        return None
    c = {"step": TB.device_case, "nni": TN.device_case, "support": TN.device_case, "spr": TS.device_case}.get(mode, TA.device_case)(*arg[:3 if mode == "add" else 2])
    t = got["t_star"].view(np.float64)
    starts = np.asarray(c.start, np.float64)
    if mode == "step":
        t = t[1:]                                               # branch by branch; the root has none
        moved = np.abs(t - starts[1:]) > 1e-9
    else:                                                       # a start is one of the tree's lengths, or their mean (a new pendant)
        if mode == "add":
            t = t[:, np.asarray(c.parent) >= 0]
            starts = np.append(starts, TA.mean_len(c.parent, c.start, c.min_len, c.max_len))
        t = t.reshape(-1)
        moved = (np.abs(t[None, :] - starts[:, None]) > 1e-9).all(axis=0)
    if t.size == 0:
        return "no t_star at all"
    if not moved.any():
        return "no t_star that differs from its start"
    if not ((t > c.min_len) & (t < c.max_len)).any():
        return "every t_star at a bound"
    return None
