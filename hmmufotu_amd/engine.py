"""ctypes host binding of libhmmufotu_amd.so (include/hmmufotu_amd.h).

The Python side mirrors the per-read surface of the reference (src/HmmUFOtu_main.h:70-113):
`Batch.align / get_seed / estimate_seq / filter_placements / place_seq / calc_q_values`
operate on a whole batch of reads.  There is no CPU fallback: `load_library()` raises if the
HIP extension is missing and every compute call raises `EngineError` without a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HU_LIB") or os.path.join(_HERE, "libhmmufotu_amd.so")      # HU_LIB: another build of the same library (kernel-geometry experiments)
_LIB = None

HU_MAX_SEEDS = 64
T_NAMES = ["viterbi", "align_build", "seed_pdist", "seed_topk", "estimate", "place", "_6", "_7"]
MODE = {"global": 0, "local": 1, "ngcl": 2, "cgnl": 3}


class EngineError(RuntimeError):
    pass


class ProfileDesc(C.Structure):
    _fields_ = [("K", C.c_int32), ("L", C.c_int32), ("EM", C.POINTER(C.c_double)), ("EI", C.POINTER(C.c_double)),
                ("T", C.POINTER(C.c_double)), ("p2cs", C.POINTER(C.c_int32))]


class ModelDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("pi", C.c_double * 4), ("par", C.c_double * 16), ("dg_k", C.c_int32),
                ("dg_rate", C.c_double * 16)]


class TreeDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("cs_len", C.c_int32), ("parent", C.POINTER(C.c_int32)), ("blen", C.POINTER(C.c_double)),
                ("seq", C.POINTER(C.c_int8)), ("up", C.c_void_p), ("down", C.c_void_p), ("height", C.POINTER(C.c_double)),
                ("anno_id", C.POINTER(C.c_int32)), ("anno_dist", C.POINTER(C.c_double)), ("win_start", C.c_int64),
                ("win_len", C.c_int64), ("msgs_on_device", C.c_int32)]


class Opts(C.Structure):
    _fields_ = [("align_mode", C.c_int32), ("max_nseed", C.c_int32), ("max_diff", C.c_double), ("max_height", C.c_double),
                ("max_error", C.c_double), ("weighted", C.c_int32), ("only_ml", C.c_int32), ("prior", C.c_int32),
                ("ignore_orient", C.c_int32), ("fix_root_loglik", C.c_int32), ("seed_order", C.c_int32)]


class AlignRec(C.Structure):
    _fields_ = [("seq_start", C.c_int32), ("seq_end", C.c_int32), ("hmm_start", C.c_int32), ("hmm_end", C.c_int32),
                ("cs_start", C.c_int32), ("cs_end", C.c_int32), ("status", C.c_int32), ("used_full", C.c_int32), ("cost", C.c_double)]


class PlaceRec(C.Structure):
    _fields_ = [("c_node", C.c_int32), ("p_node", C.c_int32), ("a_node", C.c_int32), ("n_cand", C.c_int32),
                ("wuv", C.c_double), ("ratio", C.c_double), ("wnr", C.c_double), ("loglik", C.c_double), ("height", C.c_double),
                ("q_place", C.c_double), ("q_taxon", C.c_double), ("anno_dist", C.c_double), ("est_loglik", C.c_double),
                ("root_loglik", C.c_double)]


READ_OK, READ_INVALID, READ_CHIMERA, READ_OUT_OF_WINDOW = 1, 0, 2, 16     # hu_align_rec.status (HU_READ_*)
ALIGN_DTYPE = np.dtype([("seq_start", "i4"), ("seq_end", "i4"), ("hmm_start", "i4"), ("hmm_end", "i4"), ("cs_start", "i4"),
                        ("cs_end", "i4"), ("status", "i4"), ("used_full", "i4"), ("cost", "f8")])
PLACE_DTYPE = np.dtype([("c_node", "i4"), ("p_node", "i4"), ("a_node", "i4"), ("n_cand", "i4"), ("wuv", "f8"), ("ratio", "f8"),
                        ("wnr", "f8"), ("loglik", "f8"), ("height", "f8"), ("q_place", "f8"), ("q_taxon", "f8"),
                        ("anno_dist", "f8"), ("est_loglik", "f8"), ("root_loglik", "f8")])


class ChimeraOpts(C.Structure):
    _fields_ = [("num_seg", C.c_int32), ("reserved", C.c_int32), ("max_chimera_error", C.c_double), ("min_chimera_lod", C.c_double)]


CHIMERA_DTYPE = np.dtype([("checked", "i4"), ("is_chimera", "i4"), ("seg5_start", "i4"), ("seg5_end", "i4"), ("seg3_start", "i4"),
                          ("seg3_end", "i4"), ("n_seg5", "i4"), ("n_seg3", "i4"), ("seg5", PLACE_DTYPE), ("seg3", PLACE_DTYPE),
                          ("alt5_loglik", "f8"), ("alt3_loglik", "f8"), ("lod", "f8")])


def build_library(force: bool = False) -> str:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".hip", ".cpp", ".h"))]
    deps.append(os.path.join(os.path.dirname(_HERE), "include", "hmmufotu_amd.h"))
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps):
        subprocess.check_call(["make", "-C", src, "-B", "all"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise EngineError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % LIB_PATH)
        # One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64.so (same soname as the system one),
        # and a process that has both mapped sees the GPU from only the first.  Map torch's copy first (without importing
        # torch) so that the engine binds to it whichever of the two is imported first.
        try:
            import importlib.util
            spec = importlib.util.find_spec("torch")
            hip = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else ""
            if hip and os.path.exists(hip):
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
        except OSError:
            pass
        _LIB = C.CDLL(LIB_PATH)
        _LIB.hu_last_error.restype = C.c_char_p
    return _LIB


def _chk(rc: int):
    if rc != 0:
        raise EngineError("hmmufotu_amd error %d: %s" % (rc, load_library().hu_last_error().decode()))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def anneal_max_mismatch(max_dist: float, length: int) -> int:
    """the hit threshold of hu_anneal_batch: the largest d with d / length <= max_dist in double precision, -1 if none"""
    lib = load_library()
    lib.hu_anneal_max_mismatch.restype = C.c_int64
    return int(lib.hu_anneal_max_mismatch(C.c_double(max_dist), C.c_int32(length)))


def anneal_match_table() -> np.ndarray:
    """[256] uint8: the node codes each alignment byte matches (bit 0..3 = A C G T, bit 4 = gap -2, bit 5 = invalid -1)"""
    t = np.zeros(256, np.uint8)
    _chk(load_library().hu_anneal_match_table(_p(t, C.c_uint8)))
    return t


_COMPL = str.maketrans("ACGTUYRKMBVDHacgtuyrkmbvdh", "TGCAARYMKVBHDtgcaarymkvbhd")


def revcom_as_read(s: str) -> str:
    """PrimarySeq::revcom (src/PrimarySeq.h:229-231): IUPACNucl complements, a lower-case letter complemented in lower case
    (src/IUPACNucl.h:73-75), every other character kept"""
    return s[::-1].translate(_COMPL)


def device_count() -> int:
    return int(load_library().hu_device_count())


def default_opts(**kw) -> Opts:
    o = Opts()
    load_library().hu_default_opts(C.byref(o))
    for k, v in kw.items():
        if k == "align_mode" and isinstance(v, str):
            v = MODE[v]
        setattr(o, k, v)
    return o


def model_desc(type_id: int, pi, par, dg_rates=None) -> ModelDesc:
    m = ModelDesc()
    m.type = int(type_id)
    for i in range(4):
        m.pi[i] = float(pi[i])
    par = np.asarray(par, np.float64).ravel()
    for i in range(min(16, len(par))):
        m.par[i] = float(par[i])
    dg = np.asarray(dg_rates if dg_rates is not None else [], np.float64)
    m.dg_k = len(dg)
    for i in range(len(dg)):
        m.dg_rate[i] = float(dg[i])
    return m


def model_spectral(md: ModelDesc):
    """Host-only: (U, lam, U1) with P(t) = U diag(exp(lam t)) U1 as the kernels use it."""
    U = np.zeros(16); lam = np.zeros(4); U1 = np.zeros(16)
    _chk(load_library().hu_model_spectral(C.byref(md), _p(U, C.c_double), _p(lam, C.c_double), _p(U1, C.c_double)))
    return U.reshape(4, 4), lam, U1.reshape(4, 4)


def parse_files(hmm_path=None, ptu_path=None):
    """Host-only parse of the reference's .hmm / .ptu formats (no device needed)."""
    L_ = load_library()
    K = C.c_int32(0); L = C.c_int32(0); n = C.c_int32(0); root = C.c_int32(0); md = ModelDesc()
    hp = hmm_path.encode() if hmm_path else None
    pp = ptu_path.encode() if ptu_path else None
    _chk(L_.hu_files_parse(hp, pp, C.byref(K), C.byref(L), C.byref(n), C.byref(root), *([None] * 12), C.byref(md), 0))
    out = dict(K=K.value, L=L.value, n_nodes=n.value, root=root.value, model=md)
    args = [None] * 12
    if hmm_path:
        out.update(EM=np.zeros((K.value + 1, 4)), EI=np.zeros((K.value + 1, 4)), T=np.zeros((K.value + 1, 7)),
                   p2cs=np.zeros(K.value + 1, np.int32), entry_cost=np.zeros(K.value + 1), exit_cost=np.zeros(K.value + 1))
        args[0:6] = [_p(out["EM"], C.c_double), _p(out["EI"], C.c_double), _p(out["T"], C.c_double), _p(out["p2cs"], C.c_int32),
                     _p(out["entry_cost"], C.c_double), _p(out["exit_cost"], C.c_double)]
    if ptu_path:
        nn, ll = n.value, L.value
        out.update(parent=np.zeros(nn, np.int32), blen=np.zeros(nn), seq=np.zeros((nn, ll), np.int8), height=np.zeros(nn),
                   up=np.zeros((nn, ll, 4)), down=np.zeros((nn, ll, 4)))
        args[6:12] = [_p(out["parent"], C.c_int32), _p(out["blen"], C.c_double), _p(out["seq"], C.c_int8), _p(out["height"], C.c_double),
                      _p(out["up"], C.c_double), _p(out["down"], C.c_double)]
    _chk(L_.hu_files_parse(hp, pp, C.byref(K), C.byref(L), C.byref(n), C.byref(root), *args, C.byref(md), 1))
    return out


def tree_evaluate(parent, blen, seq, model: ModelDesc, up_ptr: int, down_ptr: int, win_start=0, win_len=0, device=0):
    """hu_tree_evaluate: fills the DEVICE buffers at up_ptr/down_ptr ([n][win_len][4] float64, log space),
    returns (seq with inferred inner rows, heights)."""
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64)
    seq = np.ascontiguousarray(seq, np.int8).copy()
    n, L = seq.shape
    h = np.zeros(n)
    _chk(load_library().hu_tree_evaluate(C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                         C.byref(model), C.c_int(device), C.c_int64(win_start), C.c_int64(win_len),
                                         C.c_void_p(int(up_ptr)), C.c_void_p(int(down_ptr)), _p(h, C.c_double)))
    return seq, h


def msa_encode_table() -> np.ndarray:
    """hu_msa_encode_table: encode(toupper(c)) of the MSA's IUPACNucl alphabet for every byte (0..3 residue, a degenerate letter as
    the first base of its expansion, -2 gap, -1 other)"""
    t = np.zeros(256, np.int8)
    _chk(load_library().hu_msa_encode_table(_p(t, C.c_int8)))
    return t


def msa_stats(rows, device=0) -> dict:
    """hu_msa_stats on an alignment (list of equal-length str/bytes rows, or a uint8 [n][L] array): the raw and weighted column
    counts, the per-sequence start / end / length and the normalised sequence weights of the reference's MSA.
    keep marks the columns MSA::prune keeps (at least one residue)."""
    if isinstance(rows, np.ndarray):
        a = np.ascontiguousarray(rows, np.uint8)
    else:
        b = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
        if not b or any(len(r) != len(b[0]) for r in b):
            raise EngineError("msa_stats: rows must be non-empty and of equal length")
        a = np.frombuffer(b"".join(b), np.uint8).reshape(len(b), len(b[0]))
    n, L = a.shape
    out = dict(res_count=np.zeros((4, L), np.int32), gap_count=np.zeros(L, np.int32), start=np.zeros(n, np.int32), end=np.zeros(n, np.int32),
               len=np.zeros(n, np.int32), seq_weight=np.zeros(n), res_wcount=np.zeros((4, L)), gap_wcount=np.zeros(L))
    _chk(load_library().hu_msa_stats(C.c_int(device), C.c_int64(n), C.c_int64(L), a.ctypes.data_as(C.c_char_p),
                                     _p(out["res_count"], C.c_int32), _p(out["gap_count"], C.c_int32), _p(out["start"], C.c_int32),
                                     _p(out["end"], C.c_int32), _p(out["len"], C.c_int32), _p(out["seq_weight"], C.c_double),
                                     _p(out["res_wcount"], C.c_double), _p(out["gap_wcount"], C.c_double)))
    out["keep"] = out["res_count"].sum(axis=0) > 0
    return out


def _msa_rows(rows, what) -> np.ndarray:
    """an alignment (list of equal-length str/bytes rows, or a uint8 [n][L] array) as a contiguous uint8 [n][L] array"""
    if isinstance(rows, np.ndarray):
        a = np.ascontiguousarray(rows, np.uint8)
        if a.ndim != 2 or a.size == 0:
            raise EngineError("%s: rows must be a non-empty [n][L] array" % what)
        return a
    b = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
    if not b or any(len(r) != len(b[0]) for r in b):
        raise EngineError("%s: rows must be non-empty and of equal length" % what)
    return np.frombuffer(b"".join(b), np.uint8).reshape(len(b), len(b[0]))


def suffix_array_tile() -> int:
    """hu_suffix_array_tile: the pairs one wave sorts per radix pass"""
    return int(load_library().hu_suffix_array_tile())


def suffix_array(text, device=0, info=False):
    """hu_suffix_array: the suffix array (int32 [n]) of a text of symbols 0..4 (bytes or a uint8 array), built on the device;
    info=True: (sa, doubling rounds, device seconds)"""
    t = np.ascontiguousarray(np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text, np.uint8).ravel()
    sa = np.zeros(len(t), np.int32)
    rounds = C.c_int32(0); sec = C.c_double(0)
    _chk(load_library().hu_suffix_array(C.c_int(device), _p(t, C.c_uint8), C.c_int64(len(t)), _p(sa, C.c_int32), C.byref(rounds), C.byref(sec)))
    return (sa, int(rounds.value), float(sec.value)) if info else sa


def _csfm_args(what, rows, cs_seq, cs_identity):
    a = _msa_rows(rows, what)
    n, L = a.shape
    cs = cs_seq.encode() if isinstance(cs_seq, str) else bytes(cs_seq)
    ident = np.ascontiguousarray(cs_identity, np.float64).ravel()
    if len(cs) != L or len(ident) != L or b"\0" in cs:
        raise EngineError("%s: cs_seq has %d characters and cs_identity %d values, the rows %d columns" % (what, len(cs), len(ident), L))
    return a, n, L, cs, ident


def csfm_encode(path, rows, cs_seq, cs_identity, sa):
    """hu_csfm_encode (host only): the reference's <DB>.csfm of an alignment from a GIVEN suffix array of its concatenated text.
    rows as msa_stats takes them; cs_seq [L] characters; cs_identity [L]"""
    a, n, L, cs, ident = _csfm_args("csfm_encode", rows, cs_seq, cs_identity)
    sa = np.ascontiguousarray(sa, np.int32).ravel()
    need = int((msa_encode_table()[a] >= 0).sum()) + n + 1
    if len(sa) != need:
        raise EngineError("csfm_encode: the suffix array has %d entries, the concatenated text %d symbols" % (len(sa), need))
    _chk(load_library().hu_csfm_encode(str(path).encode(), C.c_int64(n), C.c_int64(L), a.ctypes.data_as(C.c_char_p), cs, _p(ident, C.c_double), _p(sa, C.c_int32)))


def csfm_write(path, rows, cs_seq, cs_identity, device=0):
    """hu_csfm_write: the same file, the suffix array, the BWT and the samples built on the device"""
    a, n, L, cs, ident = _csfm_args("csfm_write", rows, cs_seq, cs_identity)
    _chk(load_library().hu_csfm_write(str(path).encode(), C.c_int64(n), C.c_int64(L), a.ctypes.data_as(C.c_char_p), cs, _p(ident, C.c_double), C.c_int(device)))


def csfm_write_timing() -> dict:
    """hu_csfm_write_timing: the phases of this thread's last csfm_write, in seconds, and its doubling rounds"""
    s = np.zeros(4); r = C.c_int32(0)
    _chk(load_library().hu_csfm_write_timing(_p(s, C.c_double), C.byref(r)))
    return dict(text=s[0], device=s[1], encode_write=s[2], suffix_array=s[3], rounds=int(r.value))


SM_TYPES = ["GTR", "TN93", "HKY85", "F81", "K80", "JC69"]
SM_METHODS = {"gojobori": 0, "goldman": 1}


def sm_training_set(parent, child_off, child_idx, row_of, method="Gojobori") -> np.ndarray:
    """hu_sm_training_set (host only): the items [k][3] = (row0, row1, row2) of the reference's Gojobori (triples) or Goldman (pairs,
    row0 = -1) training set, on the arrays of newick_parse and row_of [n] (the MSA row of every leaf, -1 elsewhere).  Gojobori draws
    from the C library's rand() as the reference does; this call never seeds it."""
    parent = np.ascontiguousarray(parent, np.int32); co = np.ascontiguousarray(child_off, np.int32)
    ci = np.ascontiguousarray(child_idx, np.int32); ro = np.ascontiguousarray(row_of, np.int32)
    n = len(parent)
    if str(method).lower() not in SM_METHODS:
        raise EngineError("sm_training_set: unknown training method '%s'" % method)
    if len(co) != n + 1 or len(ci) < n - 1 or len(ro) != n:
        raise EngineError("sm_training_set: the arrays do not describe one tree of %d nodes" % n)
    if len(ci) == 0:
        ci = np.zeros(1, np.int32)
    items = np.zeros((n, 3), np.int32); k = C.c_int64(0)
    _chk(load_library().hu_sm_training_set(C.c_int32(n), _p(parent, C.c_int32), _p(co, C.c_int32), _p(ci, C.c_int32), _p(ro, C.c_int32),
                                           C.c_int(SM_METHODS[str(method).lower()]), _p(items, C.c_int32), C.byref(k)))
    return items[:k.value].copy()


def sm_counts(rows, items, device=0) -> dict:
    """hu_sm_counts: for int8 rows [n_rows][cs_len] (codes of msa_encode_table) and items [k][3], on the device: counts [k][4][4]
    (from, to), dn [k][4] = d, N of (row0, row1) and of (row0, row2) — for a pair (row0 = -1) of (row1, row1) and (row1, row2) —,
    base [n_rows][4]; pass [k]: the reference's distance test on dn (hu_sm_item_pass)."""
    rows = np.ascontiguousarray(rows, np.int8)
    items = np.ascontiguousarray(items, np.int32).reshape(-1, 3)
    if rows.ndim != 2 or rows.size == 0:
        raise EngineError("sm_counts: rows must be a non-empty [n_rows][cs_len] array")
    n, L = rows.shape; k = len(items)
    out = dict(counts=np.zeros((k, 4, 4), np.int32), dn=np.zeros((k, 4), np.int32), base=np.zeros((n, 4), np.int32))
    lib = load_library()
    _chk(lib.hu_sm_counts(C.c_int(device), C.c_int64(n), C.c_int64(L), _p(rows, C.c_int8), C.c_int64(k), _p(items, C.c_int32),
                          _p(out["counts"], C.c_int32), _p(out["dn"], C.c_int32), _p(out["base"], C.c_int32)))
    out["pass"] = sm_item_pass(items, out["dn"])
    return out


def sm_counts_timing() -> dict:
    """hu_sm_counts_timing: the phases of this thread's last sm_counts, in seconds"""
    s = np.zeros(3)
    _chk(load_library().hu_sm_counts_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], kernel=s[1], to_host=s[2])


def sm_item_pass(items, dn) -> np.ndarray:
    """hu_sm_item_pass: per item whether its p-distances are within DNASubModel::MAX_PDIST (NaN fails)"""
    items = np.ascontiguousarray(items, np.int32).reshape(-1, 3); dn = np.ascontiguousarray(dn, np.int32).reshape(-1, 4)
    if len(items) != len(dn):
        raise EngineError("sm_item_pass: %d items, %d distance rows" % (len(items), len(dn)))
    ok = np.zeros(len(items), np.int32)
    _chk(load_library().hu_sm_item_pass(C.c_int64(len(items)), _p(items, C.c_int32), _p(dn, C.c_int32), _p(ok, C.c_int32)))
    return ok.astype(bool)


def sm_train(model_type, mats, passed, base, info=False):
    """hu_sm_train (host only): the ModelDesc of type model_type ("GTR" .. "JC69" or its index) trained on mats [k][4][4] in item order,
    of which passed [k] marks the ones the reference's vector holds, and the four base counts.  info=True: (model, matrices used)"""
    t = SM_TYPES.index(model_type) if isinstance(model_type, str) else int(model_type)
    mats = np.ascontiguousarray(mats, np.float64).reshape(-1, 16)
    ok = np.ascontiguousarray(np.asarray(passed).astype(bool), np.int32).ravel()
    f = np.ascontiguousarray(base, np.int64).ravel()
    if len(ok) != len(mats) or len(f) != 4:
        raise EngineError("sm_train: %d matrices, %d decisions, %d base counts" % (len(mats), len(ok), len(f)))
    md = ModelDesc(); used = C.c_int64(0)
    _chk(load_library().hu_sm_train(C.c_int(t), C.c_int64(len(mats)), _p(mats, C.c_double), _p(ok, C.c_int32), _p(f, C.c_int64), C.byref(md), C.byref(used)))
    return (md, int(used.value)) if info else md


def sm_write_text(model: ModelDesc) -> str:
    """hu_sm_write_text: the model file of a ModelDesc as DNASubModel::write lays it out, every number as %.17g"""
    lib = load_library()
    lib.hu_sm_write_text.restype = C.c_int64
    n = int(lib.hu_sm_write_text(C.byref(model), None, C.c_int64(0)))
    if n < 0:
        _chk(n)
    buf = C.create_string_buffer(n + 1)
    lib.hu_sm_write_text(C.byref(model), buf, C.c_int64(n + 1))
    return buf.value.decode()


HMM_MAX_MIX = 32


class HmmPrior(C.Structure):
    """hu_hmm_prior: the five Dirichlet models of a .dm file"""
    _fields_ = [("me_L", C.c_int32), ("pad0", C.c_int32), ("me_q", C.c_double * HMM_MAX_MIX), ("me_alpha", (C.c_double * HMM_MAX_MIX) * 4),
                ("ie_alpha", C.c_double * 4), ("mt_alpha", C.c_double * 3), ("it_alpha", C.c_double * 2), ("dt_alpha", C.c_double * 2)]

    def as_dict(self) -> dict:
        L = int(self.me_L)
        return dict(me_q=np.array(self.me_q[:L]), me_alpha=np.array([list(r[:L]) for r in self.me_alpha]), ie_alpha=np.array(self.ie_alpha[:]),
                    mt_alpha=np.array(self.mt_alpha[:]), it_alpha=np.array(self.it_alpha[:]), dt_alpha=np.array(self.dt_alpha[:]))


def hmm_prior_read(path: str) -> HmmPrior:
    """hu_hmm_prior_read (host only): the prior file (.dm) of hmmufotu-train-hmm — a Dirichlet mixture for the match emissions and four
    Dirichlet densities for the insert emissions and the M, I and D transitions.  A damaged file raises EngineError."""
    p = HmmPrior()
    _chk(load_library().hu_hmm_prior_read(os.fsencode(str(path)), C.byref(p)))
    return p


def hmm_match_columns(res_wcount, gap_wcount, n_seq: int, symfrac=0.5) -> dict:
    """hu_hmm_match_columns (host only): from the weighted counts of msa_stats over the pruned columns (res_wcount [4][L], gap_wcount [L])
    the match columns of a profile: mask [L], K, and per profile position map (1-based column), cons (str) and identity"""
    rw = np.ascontiguousarray(res_wcount, np.float64); gw = np.ascontiguousarray(gap_wcount, np.float64).ravel()
    if rw.ndim != 2 or rw.shape[0] != 4 or rw.shape[1] != len(gw) or len(gw) == 0:
        raise EngineError("hmm_match_columns: res_wcount must be [4][L] and gap_wcount [L]")
    L = len(gw)
    mask = np.zeros(L, np.uint8); mp = np.zeros(L, np.int32); cons = C.create_string_buffer(L); ident = np.zeros(L); K = C.c_int32(0)
    _chk(load_library().hu_hmm_match_columns(C.c_int64(L), C.c_int64(int(n_seq)), _p(rw, C.c_double), _p(gw, C.c_double), C.c_double(symfrac),
                                             _p(mask, C.c_uint8), C.byref(K), _p(mp, C.c_int32), cons, _p(ident, C.c_double)))
    k = int(K.value)
    return dict(mask=mask.astype(bool), K=k, map=mp[:k].copy(), cons=cons.raw[:k].decode(), identity=ident[:k].copy())


def hmm_counts(rows, weight, start, end, mask, device=0) -> dict:
    """hu_hmm_counts, on the device: the raw weighted counts of BandedHMMP7::build over the pruned alignment rows (list of equal-length
    str/bytes, or a uint8 [n][L] array) with the weights, starts and ends of msa_stats and the mask of hmm_match_columns:
    e_m [K+1][4] (row 0: COMPO), e_i [K+1][4], t [K+1][3][3] indexed (from, to) with M, I, D = 0, 1, 2"""
    a = _msa_rows(rows, "hmm_counts")
    n, L = a.shape
    w = np.ascontiguousarray(weight, np.float64).ravel(); st = np.ascontiguousarray(start, np.int32).ravel(); en = np.ascontiguousarray(end, np.int32).ravel()
    m = np.ascontiguousarray(np.asarray(mask).astype(bool), np.uint8).ravel()
    if len(w) != n or len(st) != n or len(en) != n or len(m) != L:
        raise EngineError("hmm_counts: %d rows x %d columns, %d weights, %d starts, %d ends, a mask of %d" % (n, L, len(w), len(st), len(en), len(m)))
    K = int(m.sum())
    out = dict(e_m=np.zeros((K + 1, 4)), e_i=np.zeros((K + 1, 4)), t=np.zeros((K + 1, 3, 3)))
    _chk(load_library().hu_hmm_counts(C.c_int(device), C.c_int64(n), C.c_int64(L), a.ctypes.data_as(C.c_char_p), _p(w, C.c_double), _p(st, C.c_int32),
                                      _p(en, C.c_int32), _p(m, C.c_uint8), C.c_int32(K), _p(out["e_m"], C.c_double), _p(out["e_i"], C.c_double),
                                      _p(out["t"], C.c_double)))
    return out


def hmm_counts_timing() -> dict:
    """hu_hmm_counts_timing: the phases of this thread's last hmm_counts, in seconds, and the device memory it held"""
    s = np.zeros(4); peak = C.c_int64(0)
    _chk(load_library().hu_hmm_counts_timing(_p(s, C.c_double), C.byref(peak)))
    return dict(to_device=s[0], states_kernel=s[1], counts_kernel=s[2], to_host=s[3], peak_bytes=int(peak.value))


def hmm_estimate(e_m, e_i, t, n_seq: int, prior: HmmPrior) -> dict:
    """hu_hmm_estimate (host only): the effective sequence number by bisection on the mean relative entropy and the probabilities of the
    profile, priors applied: p_m, p_i [K+1][4], p_t [K+1][3][3], eff_n, passes"""
    em = np.ascontiguousarray(e_m, np.float64); ei = np.ascontiguousarray(e_i, np.float64); tt = np.ascontiguousarray(t, np.float64)
    if em.ndim != 2 or em.shape[1] != 4 or em.shape[0] < 2 or ei.shape != em.shape or tt.shape != (em.shape[0], 3, 3):
        raise EngineError("hmm_estimate: counts must be e_m [K+1][4], e_i [K+1][4], t [K+1][3][3] with K >= 1")
    K = em.shape[0] - 1
    out = dict(p_m=np.zeros_like(em), p_i=np.zeros_like(ei), p_t=np.zeros_like(tt))
    eff = C.c_double(0); passes = C.c_int32(0)
    _chk(load_library().hu_hmm_estimate(C.c_int32(K), _p(em, C.c_double), _p(ei, C.c_double), _p(tt, C.c_double), C.c_int64(int(n_seq)), C.byref(prior),
                                        _p(out["p_m"], C.c_double), _p(out["p_i"], C.c_double), _p(out["p_t"], C.c_double), C.byref(eff), C.byref(passes)))
    out["eff_n"] = float(eff.value); out["passes"] = int(passes.value)
    return out


def hmm_write(path, p_m, p_i, p_t, map, cons, cs_len: int, n_seq: int, eff_n: float, name="unnamed", version="hmmufotu_amd", date=""):
    """hu_hmm_write (host only): the profile as the text of the reference's operator<<, costs at 6 significant digits"""
    pm = np.ascontiguousarray(p_m, np.float64); pi = np.ascontiguousarray(p_i, np.float64); pt = np.ascontiguousarray(p_t, np.float64)
    mp = np.ascontiguousarray(map, np.int32).ravel(); cs = cons.encode() if isinstance(cons, str) else bytes(cons)
    K = pm.shape[0] - 1
    if pm.ndim != 2 or pm.shape[1] != 4 or pi.shape != pm.shape or pt.shape != (K + 1, 3, 3) or len(mp) != K or len(cs) != K:
        raise EngineError("hmm_write: p_m, p_i [K+1][4], p_t [K+1][3][3], map and cons of K entries")
    _chk(load_library().hu_hmm_write(os.fsencode(str(path)), str(version).encode(), str(name).encode(), C.c_int32(K), C.c_int32(int(cs_len)),
                                     _p(pm, C.c_double), _p(pi, C.c_double), _p(pt, C.c_double), _p(mp, C.c_int32), cs, C.c_int64(int(n_seq)),
                                     C.c_double(eff_n), str(date).encode()))


DM_STATUS = {1: "converged", 2: "max-it", 3: "nan-overfit", 4: "nan-unused", 5: "not-finite"}


class DmProblem(C.Structure):
    _fields_ = [("K", C.c_int32), ("L", C.c_int32), ("M", C.c_int64), ("data", C.POINTER(C.c_double)), ("alpha0", C.POINTER(C.c_double)),
                ("q0", C.POINTER(C.c_double))]


class DmOpts(C.Structure):
    _fields_ = [("eta", C.c_double), ("abs_eps_cost", C.c_double), ("rel_eps_cost", C.c_double), ("abs_eps_params", C.c_double),
                ("rel_eps_params", C.c_double), ("max_iter", C.c_int64), ("chunk", C.c_int32), ("pad0", C.c_int32)]


class DmResult(C.Structure):
    _fields_ = [("alpha", (C.c_double * 10) * 4), ("q", C.c_double * 10), ("cost", C.c_double), ("iterations", C.c_int64), ("status", C.c_int32),
                ("pad0", C.c_int32)]


def dm_training_data(rows, weight, pri_rate=0.05, symfrac=0.5, device=0) -> dict:
    """hu_dm_training_data, on the device: the five training sets of hmmufotu-train-dm from the pruned alignment rows and the sequence
    weights of msa_stats, scaled by (1 / pri_rate) / n here: mask [L], and me, ie [4][.], mt [3][.], it, dt [2][.] as the reference's
    matrices, one data column per column of the array"""
    a = _msa_rows(rows, "dm_training_data")
    n, L = a.shape
    w = np.ascontiguousarray(weight, np.float64).ravel()
    if len(w) != n:
        raise EngineError("dm_training_data: %d rows, %d weights" % (n, len(w)))
    mask = np.zeros(L, np.uint8); cnt = np.zeros(5, np.int64)
    sets = [np.zeros((L, k)) for k in (4, 4, 3, 2, 2)]
    _chk(load_library().hu_dm_training_data(C.c_int(device), C.c_int64(n), C.c_int64(L), a.ctypes.data_as(C.c_char_p), _p(w, C.c_double), C.c_double(pri_rate),
                                            C.c_double(symfrac), _p(mask, C.c_uint8), *[_p(s, C.c_double) for s in sets], _p(cnt, C.c_int64)))
    out = {k: np.ascontiguousarray(s[:int(c)].T) for k, s, c in zip(("me", "ie", "mt", "it", "dt"), sets, cnt)}
    out["mask"] = mask.astype(bool)
    return out


def dm_training_data_timing() -> dict:
    """hu_dm_training_data_timing: the phases of this thread's last dm_training_data, in seconds, and the device memory it held"""
    s = np.zeros(4); peak = C.c_int64(0)
    _chk(load_library().hu_dm_training_data_timing(_p(s, C.c_double), C.byref(peak)))
    return dict(to_device=s[0], wcounts_and_mask=s[1], states_kernels=s[2], counts_kernel=s[3], peak_bytes=int(peak.value))


def dm_shuffle(M: int, seed=None) -> np.ndarray:
    """hu_dm_shuffle (host only): std::random_shuffle of 0 .. M - 1 on the C library's rand(); seed given: srand(seed) first, else the
    stream goes on"""
    idx = np.zeros(max(int(M), 1), np.int32)
    sd = C.c_uint32(int(seed) & 0xFFFFFFFF) if seed is not None else None
    _chk(load_library().hu_dm_shuffle(C.c_int64(int(M)), C.byref(sd) if sd is not None else None, _p(idx, C.c_int32)))
    return idx[:int(M)].copy()


def _dm_data(data, what):
    d = np.asarray(data, np.float64)
    if d.ndim != 2 or not 2 <= d.shape[0] <= 4:
        raise EngineError("%s: data must be [K][M] with K 2 .. 4" % what)
    return np.ascontiguousarray(d.T)                                                    # [M][K]: a data column's values together


def dm_moment_init(data, L=1, idx=None) -> np.ndarray:
    """hu_dm_moment_init (host only): where the training of a density (L = 1) or of a mixture of L components (idx: the order of
    dm_shuffle) starts, alpha [K][L]; 1 where the reference leaves the model as it is"""
    d = _dm_data(data, "dm_moment_init")
    M, K = d.shape
    ix = np.ascontiguousarray(idx, np.int32).ravel() if idx is not None else None
    if L > 1 and M > 0 and (ix is None or len(ix) != M):
        raise EngineError("dm_moment_init: a mixture needs idx [M]")
    alpha = np.zeros((K, int(L)))
    _chk(load_library().hu_dm_moment_init(C.c_int32(K), C.c_int32(int(L)), C.c_int64(M), _p(d, C.c_double), _p(ix, C.c_int32) if ix is not None else None,
                                          _p(alpha, C.c_double)))
    return alpha


def dm_train(problems, eta=0.001, abs_eps_cost=0.0, rel_eps_cost=1e-6, abs_eps_params=0.0, rel_eps_params=1e-4, max_iter=0, chunk=None, device=0,
             progress=None) -> list:
    """hu_dm_train, on the device: gradient ascent of a batch of independent problems, one workgroup each.  problems: dicts with data
    [K][M], alpha0 [K][L] (a density: [K] or [K][1]) and optionally q0 [L].  Per problem a dict of alpha [K][L], q [L], cost, iterations
    and status (a name of DM_STATUS).  progress(iterations, running) is called after every launch of `chunk` iterations."""
    lib = load_library()
    o = DmOpts()
    lib.hu_dm_default_opts(C.byref(o))
    o.eta, o.abs_eps_cost, o.rel_eps_cost, o.abs_eps_params, o.rel_eps_params, o.max_iter = eta, abs_eps_cost, rel_eps_cost, abs_eps_params, rel_eps_params, int(max_iter)
    if chunk is not None:
        o.chunk = int(chunk)
    n = len(problems)
    P = (DmProblem * max(n, 1))(); R = (DmResult * max(n, 1))()
    keep = []
    for i, pr in enumerate(problems):
        d = _dm_data(pr["data"], "dm_train")
        a0 = np.ascontiguousarray(np.asarray(pr["alpha0"], np.float64).reshape(d.shape[1], -1))
        q0 = np.ascontiguousarray(pr["q0"], np.float64).ravel() if pr.get("q0") is not None else None
        if q0 is not None and len(q0) != a0.shape[1]:
            raise EngineError("dm_train: problem %d: q0 of %d entries, alpha0 of %d components" % (i, len(q0), a0.shape[1]))
        keep.append((d, a0, q0))
        P[i] = DmProblem(d.shape[1], a0.shape[1], d.shape[0], _p(d, C.c_double), _p(a0, C.c_double), _p(q0, C.c_double) if q0 is not None else None)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int32)
    cb = CB((lambda user, it, running: progress(int(it), int(running))) if progress else 0)
    _chk(lib.hu_dm_train(C.c_int(device), C.c_int32(n), P, C.byref(o), R, cb, None))
    out = []
    for i, (d, a0, q0) in enumerate(keep):
        K, L = a0.shape
        out.append(dict(alpha=np.array([list(R[i].alpha[r][:L]) for r in range(K)]), q=np.array(R[i].q[:L]), cost=float(R[i].cost),
                        iterations=int(R[i].iterations), status=DM_STATUS.get(int(R[i].status), str(int(R[i].status)))))
    return out


def dm_special(x, device=0):
    """hu_dm_special (test probe): the training kernel's lgamma and digamma at the points x > 0"""
    xs = np.ascontiguousarray(x, np.float64).ravel()
    lg = np.zeros_like(xs); dg = np.zeros_like(xs)
    _chk(load_library().hu_dm_special(C.c_int(device), C.c_int64(len(xs)), _p(xs, C.c_double), _p(lg, C.c_double), _p(dg, C.c_double)))
    return lg, dg


def dm_write(path, me_q, me_alpha, ie_alpha, mt_alpha, it_alpha, dt_alpha, cost):
    """hu_dm_write (host only): a prior file (.dm) as the reference's operator<< writes it; cost: the five training costs ME IE MT IT DT"""
    p = HmmPrior()
    q = np.asarray(me_q, np.float64).ravel(); a = np.asarray(me_alpha, np.float64)
    L = len(q)
    if a.shape != (4, L) or not 1 <= L <= HMM_MAX_MIX:
        raise EngineError("dm_write: me_q [L] and me_alpha [4][L]")
    p.me_L = L
    for j in range(L):
        p.me_q[j] = q[j]
        for i in range(4):
            p.me_alpha[i][j] = a[i, j]
    for name, v, k in (("ie_alpha", ie_alpha, 4), ("mt_alpha", mt_alpha, 3), ("it_alpha", it_alpha, 2), ("dt_alpha", dt_alpha, 2)):
        v = np.asarray(v, np.float64).ravel()
        if len(v) != k:
            raise EngineError("dm_write: %s of %d entries" % (name, k))
        for i in range(k):
            getattr(p, name)[i] = v[i]
    c = np.ascontiguousarray(cost, np.float64).ravel()
    if len(c) != 5:
        raise EngineError("dm_write: five costs")
    _chk(load_library().hu_dm_write(os.fsencode(str(path)), C.byref(p), _p(c, C.c_double)))


class SimOpts(C.Structure):
    _fields_ = [("max_dist", C.c_double), ("mean_size", C.c_double), ("sd_size", C.c_double), ("min_size", C.c_double), ("max_size", C.c_double),
                ("n_regions", C.c_int64), ("regions", C.POINTER(C.c_int32))]


def sim_philox(counter, key) -> np.ndarray:
    """hu_sim_philox (host only): the four words of Philox4x32-10 for a counter [4] and a key [2], the generator of the simulated reads"""
    c = np.ascontiguousarray(counter, np.uint32).ravel(); k = np.ascontiguousarray(key, np.uint32).ravel()
    if len(c) != 4 or len(k) != 2:
        raise EngineError("sim_philox: a counter of 4 words and a key of 2")
    out = np.zeros(4, np.uint32)
    _chk(load_library().hu_sim_philox(_p(c, C.c_uint32), _p(k, C.c_uint32), _p(out, C.c_uint32)))
    return out


def sim_plan(parent, blen, height, cs_len: int, n: int, seed: int, max_dist=np.inf, mean_size=500.0, sd_size=30.0, min_size=0.0, max_size=0.0,
             regions=None, attempt=0, info=False) -> dict:
    """hu_sim_plan (host only): node, rc, start, end of n reads by the rejection loop of hmmufotu-sim on a tree's arrays.  regions: the
    (start, end) pairs of a BED file; those outside the consensus are dropped.  attempt: the first attempt number, for a plan made in
    pieces; info=True adds the next one as "attempt"."""
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64); height = np.ascontiguousarray(height, np.float64)
    nn = len(parent)
    if len(blen) != nn or len(height) != nn:
        raise EngineError("sim_plan: parent, blen and height must have one entry per node")
    o = SimOpts(float(max_dist), float(mean_size), float(sd_size), float(min_size), float(max_size), 0, None)
    reg = np.ascontiguousarray(regions if regions is not None else [], np.int32).reshape(-1, 2)
    if len(reg):
        o.n_regions = len(reg); o.regions = _p(reg, C.c_int32)
    out = dict(node=np.zeros(n, np.int32), rc=np.zeros(n), start=np.zeros(n, np.int32), end=np.zeros(n, np.int32))
    att = C.c_int64(int(attempt))
    _chk(load_library().hu_sim_plan(C.c_int32(nn), C.c_int32(int(cs_len)), _p(parent, C.c_int32), _p(blen, C.c_double), _p(height, C.c_double), C.byref(o),
                                    C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(att), C.c_int64(n), _p(out["node"], C.c_int32), _p(out["rc"], C.c_double),
                                    _p(out["start"], C.c_int32), _p(out["end"], C.c_int32)))
    if info:
        out["attempt"] = int(att.value)
    return out


def sim_description(c: int, p: int, taxon_c: str, taxon_p: str, rc: float, start: int, end: int, seq_len: int) -> str:
    """hu_sim_description (host only): the description of a simulated read's FASTA record as hmmufotu-sim writes it"""
    lib = load_library()
    lib.hu_sim_description.restype = C.c_int64
    args = (C.c_int32(c), C.c_int32(p), taxon_c.encode(), taxon_p.encode(), C.c_double(rc), C.c_int32(start), C.c_int32(end), C.c_int64(seq_len))
    n = int(lib.hu_sim_description(*args, None, C.c_int64(0)))
    if n < 0:
        _chk(n)
    buf = C.create_string_buffer(n + 1)
    lib.hu_sim_description(*args, buf, C.c_int64(n + 1))
    return buf.value.decode()


def sim_timing() -> dict:
    """hu_sim_timing: the phases of this thread's last Database.sim_reads, in seconds"""
    s = np.zeros(3)
    _chk(load_library().hu_sim_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], kernel=s[1], to_host=s[2])


class OtuOpts(C.Structure):
    _fields_ = [("chunk", C.c_int32), ("key_bits", C.c_int32)]


OTU_METHODS = {"uniform": 0, "multinomial": 1}


def _otu_dict(h) -> dict:
    """the content of a hu_otu_table as Python values"""
    lib = load_library()
    for f in (lib.hu_otu_table_otu, lib.hu_otu_table_taxon, lib.hu_otu_table_sample):
        f.restype = C.c_char_p
    lib.hu_otu_table_counts.restype = C.POINTER(C.c_double)
    m = C.c_int64(); n = C.c_int64()
    _chk(lib.hu_otu_table_dims(h, C.byref(m), C.byref(n)))
    M, S = int(m.value), int(n.value)
    counts = np.ctypeslib.as_array(lib.hu_otu_table_counts(h), shape=(M, S)).copy() if M * S else np.zeros((M, S))
    return dict(otus=[lib.hu_otu_table_otu(h, C.c_int64(i)).decode() for i in range(M)], taxa=[lib.hu_otu_table_taxon(h, C.c_int64(i)).decode() for i in range(M)],
                samples=[lib.hu_otu_table_sample(h, C.c_int64(j)).decode() for j in range(S)], counts=counts)


def _otu_handle(table):
    """a hu_otu_table from dict(otus, taxa, samples, counts [otus][samples]); the caller frees it"""
    otus = [str(x).encode() for x in table["otus"]]; taxa = [str(x).encode() for x in table["taxa"]]; samples = [str(x).encode() for x in table["samples"]]
    M, S = len(otus), len(samples)
    counts = np.ascontiguousarray(table["counts"], np.float64).reshape(M, S) if M * S else np.zeros((M, S))
    if len(taxa) != M:
        raise EngineError("otu table: one taxonomy per OTU")
    h = C.c_void_p()
    _chk(load_library().hu_otu_table_new(C.c_int64(M), C.c_int64(S), (C.c_char_p * max(M, 1))(*otus), (C.c_char_p * max(M, 1))(*taxa), (C.c_char_p * max(S, 1))(*samples),
                                         _p(counts, C.c_double), C.byref(h)))
    return h


def otu_table_read(path) -> dict:
    """hu_otu_table_read (host only): an OTU table in the reference's "table" format as dict(otus, taxa, samples, counts [otus][samples])"""
    lib = load_library()
    h = C.c_void_p()
    _chk(lib.hu_otu_table_read(os.fsencode(str(path)), C.byref(h)))
    try:
        return _otu_dict(h)
    finally:
        lib.hu_otu_table_free(h)


def otu_table_write(path, table, info=""):
    """hu_otu_table_write (host only): "# HmmUFOtu v1.5.1" + info, the header, one row per OTU, numbers as hmmufotu-amd-sum prints them"""
    lib = load_library()
    h = _otu_handle(table)
    try:
        _chk(lib.hu_otu_table_write(h, os.fsencode(str(path)), info.encode()))
    finally:
        lib.hu_otu_table_free(h)


def otu_table_merge(tables) -> dict:
    """hu_otu_table_merge (host only): the tables added up in the order given, as OTUTable::operator+= adds them"""
    lib = load_library()
    acc = _otu_handle(dict(otus=[], taxa=[], samples=[], counts=[]))
    try:
        for t in tables:
            h = _otu_handle(t)
            try:
                _chk(lib.hu_otu_table_merge(acc, h))
            finally:
                lib.hu_otu_table_free(h)
        return _otu_dict(acc)
    finally:
        lib.hu_otu_table_free(acc)


def otu_table_normalize(table, Z=0.0) -> dict:
    """hu_otu_table_normalize (host only): every cell / (column sum / Z), Z 0 = the largest column sum; "zero_columns": the samples without
    reads, which stay 0"""
    lib = load_library()
    h = _otu_handle(table)
    try:
        z = C.c_int64()
        _chk(lib.hu_otu_table_normalize(h, C.c_double(float(Z)), C.byref(z)))
        out = _otu_dict(h)
        out["zero_columns"] = int(z.value)
        return out
    finally:
        lib.hu_otu_table_free(h)


def otu_table_prune(table, min_sample=0, otus=True) -> dict:
    """hu_otu_table_prune_samples, then hu_otu_table_prune_otus (host only): the samples whose total is below min_sample go (0: none), then
    the OTUs without reads"""
    lib = load_library()
    h = _otu_handle(table)
    try:
        _chk(lib.hu_otu_table_prune_samples(h, C.c_uint64(int(min_sample))))
        if otus:
            _chk(lib.hu_otu_table_prune_otus(h))
        return _otu_dict(h)
    finally:
        lib.hu_otu_table_free(h)


def otu_subset(counts, size, method="uniform", seed=0, device=0, chunk=None, key_bits=64) -> np.ndarray:
    """hu_otu_subset: every sample (column) of counts [otus][samples] rarefied to `size` reads, without ("uniform") or with ("multinomial")
    replacement; samples of at most `size` reads come back untouched.  device < 0: the library's host path, which gives the same integers."""
    c = np.ascontiguousarray(counts, np.float64)
    if c.ndim != 2:
        raise EngineError("otu_subset: counts [otus][samples]")
    if method not in OTU_METHODS:
        raise EngineError("otu_subset: method 'uniform' or 'multinomial', not %r" % (method,))
    lib = load_library()
    o = OtuOpts()
    lib.hu_otu_default_opts(C.byref(o))
    if chunk is not None:
        o.chunk = int(chunk)
    o.key_bits = int(key_bits)
    out = np.zeros_like(c)
    _chk(lib.hu_otu_subset(C.c_int(int(device)), C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), _p(c, C.c_double), C.c_uint64(int(size) if int(size) > 0 else 0),
                           C.c_int(OTU_METHODS[method]), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(o), _p(out, C.c_double)))
    return out


def otu_subset_timing() -> dict:
    """hu_otu_subset_timing: the phases of this thread's last otu_subset on a device, in seconds"""
    s = np.zeros(3)
    _chk(load_library().hu_otu_subset_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], kernels=s[1], to_host=s[2])


class UnifracOpts(C.Structure):
    _fields_ = [("method", C.c_int32), ("host", C.c_int32), ("alpha", C.c_double), ("slab", C.c_int64), ("mem_budget", C.c_int64)]


class UnifracTree(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("parent", C.POINTER(C.c_int32)), ("blen", C.POINTER(C.c_double))]


UNIFRAC_METHODS = {"unweighted": 0, "weighted": 1, "weighted-raw": 2, "generalized": 3, "bray-curtis": 4, "jaccard": 5}


def unifrac_default_slab(n_sample: int, n_branch: int) -> int:
    """hu_unifrac_default_slab: the branches per slab that a table of n_sample samples and n_branch kept branches gets"""
    lib = load_library()
    lib.hu_unifrac_default_slab.restype = C.c_int64
    return int(lib.hu_unifrac_default_slab(C.c_int64(int(n_sample)), C.c_int64(int(n_branch))))


def _unifrac_args(what, counts, otu_node, parent, blen, method, alpha, slab, host, mem_budget):
    c = np.ascontiguousarray(counts, np.float64)
    if c.ndim != 2:
        raise EngineError(what + ": counts [otus][samples]")
    if method not in UNIFRAC_METHODS:
        raise EngineError(what + ": method one of %s, not %r" % (", ".join(UNIFRAC_METHODS), method))
    o = UnifracOpts()
    load_library().hu_unifrac_default_opts(C.byref(o))
    o.method = UNIFRAC_METHODS[method]; o.host = 1 if host else 0; o.slab = int(slab or 0); o.mem_budget = int(mem_budget or 0)
    if alpha is not None:
        o.alpha = float(alpha)
    keep = [c]
    tree = None; node = None
    if parent is not None:
        par = np.ascontiguousarray(parent, np.int32); bl = np.ascontiguousarray(blen, np.float64)
        if par.ndim != 1 or bl.shape != par.shape:
            raise EngineError(what + ": parent and blen [nodes]")
        if otu_node is None or len(otu_node) != c.shape[0]:
            raise EngineError(what + ": one node per OTU row")
        nd = np.ascontiguousarray(otu_node, np.int32)
        tree = UnifracTree(len(par), _p(par, C.c_int32), _p(bl, C.c_double)); node = _p(nd, C.c_int32)
        keep += [par, bl, nd]
    return c, o, tree, node, keep


def unifrac(counts, otu_node=None, parent=None, blen=None, method="weighted", alpha=None, slab=0, device=0, host=False, pd=False, mem_budget=0):
    """hu_unifrac: the distances [samples][samples] between the columns of counts [otus][samples] on the tree (parent [nodes] with -1 for
    the root, blen [nodes]); otu_node [otus] is the node of every row.  "bray-curtis" and "jaccard" take no tree.  slab 0: the documented
    function of the table's size.  host: the library's host path, no device needed.  pd: also Faith's PD, returned as (dist, pd)."""
    c, o, tree, node, keep = _unifrac_args("unifrac", counts, otu_node, parent, blen, method, alpha, slab, host, mem_budget)
    S = c.shape[1]
    dist = np.zeros((S, S)); fpd = np.zeros(S)
    _chk(load_library().hu_unifrac(C.c_int(int(device)), C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(S), node, _p(c, C.c_double),
                                   C.byref(o), _p(dist, C.c_double), _p(fpd, C.c_double) if pd else None))
    return (dist, fpd) if pd else dist


def unifrac_embed(counts, otu_node=None, parent=None, blen=None, method="weighted", device=0, host=False, mem_budget=0) -> dict:
    """hu_unifrac_embed: the kept branches (in depth-first order) as dict(node [B], blen [B], P [B][samples]): P[k][j] is the share of
    sample j's reads that lie below branch k"""
    c, o, tree, node, keep = _unifrac_args("unifrac_embed", counts, otu_node, parent, blen, method, None, 0, host, mem_budget)
    lib = load_library()
    nb = C.c_int64(0)
    args = (C.c_int(int(device)), C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), node, _p(c, C.c_double), C.byref(o), C.byref(nb))
    _chk(lib.hu_unifrac_embed(*args, C.c_int64(0), None, None, None))
    B = int(nb.value)
    bn = np.zeros(B, np.int32); bl = np.zeros(B); P = np.zeros((B, c.shape[1]))
    if B:
        _chk(lib.hu_unifrac_embed(*args, C.c_int64(B), _p(bn, C.c_int32), _p(bl, C.c_double), _p(P, C.c_double)))
    return dict(node=bn, blen=bl, P=P)


def unifrac_timing() -> dict:
    """hu_unifrac_timing: the phases of this thread's last unifrac / unifrac_embed on a device, in seconds"""
    s = np.zeros(4)
    _chk(load_library().hu_unifrac_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], embed=s[1], pairs=s[2], to_host=s[3])


class PermanovaOpts(C.Structure):
    _fields_ = [("perms", C.c_int64), ("seed", C.c_uint64), ("host", C.c_int32), ("reserved", C.c_int32), ("chunk", C.c_int64), ("mem_budget", C.c_int64)]


class PermanovaResult(C.Structure):
    _fields_ = [("n", C.c_int64), ("a", C.c_int64), ("perms", C.c_int64), ("ss_total", C.c_double), ("ss_within", C.c_double), ("ss_among", C.c_double),
                ("F", C.c_double), ("R2", C.c_double), ("count_le", C.c_int64), ("p", C.c_double)]


def permanova(dist, group, perms=999, seed=1, chunk=0, device=0, host=False, mem_budget=0) -> dict:
    """hu_permanova: PERMANOVA of the labels group [n] (0 .. a-1) on the distance matrix dist [n][n]: dict(n, a, perms, ss_total, ss_within,
    ss_among, F, R2, count_le, p, ssw_perm [perms]).  chunk 0: as many permutations per launch as the memory holds.  host: the library's
    host path, no device needed; it gives the same bits."""
    d = np.ascontiguousarray(dist, np.float64); g = np.ascontiguousarray(group, np.int32)
    if d.ndim != 2 or d.shape[0] != d.shape[1] or g.shape != (d.shape[0],):
        raise EngineError("permanova: dist [n][n] and group [n]")
    lib = load_library()
    o = PermanovaOpts()
    lib.hu_permanova_default_opts(C.byref(o))
    o.perms = int(perms); o.seed = int(seed) & (2 ** 64 - 1); o.host = 1 if host else 0; o.chunk = int(chunk or 0); o.mem_budget = int(mem_budget or 0)
    r = PermanovaResult()
    ssw = np.zeros(max(int(perms), 0))
    _chk(lib.hu_permanova(C.c_int(int(device)), C.c_int64(d.shape[0]), _p(d, C.c_double), _p(g, C.c_int32), C.byref(o), C.byref(r), _p(ssw, C.c_double) if len(ssw) else None))
    out = {k: getattr(r, k) for k, _ in PermanovaResult._fields_}
    out["ssw_perm"] = ssw
    return out


def permanova_labels(group, seed=1, first=0, count=1) -> np.ndarray:
    """hu_permanova_labels (host only): [count][n], the labellings of permutations first .. first + count - 1 of the labels group [n]"""
    g = np.ascontiguousarray(group, np.int32)
    if g.ndim != 1:
        raise EngineError("permanova_labels: group [n]")
    out = np.zeros((int(count), len(g)), np.int32)
    _chk(load_library().hu_permanova_labels(C.c_int64(len(g)), _p(g, C.c_int32), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int64(int(first)), C.c_int64(int(count)),
                                            _p(out, C.c_int32)))
    return out


def permanova_need(n: int, a: int, chunk: int) -> int:
    """hu_permanova_need: the bytes of device memory that n samples in a groups take with `chunk` permutations per launch"""
    lib = load_library()
    lib.hu_permanova_need.restype = C.c_int64
    return int(lib.hu_permanova_need(C.c_int64(int(n)), C.c_int64(int(a)), C.c_int64(int(chunk))))


def permanova_timing() -> dict:
    """hu_permanova_timing: the phases of this thread's last permanova on a device, in seconds"""
    s = np.zeros(4)
    _chk(load_library().hu_permanova_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], shuffle=s[1], pairs=s[2], finish=s[3])


class DesignVar(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("value", C.POINTER(C.c_double)), ("label", C.POINTER(C.c_int32))]


class DesignTerm(C.Structure):
    _fields_ = [("a", C.c_int32), ("b", C.c_int32)]


class PermanovaDesignOpts(C.Structure):
    _fields_ = [("perms", C.c_int64), ("seed", C.c_uint64), ("host", C.c_int32), ("index32", C.c_int32), ("chunk", C.c_int64), ("mem_budget", C.c_int64)]


class PermanovaDesignTerm(C.Structure):
    _fields_ = [("df", C.c_int64), ("df_res", C.c_int64), ("ss", C.c_double), ("ss_res", C.c_double), ("ss_total", C.c_double), ("R2", C.c_double),
                ("F", C.c_double), ("count_ge", C.c_int64), ("count_nan", C.c_int64), ("p", C.c_double)]


def design_build(variables: dict, terms, factors=()) -> dict:
    """hu_design_build (host only): the orthonormal, centred basis of a design.  variables: name -> values [n]; a variable is numeric when
    its values are numbers and its name is not in `factors`, otherwise categorical, its levels numbered in order of first appearance.
    terms: names, an interaction as 'a:b'.  dict(Q [n][q], q, term_start [T + 1], df [T], dropped [T])."""
    names = list(variables)
    if not names or not terms:
        raise EngineError("design_build: variables and one term at the least")
    keep, cvars = [], (DesignVar * len(names))()
    n = len(variables[names[0]])
    for k, name in enumerate(names):
        vals = list(variables[name])
        if len(vals) != n:
            raise EngineError("design_build: variable '%s' has %d of %d values" % (name, len(vals), n))
        numeric = name not in factors and all(isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool) for x in vals)
        if numeric:
            a = np.ascontiguousarray(vals, np.float64)
            cvars[k].kind = 0; cvars[k].value = _p(a, C.c_double)
        else:
            first = {}
            a = np.ascontiguousarray([first.setdefault(x, len(first)) for x in vals], np.int32)
            cvars[k].kind = 1; cvars[k].label = _p(a, C.c_int32)
        keep.append(a)
    cterms = (DesignTerm * len(terms))()
    for t, term in enumerate(terms):
        parts = str(term).split(":")
        if len(parts) > 2 or any(p not in names for p in parts):
            raise EngineError("design_build: term '%s': one variable, or two joined by ':'" % term)
        cterms[t].a = names.index(parts[0]); cterms[t].b = names.index(parts[1]) if len(parts) == 2 else -1
    lib = load_library()
    lib.hu_design_raw_columns.restype = C.c_int64
    T = len(terms)
    raw = int(lib.hu_design_raw_columns(C.c_int64(n), C.c_int64(len(names)), cvars, C.c_int64(T), cterms))
    if raw < 0:
        _chk(-1)
    Q = np.zeros(max(n * raw, 1)); q = C.c_int64()
    ts = np.zeros(T + 1, np.int64); df = np.zeros(T, np.int64); dropped = np.zeros(T, np.int64)
    tn = (C.c_char_p * T)(*[str(t).encode() for t in terms])
    _chk(lib.hu_design_build(C.c_int64(n), C.c_int64(len(names)), cvars, C.c_int64(T), cterms, tn, _p(Q, C.c_double), C.byref(q), _p(ts, C.c_int64), _p(df, C.c_int64),
                             _p(dropped, C.c_int64)))
    return dict(Q=Q[:n * q.value].reshape(n, q.value).copy(), q=q.value, term_start=ts, df=df, dropped=dropped)


def permanova_perms(n: int, strata=None, seed=1, first=0, count=1) -> np.ndarray:
    """hu_permanova_perms (host only): [count][n], the index arrays of permutations first .. first + count - 1: the design row of sample i
    is row out[p][i] of the basis.  strata [n]: dense labels; a sample moves within its stratum only."""
    s = None if strata is None else np.ascontiguousarray(strata, np.int32)
    if s is not None and s.shape != (int(n),):
        raise EngineError("permanova_perms: strata [n]")
    out = np.zeros((int(count), int(n)), np.int64)
    _chk(load_library().hu_permanova_perms(C.c_int64(int(n)), _p(s, C.c_int32) if s is not None else None, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_int64(int(first)),
                                           C.c_int64(int(count)), _p(out, C.c_int64)))
    return out


def permanova_design(dist, Q, term_start, strata=None, perms=999, seed=1, chunk=0, device=0, host=False, mem_budget=0, index32=False) -> dict:
    """hu_permanova_design: sequential PERMANOVA of the terms of the basis Q [n][q] (design_build) on the distance matrix dist [n][n]:
    dict(terms [T] of dict(df, df_res, ss, ss_res, ss_total, R2, F, count_ge, count_nan, p), ss_total, ss_res, df_res, ss_perm [perms][T]).
    host: the library's host path, no device needed; the two paths agree within the bound of DESIGN.md §33, not in their bits."""
    d = np.ascontiguousarray(dist, np.float64); B = np.ascontiguousarray(Q, np.float64); ts = np.ascontiguousarray(term_start, np.int64)
    s = None if strata is None else np.ascontiguousarray(strata, np.int32)
    if d.ndim != 2 or d.shape[0] != d.shape[1] or B.ndim != 2 or B.shape[0] != d.shape[0] or ts.ndim != 1 or len(ts) < 2 or (s is not None and s.shape != (d.shape[0],)):
        raise EngineError("permanova_design: dist [n][n], Q [n][q], term_start [T + 1] and strata [n]")
    lib = load_library()
    o = PermanovaDesignOpts()
    lib.hu_permanova_design_default_opts(C.byref(o))
    o.perms = int(perms); o.seed = int(seed) & (2 ** 64 - 1); o.host = 1 if host else 0; o.index32 = 1 if index32 else 0; o.chunk = int(chunk or 0)
    o.mem_budget = int(mem_budget or 0)
    T = len(ts) - 1
    res = (PermanovaDesignTerm * T)()
    ss = np.zeros((max(int(perms), 0), T))
    _chk(lib.hu_permanova_design(C.c_int(int(device)), C.c_int64(d.shape[0]), _p(d, C.c_double), _p(B, C.c_double), C.c_int64(B.shape[1]), C.c_int64(T), _p(ts, C.c_int64),
                                 _p(s, C.c_int32) if s is not None else None, C.byref(o), res, _p(ss, C.c_double) if ss.size else None))
    terms = [{k: getattr(r, k) for k, _ in PermanovaDesignTerm._fields_} for r in res]
    return dict(terms=terms, ss_total=terms[0]["ss_total"], ss_res=terms[0]["ss_res"], df_res=terms[0]["df_res"], ss_perm=ss)


def permanova_design_need(n: int, q: int, T: int, chunk: int, index32=False) -> int:
    """hu_permanova_design_need: the bytes of device memory that n samples, q design columns in T terms and `chunk` permutations per launch take"""
    lib = load_library()
    lib.hu_permanova_design_need.restype = C.c_int64
    return int(lib.hu_permanova_design_need(C.c_int64(int(n)), C.c_int64(int(q)), C.c_int64(int(T)), C.c_int64(int(chunk)), C.c_int32(1 if index32 else 0)))


def permanova_design_timing() -> dict:
    """hu_permanova_design_timing: the phases of this thread's last permanova_design on a device, in seconds"""
    s = np.zeros(4)
    _chk(load_library().hu_permanova_design_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], shuffle=s[1], quad=s[2], finish=s[3])


def dist_matrix_read(path) -> dict:
    """hu_dist_matrix_read (host only): the matrix hmmufotu-amd-unifrac -o writes, as dict(samples, dist [n][n])"""
    lib = load_library()
    h = C.c_void_p()
    _chk(lib.hu_dist_matrix_read(os.fsencode(str(path)), C.byref(h)))
    try:
        n = C.c_int64()
        _chk(lib.hu_dist_matrix_dims(h, C.byref(n)))
        lib.hu_dist_matrix_sample.restype = C.c_char_p
        lib.hu_dist_matrix_values.restype = C.POINTER(C.c_double)
        names = [lib.hu_dist_matrix_sample(h, C.c_int64(i)).decode() for i in range(n.value)]
        d = np.ctypeslib.as_array(lib.hu_dist_matrix_values(h), shape=(n.value, n.value)).copy() if n.value else np.zeros((0, 0))
        return dict(samples=names, dist=d)
    finally:
        lib.hu_dist_matrix_free(h)


class PcoaOpts(C.Structure):
    _fields_ = [("k", C.c_int64), ("oversample", C.c_int64), ("tol", C.c_double), ("max_it", C.c_int64), ("seed", C.c_uint64), ("host", C.c_int32), ("reserved", C.c_int32),
                ("mem_budget", C.c_int64)]


class PcoaResult(C.Structure):
    _fields_ = [("n", C.c_int64), ("k", C.c_int64), ("m_final", C.c_int64), ("iterations", C.c_int64), ("trace", C.c_double), ("positive_in_block", C.c_int64)]


def pcoa(dist, k=3, oversample=8, tol=1e-10, max_it=1000, seed=1, device=0, host=False, mem_budget=0) -> dict:
    """hu_pcoa: the k leading principal coordinates of the distance matrix dist [n][n]: dict(n, k, m_final, iterations, trace,
    positive_in_block, coords [n][k], eigval [k], resid [k], prop [k] = eigval / trace).  host: the library's host path, no device needed;
    the two paths agree within their residuals, not in their bits."""
    d = np.ascontiguousarray(dist, np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise EngineError("pcoa: dist [n][n]")
    lib = load_library()
    o = PcoaOpts()
    lib.hu_pcoa_default_opts(C.byref(o))
    o.k = int(k); o.oversample = int(oversample); o.tol = float(tol); o.max_it = int(max_it); o.seed = int(seed) & (2 ** 64 - 1); o.host = 1 if host else 0
    o.mem_budget = int(mem_budget or 0)
    r = PcoaResult()
    kk = max(int(k), 1)
    coords = np.zeros((d.shape[0], kk)); eig = np.zeros(kk); res = np.zeros(kk)
    _chk(lib.hu_pcoa(C.c_int(int(device)), C.c_int64(d.shape[0]), _p(d, C.c_double), C.byref(o), C.byref(r), _p(coords, C.c_double), _p(eig, C.c_double), _p(res, C.c_double)))
    out = {f: getattr(r, f) for f, _ in PcoaResult._fields_}
    out.update(coords=coords, eigval=eig, resid=res, prop=eig / r.trace)
    return out


def pcoa_need(n: int, k: int, oversample: int) -> int:
    """hu_pcoa_need: the bytes of device memory that n samples take with a block of min(k + oversample, n - 1) columns"""
    lib = load_library()
    lib.hu_pcoa_need.restype = C.c_int64
    return int(lib.hu_pcoa_need(C.c_int64(int(n)), C.c_int64(int(k)), C.c_int64(int(oversample))))


def pcoa_slabs(n: int) -> int:
    """hu_pcoa_slabs: the K slabs of the product kernel for n samples"""
    lib = load_library()
    lib.hu_pcoa_slabs.restype = C.c_int64
    return int(lib.hu_pcoa_slabs(C.c_int64(int(n))))


def pcoa_timing() -> dict:
    """hu_pcoa_timing: the phases of this thread's last pcoa, in seconds"""
    s = np.zeros(6)
    _chk(load_library().hu_pcoa_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], square=s[1], product=s[2], small=s[3], host_mxm=s[4], to_host=s[5])


class AlphaOpts(C.Structure):
    _fields_ = [("host", C.c_int32), ("chunk", C.c_int32), ("key_bits", C.c_int32), ("reserved", C.c_int32), ("draw_chunk", C.c_int64), ("mem_budget", C.c_int64)]


ALPHA_REC = np.dtype([("reads", np.uint64), ("S", np.uint64), ("F1", np.uint64), ("F2", np.uint64), ("Q", np.uint64), ("A", np.float64), ("PD", np.float64),
                      ("observed", np.float64), ("singles", np.float64), ("doubles", np.float64), ("chao1", np.float64), ("shannon", np.float64),
                      ("simpson", np.float64), ("goods_coverage", np.float64), ("faith_pd", np.float64)])


def _alpha_args(what, counts, otu_node, parent, blen, depths, host, chunk, key_bits, draw_chunk, mem_budget):
    c, _, tree, node, keep = _unifrac_args(what, counts, otu_node, parent, blen, "unweighted", None, 0, host, 0)
    o = AlphaOpts()
    load_library().hu_alpha_default_opts(C.byref(o))
    o.host = 1 if host else 0; o.key_bits = int(key_bits); o.draw_chunk = int(draw_chunk or 0); o.mem_budget = int(mem_budget or 0)
    if chunk is not None:
        o.chunk = int(chunk)
    if any(int(m) < 0 or int(m) >= 2 ** 64 for m in depths):
        raise EngineError(what + ": a depth is a whole number")
    d = np.array([int(m) for m in depths], np.uint64)
    return c, o, tree, node, d, keep


def alpha_diversity(counts, otu_node=None, parent=None, blen=None, depths=(), reps=0, seed=1, device=0, host=False, chunk=None, key_bits=64, draw_chunk=0, mem_budget=0) -> dict:
    """hu_alpha: the alpha diversity of every column of counts [otus][samples], and of its rarefied draws: dict(whole, draws), each a dict
    of named arrays (reads, S, F1, F2, Q, A, PD, observed, singles, doubles, chao1, shannon, simpson, goods_coverage, faith_pd); whole
    [samples], draws [samples][depths][reps].  The draw (j, m, r) is column j of otu_subset(counts, m, seed=seed + r); one that does not
    exist (m above the sample's reads) has reads 0 and NaN.  With a tree (parent [nodes] with -1 for the root, blen [nodes], otu_node [otus])
    PD is Faith's PD, without one NaN.  host, or device < 0: the library's host path, no device needed."""
    c, o, tree, node, d, keep = _alpha_args("alpha_diversity", counts, otu_node, parent, blen, depths, host or int(device) < 0, chunk, key_bits, draw_chunk, mem_budget)
    S = c.shape[1]
    R = int(reps)
    if S * len(d) * max(R, 0) > 2 ** 31:                            # the library's refusal, before the room for the draws is asked for
        raise EngineError("alpha_diversity: %d depths x %d repeats x %d samples: more than 2^31 draws" % (len(d), R, S))
    whole = np.zeros(S, ALPHA_REC); draws = np.zeros((S, len(d), max(R, 0)), ALPHA_REC)
    _chk(load_library().hu_alpha(C.c_int(int(device)), C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(S), node, _p(c, C.c_double),
                                 C.c_int64(len(d)), _p(d, C.c_uint64) if len(d) else None, C.c_int64(R), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(o),
                                 whole.ctypes.data_as(C.c_void_p), draws.ctypes.data_as(C.c_void_p) if draws.size else None))
    return dict(whole={f: whole[f].copy() for f in ALPHA_REC.names}, draws={f: draws[f].copy() for f in ALPHA_REC.names})


def alpha_sizes(counts, otu_node=None, parent=None, blen=None, depths=(), reps=0, chunk=None) -> dict:
    """hu_alpha_sizes: what alpha_need takes, for a call of alpha_diversity: dict(n_cell, n_entry, max_nnz, max_chunk, n_draw, n_branch);
    n_draw counts the whole samples too"""
    c, o, tree, node, d, keep = _alpha_args("alpha_sizes", counts, otu_node, parent, blen, depths, True, chunk, 64, 0, 0)
    out = np.zeros(6, np.int64)
    _chk(load_library().hu_alpha_sizes(C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), node, _p(c, C.c_double),
                                       C.c_int64(len(d)), _p(d, C.c_uint64) if len(d) else None, C.c_int64(int(reps)), C.byref(o), _p(out, C.c_int64)))
    return dict(zip(("n_cell", "n_entry", "max_nnz", "max_chunk", "n_draw", "n_branch"), (int(v) for v in out)))


def alpha_need(n_sample: int, n_cell: int, n_entry: int, max_nnz: int, max_chunk: int, n_draw: int) -> int:
    """hu_alpha_need: the bytes of device memory for n_draw resident draws"""
    lib = load_library()
    lib.hu_alpha_need.restype = C.c_int64
    return int(lib.hu_alpha_need(*(C.c_int64(int(v)) for v in (n_sample, n_cell, n_entry, max_nnz, max_chunk, n_draw))))


def alpha_timing() -> dict:
    """hu_alpha_timing: the phases of this thread's last alpha_diversity on a device, in seconds"""
    s = np.zeros(6)
    _chk(load_library().hu_alpha_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], select=s[1], take=s[2], metrics=s[3], pd=s[4], to_host=s[5])


class UnifracRarefiedOpts(C.Structure):
    _fields_ = [("method", C.c_int32), ("host", C.c_int32), ("alpha", C.c_double), ("slab", C.c_int64), ("chunk", C.c_int32), ("key_bits", C.c_int32),
                ("draw_chunk", C.c_int64), ("mem_budget", C.c_int64)]


def _unifrac_rarefied_args(what, counts, otu_node, parent, blen, depth, reps, method, alpha, slab, host, chunk, key_bits, draw_chunk, mem_budget):
    c, uo, tree, node, keep = _unifrac_args(what, counts, otu_node, parent, blen, method, alpha, slab, host, 0)
    o = UnifracRarefiedOpts()
    load_library().hu_unifrac_rarefied_default_opts(C.byref(o))
    o.method = uo.method; o.host = 1 if host else 0; o.alpha = uo.alpha; o.slab = uo.slab; o.key_bits = int(key_bits)
    o.draw_chunk = int(draw_chunk or 0); o.mem_budget = int(mem_budget or 0)
    if chunk is not None:
        o.chunk = int(chunk)
    if int(depth) < 0 or int(depth) >= 2 ** 64:
        raise EngineError(what + ": the depth is a whole number")
    return c, o, tree, node, keep


def unifrac_rarefied_sizes(counts, otu_node=None, parent=None, blen=None, depth=1, reps=1, method="weighted", alpha=None, slab=0, chunk=None) -> dict:
    """hu_unifrac_rarefied_sizes (host only): what unifrac_rarefied_need takes, for a call of unifrac_rarefied: dict(n_kept, n_cell, n_entry,
    max_nnz, max_chunk, n_branch, slab, max_depth2); max_depth2 is the largest depth that keeps 2 samples"""
    c, o, tree, node, keep = _unifrac_rarefied_args("unifrac_rarefied_sizes", counts, otu_node, parent, blen, depth, reps, method, alpha, slab, True, chunk, 64, 0, 0)
    out = np.zeros(8, np.int64)
    _chk(load_library().hu_unifrac_rarefied_sizes(C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), node, _p(c, C.c_double),
                                                  C.c_uint64(int(depth)), C.c_int64(int(reps)), C.byref(o), _p(out, C.c_int64)))
    return dict(zip(("n_kept", "n_cell", "n_entry", "max_nnz", "max_chunk", "n_branch", "slab", "max_depth2"), (int(v) for v in out)))


def unifrac_rarefied(counts, otu_node=None, parent=None, blen=None, depth=None, reps=None, seed=1, method="weighted", alpha=None, slab=0, device=0, host=False,
                     chunk=None, key_bits=64, draw_chunk=0, mem_budget=0, draws=False) -> dict:
    """hu_unifrac_rarefied: the distances of unifrac averaged over `reps` rarefied draws of `depth` reads: dict(mean [S'][S'], sd [S'][S'],
    kept [samples] bool, and with draws=True draws [reps][S'][S']).  The S' kept samples are the columns with at least `depth` reads, in
    table order.  Draw r is otu_subset(counts, depth, seed=seed + r) of the whole table, its distances those of unifrac on the kept columns
    with the slab of (S', B); mean and sd follow Welford's recurrence in ascending r (sd is NaN for reps == 1).  host, or device < 0: the
    library's host path, no device needed."""
    if depth is None or reps is None:
        raise EngineError("unifrac_rarefied: depth and reps are required")
    hst = host or int(device) < 0
    c, o, tree, node, keep = _unifrac_rarefied_args("unifrac_rarefied", counts, otu_node, parent, blen, depth, reps, method, alpha, slab, hst, chunk, key_bits, draw_chunk, mem_budget)
    S = c.shape[1]
    R = int(reps)
    tot = c.sum(axis=0) if c.size else np.zeros(S)
    Sk = int(np.count_nonzero(tot >= int(depth))) if int(depth) > 0 else S      # the room only: the library counts for itself
    kept = np.zeros(S, np.uint8); mean = np.zeros((Sk, Sk)); sd = np.zeros((Sk, Sk))
    dr = np.zeros((R, Sk, Sk)) if draws and 0 < R <= 100000 else None
    _chk(load_library().hu_unifrac_rarefied(C.c_int(int(device)), C.byref(tree) if tree is not None else None, C.c_int64(c.shape[0]), C.c_int64(S), node, _p(c, C.c_double),
                                            C.c_uint64(int(depth)), C.c_int64(R), C.c_uint64(int(seed) & (2 ** 64 - 1)), C.byref(o), _p(kept, C.c_uint8),
                                            _p(mean, C.c_double), _p(sd, C.c_double), _p(dr, C.c_double) if dr is not None else None))
    out = dict(mean=mean, sd=sd, kept=kept.astype(bool))
    if draws:
        out["draws"] = dr
    return out


def unifrac_rarefied_need(n_sample: int, n_kept: int, n_cell: int, n_entry: int, max_nnz: int, max_chunk: int, n_branch: int, slab: int, draw_chunk: int,
                          want_draws: bool = False) -> int:
    """hu_unifrac_rarefied_need: the bytes of device memory for draw_chunk resident draws"""
    lib = load_library()
    lib.hu_unifrac_rarefied_need.restype = C.c_int64
    return int(lib.hu_unifrac_rarefied_need(*(C.c_int64(int(v)) for v in (n_sample, n_kept, n_cell, n_entry, max_nnz, max_chunk, n_branch, slab, draw_chunk)),
                                            C.c_int32(1 if want_draws else 0)))


def unifrac_rarefied_timing() -> dict:
    """hu_unifrac_rarefied_timing: the phases of this thread's last unifrac_rarefied on a device, in seconds, and the draws that were resident at once"""
    s = np.zeros(6)
    n = C.c_int64(0)
    _chk(load_library().hu_unifrac_rarefied_timing(_p(s, C.c_double), C.byref(n)))
    return dict(to_device=s[0], draws=s[1], embed=s[2], pairs=s[3], accumulate=s[4], to_host=s[5], resident_draws=int(n.value))


class DiffabundOpts(C.Structure):
    _fields_ = [("perms", C.c_int64), ("seed", C.c_uint64), ("host", C.c_int32), ("rank_by", C.c_int32), ("min_prevalence", C.c_int64), ("chunk", C.c_int64),
                ("mem_budget", C.c_int64)]


DIFFABUND_REC = np.dtype([("tested", np.int32), ("best", np.int32), ("prevalence", np.int64), ("T_hi", np.uint64), ("T_lo", np.uint64), ("count_ge", np.int64),
                          ("H", np.float64), ("p", np.float64), ("p_maxT", np.float64), ("q", np.float64)])
RANK_BY = {"fraction": 0, "count": 1}


def diffabund(counts, group, perms=999, seed=1, rank_by="fraction", min_prevalence=1, chunk=0, device=0, host=False, mem_budget=0) -> dict:
    """hu_diffabund: Kruskal-Wallis per OTU of counts [n_otu][n_sample] between the labels group [n_sample] (0 .. a-1), with permutation
    p-values, single-step maxT and Benjamini-Hochberg: dict(rec, a structured array [n_otu] of tested, best, prevalence, T_hi, T_lo, count_ge,
    H, p, p_maxT, q (NaN and best -1 where an OTU is not tested), and max_H [perms], the largest H of every permutation).  host: the
    library's host path, no device needed; it gives the same bits."""
    c = np.ascontiguousarray(counts, np.float64); g = np.ascontiguousarray(group, np.int32)
    if c.ndim != 2 or g.shape != (c.shape[1],):
        raise EngineError("diffabund: counts [n_otu][n_sample] and group [n_sample]")
    if rank_by not in RANK_BY:
        raise EngineError("diffabund: rank_by is 'fraction' or 'count'")
    lib = load_library()
    o = DiffabundOpts()
    lib.hu_diffabund_default_opts(C.byref(o))
    o.perms = int(perms); o.seed = int(seed) & (2 ** 64 - 1); o.host = 1 if host else 0; o.rank_by = RANK_BY[rank_by]; o.min_prevalence = int(min_prevalence)
    o.chunk = int(chunk or 0); o.mem_budget = int(mem_budget or 0)
    rec = np.zeros(c.shape[0], DIFFABUND_REC)
    mx = np.zeros(max(int(perms), 0))
    _chk(lib.hu_diffabund(C.c_int(int(device)), C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), _p(c, C.c_double), _p(g, C.c_int32), C.byref(o),
                          rec.ctypes.data_as(C.c_void_p), _p(mx, C.c_double) if len(mx) else None))
    return dict(rec=rec, max_H=mx)


def diffabund_ranks(counts, rank_by="fraction") -> np.ndarray:
    """hu_diffabund_ranks (host only): [n_otu][n_sample], the doubled mid-ranks of every OTU's cells among its samples"""
    c = np.ascontiguousarray(counts, np.float64)
    if c.ndim != 2 or rank_by not in RANK_BY:
        raise EngineError("diffabund_ranks: counts [n_otu][n_sample], rank_by 'fraction' or 'count'")
    out = np.zeros(c.shape, np.int32)
    _chk(load_library().hu_diffabund_ranks(C.c_int64(c.shape[0]), C.c_int64(c.shape[1]), _p(c, C.c_double), C.c_int32(RANK_BY[rank_by]), _p(out, C.c_int32)))
    return out


def diffabund_need(n_sample: int, a: int, n_otu: int, n_cell: int, chunk: int) -> int:
    """hu_diffabund_need: the bytes of device memory for n_otu tested OTUs with n_cell cells above 0 and `chunk` permutations per launch"""
    lib = load_library()
    lib.hu_diffabund_need.restype = C.c_int64
    return int(lib.hu_diffabund_need(*(C.c_int64(int(v)) for v in (n_sample, a, n_otu, n_cell, chunk))))


def diffabund_timing() -> dict:
    """hu_diffabund_timing: the phases of this thread's last diffabund on a device, in seconds"""
    s = np.zeros(4)
    _chk(load_library().hu_diffabund_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], shuffle=s[1], sums=s[2], finish=s[3])


class NjOpts(C.Structure):
    _fields_ = [("host", C.c_int32), ("reserved", C.c_int32), ("mem_budget", C.c_int64)]


DIST_TYPES = {"pdist": 0, "JC69": 1, "K80": 2, "F81": 3, "HKY85": 4, "TN93": 5}


def _code_rows(rows, what) -> np.ndarray:
    a = np.ascontiguousarray(rows, np.int8)
    if a.ndim != 2 or a.size == 0:
        raise EngineError(what + ": rows must be a non-empty int8 [n][cs_len] array of the codes of msa_encode_table")
    return a


def msa_pair_counts(rows, device=0, host=False) -> np.ndarray:
    """hu_msa_pair_counts: int32 [n][n][4] = per pair of rows (codes of msa_encode_table, int8 [n][cs_len]) N, P_R, P_Y and Q: the
    columns where both hold a symbol, the A<->G and the C<->T differences, the transversions.  host: the library's host path."""
    a = _code_rows(rows, "msa_pair_counts")
    n, L = a.shape
    out = np.zeros((n, n, 4), np.int32)
    _chk(load_library().hu_msa_pair_counts(C.c_int(-1 if host else int(device)), C.c_int64(n), C.c_int64(L), _p(a, C.c_int8), _p(out, C.c_int32)))
    return out


def msa_distances(rows, dist="JC69", pi=None, sat=None, device=0, host=False):
    """hu_msa_distances: (D [n][n], saturated pairs) of the rows under dist (one of DIST_TYPES); pi [4] goes into F81, HKY85 and TN93;
    sat: the distance of a saturated pair, None for twice the largest finite distance.  host: the library's host path."""
    a = _code_rows(rows, "msa_distances")
    if dist not in DIST_TYPES:
        raise EngineError("msa_distances: dist one of %s, not %r" % (", ".join(DIST_TYPES), dist))
    n, L = a.shape
    D = np.zeros((n, n)); ns = C.c_int64(0)
    p = np.ascontiguousarray(pi, np.float64) if pi is not None else None
    if p is not None and p.shape != (4,):
        raise EngineError("msa_distances: pi [4]")
    _chk(load_library().hu_msa_distances(C.c_int(-1 if host else int(device)), C.c_int64(n), C.c_int64(L), _p(a, C.c_int8), C.c_int(DIST_TYPES[dist]),
                                         _p(p, C.c_double) if p is not None else None, C.c_double(0.0 if sat is None else float(sat)), _p(D, C.c_double), C.byref(ns)))
    return D, int(ns.value)


def nj(D, device=0, host=False, mem_budget=0) -> dict:
    """hu_nj: neighbour joining on the symmetric matrix D [n][n] with a zero diagonal: dict(join [n - 3][2], len [n - 3][2], last3 [3],
    last_len3 [3]); join t makes node n + t.  The host path (host=True) and the device give the same bits."""
    d = np.ascontiguousarray(D, np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise EngineError("nj: D [n][n]")
    n = d.shape[0]
    o = NjOpts()
    load_library().hu_nj_default_opts(C.byref(o))
    o.host = 1 if host else 0; o.mem_budget = int(mem_budget or 0)
    m = max(n - 3, 0)
    out = dict(join=np.zeros((m, 2), np.int32), len=np.zeros((m, 2)), last3=np.zeros(3, np.int32), last_len3=np.zeros(3))
    _chk(load_library().hu_nj(C.c_int(int(device)), C.c_int64(n), _p(d, C.c_double), C.byref(o), _p(out["join"], C.c_int32) if m else None,
                              _p(out["len"], C.c_double) if m else None, _p(out["last3"], C.c_int32), _p(out["last_len3"], C.c_double)))
    return out


def nj_newick(names, tree) -> str:
    """hu_nj_newick: the result of nj as Newick text, unrooted with three children at the top node; leaves carry names, lengths %.17g"""
    lib = load_library()
    lib.hu_nj_newick.restype = C.c_int64
    n = len(names)
    nm = (C.c_char_p * n)(*[x.encode() if isinstance(x, str) else bytes(x) for x in names])
    j = np.ascontiguousarray(tree["join"], np.int32); l = np.ascontiguousarray(tree["len"], np.float64)
    l3 = np.ascontiguousarray(tree["last3"], np.int32); ll3 = np.ascontiguousarray(tree["last_len3"], np.float64)
    if j.shape != (max(n - 3, 0), 2) or l.shape != j.shape or l3.shape != (3,) or ll3.shape != (3,):
        raise EngineError("nj_newick: the arrays of nj for %d names" % n)
    args = (C.c_int64(n), nm, _p(j, C.c_int32) if j.size else None, _p(l, C.c_double) if l.size else None, _p(l3, C.c_int32), _p(ll3, C.c_double))
    k = int(lib.hu_nj_newick(*args, None, C.c_int64(0)))
    if k < 0:
        _chk(k)
    buf = C.create_string_buffer(k + 1)
    _chk(min(0, int(lib.hu_nj_newick(*args, buf, C.c_int64(k + 1)))))
    return buf.value.decode()


def nj_timing() -> dict:
    """hu_nj_timing: the phases of this thread's last msa_distances / nj on a device, in seconds"""
    s = np.zeros(4)
    _chk(load_library().hu_nj_timing(_p(s, C.c_double)))
    return dict(to_device=s[0], distances=s[1], joins=s[2], to_host=s[3])


class BlenRound(C.Structure):
    _fields_ = [("ll", C.c_double), ("s", C.c_double), ("delta", C.c_double), ("n_capped", C.c_int64)]


class BlenOpts(C.Structure):
    _fields_ = [("eps", C.c_double), ("min_len", C.c_double), ("max_len", C.c_double), ("max_rounds", C.c_int32), ("host", C.c_int32),
                ("device", C.c_int32), ("rounds_cap", C.c_int32), ("mem_budget", C.c_int64), ("rounds", C.POINTER(BlenRound)),
                ("n_rounds", C.c_int32), ("stop", C.c_int32), ("ll_start", C.c_double), ("ll_final", C.c_double), ("n_capped", C.c_int64)]


BLEN_TAU = 1e-8
BLEN_LDS_COLS = 1450
BLEN_STOP = ("converged", "no improving step", "max rounds")


def _blen_args(what, parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget):
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64).copy()
    seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError(what + ": parent [n], blen [n] and seq [n][cs_len]")
    o = BlenOpts()
    load_library().hu_blen_default_opts(C.byref(o))
    if eps is not None:
        o.eps = float(eps)
    if min_len is not None:
        o.min_len = float(min_len)
    if max_len is not None:
        o.max_len = float(max_len)
    if max_rounds is not None:
        o.max_rounds = int(max_rounds)
    o.host = 1 if host else 0; o.device = int(device); o.mem_budget = int(mem_budget or 0)
    n, L = seq.shape
    head = (C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8), C.byref(model))
    return o, blen, n, head


def blen_need(n_nodes: int, cs_len: int) -> int:
    """hu_blen_need: the bytes the branch-length fit holds for n_nodes x cs_len"""
    lib = load_library()
    lib.hu_blen_need.restype = C.c_int64
    return int(lib.hu_blen_need(C.c_int32(n_nodes), C.c_int32(cs_len)))


def tree_branch_scores(parent, blen, seq, model: ModelDesc, t=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_branch_scores: f_u, f_u', f_u'' [n] of every branch at t [n] (None: at blen), all other lengths as in blen; seq [n][cs_len]
    holds the leaf rows in the codes of msa_encode_table.  The root's entries are 0.  host: the library's host path."""
    o, blen, n, head = _blen_args("tree_branch_scores", parent, blen, seq, model, None, None, None, None, device, host, mem_budget)
    tt = np.ascontiguousarray(t, np.float64) if t is not None else None
    if tt is not None and tt.shape != (n,):
        raise EngineError("tree_branch_scores: t [n]")
    out = dict(f=np.zeros(n), d1=np.zeros(n), d2=np.zeros(n))
    _chk(load_library().hu_tree_branch_scores(*head, _p(tt, C.c_double) if tt is not None else None, _p(out["f"], C.c_double),
                                              _p(out["d1"], C.c_double), _p(out["d2"], C.c_double)))
    return out


def tree_branch_step(parent, blen, seq, model: ModelDesc, min_len=None, max_len=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_branch_step: t_star [n], the maximiser of every f_u on [min_len, max_len] with the other lengths as in blen, to BLEN_TAU;
    f, d1, d2 at blen; capped [n]: the branches that hit the Newton cap"""
    o, blen, n, head = _blen_args("tree_branch_step", parent, blen, seq, model, None, min_len, max_len, None, device, host, mem_budget)
    out = dict(t_star=np.zeros(n), f=np.zeros(n), d1=np.zeros(n), d2=np.zeros(n), capped=np.zeros(n, np.uint8))
    _chk(load_library().hu_tree_branch_step(*head, _p(out["t_star"], C.c_double), _p(out["f"], C.c_double), _p(out["d1"], C.c_double),
                                            _p(out["d2"], C.c_double), _p(out["capped"], C.c_uint8)))
    out["n_capped"] = int(o.n_capped)
    return out


def tree_optimize_lengths(parent, blen, seq, model: ModelDesc, eps=None, min_len=None, max_len=None, max_rounds=None, device=0, host=False,
                          mem_budget=0) -> dict:
    """hu_tree_optimize_lengths: rounds of simultaneous branch steps with a halved step until the log-likelihood rises.  dict(blen [n],
    ll_start, ll_final, stop (one of BLEN_STOP), rounds: per accepted round (ll, s, delta, n_capped), n_capped, seconds)"""
    o, blen, n, head = _blen_args("tree_optimize_lengths", parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget)
    cap = max(int(o.max_rounds), 1)
    rec = (BlenRound * cap)()
    o.rounds = C.cast(rec, C.POINTER(BlenRound)); o.rounds_cap = cap
    _chk(load_library().hu_tree_optimize_lengths(*head))
    s = np.zeros(4)
    _chk(load_library().hu_blen_timing(_p(s, C.c_double)))
    return dict(blen=blen, ll_start=float(o.ll_start), ll_final=float(o.ll_final), stop=BLEN_STOP[o.stop], n_capped=int(o.n_capped),
                rounds=[dict(ll=r.ll, s=r.s, delta=r.delta, n_capped=int(r.n_capped)) for r in rec[:o.n_rounds]],
                seconds=dict(sweep=s[0], step=s[1], trial=s[2], other=s[3]))


class GammaPass(C.Structure):
    _fields_ = [("alpha", C.c_double), ("ll", C.c_double), ("n_rounds", C.c_int32), ("reserved", C.c_int32)]


class GammaOpts(C.Structure):
    _fields_ = [("blen", BlenOpts), ("k", C.c_int32), ("max_outer", C.c_int32), ("alpha", C.c_double), ("eps_ll", C.c_double),
                ("sweep_reruns", C.c_int32), ("passes_cap", C.c_int32), ("passes", C.POINTER(GammaPass)),
                ("n_outer", C.c_int32), ("stop", C.c_int32), ("alpha_fit", C.c_double), ("rates", C.c_double * 16),
                ("ll_start", C.c_double), ("ll_final", C.c_double), ("n_capped", C.c_int64)]


GAMMA_ALPHA_MIN, GAMMA_ALPHA_MAX = 0.05, 100.0
GAMMA_LDS_BYTES = 40960
GAMMA_STOP = ("converged", "max passes", "fixed alpha")


def gamma_lds_cols(k: int) -> int:
    """the columns up to which the 4 K values of a branch's columns stay in LDS (hu_gamma_in_lds)"""
    return (GAMMA_LDS_BYTES // 8 - 3 * 256 - (9 * k + (9 * k & 1))) // (4 * k)


def gamma_rates(k: int, alpha: float) -> np.ndarray:
    """hu_gamma_rates: the K category rates of the discrete Gamma with shape alpha, mean 1"""
    r = np.zeros(max(int(k), 1))
    _chk(load_library().hu_gamma_rates(C.c_int32(int(k)), C.c_double(float(alpha)), _p(r, C.c_double)))
    return r


def gamma_need(n_nodes: int, cs_len: int, k: int) -> int:
    """hu_gamma_need: the bytes the fit under the discrete Gamma holds for n_nodes x cs_len in k categories"""
    lib = load_library()
    lib.hu_gamma_need.restype = C.c_int64
    return int(lib.hu_gamma_need(C.c_int32(n_nodes), C.c_int32(cs_len), C.c_int32(k)))


def _gamma_args(what, parent, blen, seq, model, k, alpha, eps, min_len, max_len, max_rounds, device, host, mem_budget, max_outer=None, eps_ll=None,
                sweep_reruns=False):
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64).copy()
    seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError(what + ": parent [n], blen [n] and seq [n][cs_len]")
    o = GammaOpts()
    load_library().hu_gamma_default_opts(C.byref(o))
    for key, v in (("eps", eps), ("min_len", min_len), ("max_len", max_len)):
        if v is not None:
            setattr(o.blen, key, float(v))
    if max_rounds is not None:
        o.blen.max_rounds = int(max_rounds)
    o.blen.host = 1 if host else 0; o.blen.device = int(device); o.blen.mem_budget = int(mem_budget or 0)
    o.k = int(k); o.alpha = float(alpha or 0.0); o.sweep_reruns = 1 if sweep_reruns else 0
    if max_outer is not None:
        o.max_outer = int(max_outer)
    if eps_ll is not None:
        o.eps_ll = float(eps_ll)
    n, L = seq.shape
    head = (C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8), C.byref(model))
    return o, blen, n, L, head


def tree_gamma_loglik(parent, blen, seq, model: ModelDesc, k=4, alpha=1.0, device=0, host=False, mem_budget=0, sweep_reruns=False) -> dict:
    """hu_tree_gamma_loglik: dict(ll, per_col [cs_len], per_cat [k][cs_len]) under the discrete Gamma of k rates with shape alpha"""
    o, blen, n, L, head = _gamma_args("tree_gamma_loglik", parent, blen, seq, model, k, alpha, None, None, None, None, device, host, mem_budget,
                                      sweep_reruns=sweep_reruns)
    out = dict(per_col=np.zeros(L), per_cat=np.zeros((max(int(k), 1), L)))
    ll = C.c_double(0)
    _chk(load_library().hu_tree_gamma_loglik(*head, _p(out["per_col"], C.c_double), _p(out["per_cat"], C.c_double), C.byref(ll)))
    out["ll"] = float(ll.value)
    return out


def tree_gamma_branch_scores(parent, blen, seq, model: ModelDesc, k=4, alpha=1.0, t=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_gamma_branch_scores: tree_branch_scores for the objective under the discrete Gamma of k rates with shape alpha"""
    o, blen, n, L, head = _gamma_args("tree_gamma_branch_scores", parent, blen, seq, model, k, alpha, None, None, None, None, device, host, mem_budget)
    tt = np.ascontiguousarray(t, np.float64) if t is not None else None
    if tt is not None and tt.shape != (n,):
        raise EngineError("tree_gamma_branch_scores: t [n]")
    out = dict(f=np.zeros(n), d1=np.zeros(n), d2=np.zeros(n))
    _chk(load_library().hu_tree_gamma_branch_scores(*head, _p(tt, C.c_double) if tt is not None else None, _p(out["f"], C.c_double),
                                                    _p(out["d1"], C.c_double), _p(out["d2"], C.c_double)))
    return out


def tree_gamma_branch_step(parent, blen, seq, model: ModelDesc, k=4, alpha=1.0, min_len=None, max_len=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_gamma_branch_step: tree_branch_step for the objective under the discrete Gamma of k rates with shape alpha"""
    o, blen, n, L, head = _gamma_args("tree_gamma_branch_step", parent, blen, seq, model, k, alpha, None, min_len, max_len, None, device, host, mem_budget)
    out = dict(t_star=np.zeros(n), f=np.zeros(n), d1=np.zeros(n), d2=np.zeros(n), capped=np.zeros(n, np.uint8))
    _chk(load_library().hu_tree_gamma_branch_step(*head, _p(out["t_star"], C.c_double), _p(out["f"], C.c_double), _p(out["d1"], C.c_double),
                                                  _p(out["d2"], C.c_double), _p(out["capped"], C.c_uint8)))
    out["n_capped"] = int(o.n_capped)
    return out


def tree_gamma_fit(parent, blen, seq, model: ModelDesc, k=4, alpha=None, max_outer=None, eps_ll=None, eps=None, min_len=None, max_len=None,
                   max_rounds=None, device=0, host=False, mem_budget=0, sweep_reruns=False) -> dict:
    """hu_tree_gamma_fit: the lengths and, with alpha None, the shape by maximum likelihood under the discrete Gamma of k rates.
    dict(blen [n], alpha, rates [k], ll_start, ll_final, stop (one of GAMMA_STOP), passes: per pass (alpha, ll, n_rounds), n_capped, seconds)"""
    o, blen, n, L, head = _gamma_args("tree_gamma_fit", parent, blen, seq, model, k, alpha, eps, min_len, max_len, max_rounds, device, host, mem_budget,
                                      max_outer, eps_ll, sweep_reruns)
    cap = max(int(o.max_outer), 1)
    rec = (GammaPass * cap)()
    o.passes = C.cast(rec, C.POINTER(GammaPass)); o.passes_cap = cap
    _chk(load_library().hu_tree_gamma_fit(*head))
    s = np.zeros(5)
    _chk(load_library().hu_gamma_timing(_p(s, C.c_double)))
    return dict(blen=blen, alpha=float(o.alpha_fit), rates=np.array(o.rates[:int(k)]), ll_start=float(o.ll_start), ll_final=float(o.ll_final),
                stop=GAMMA_STOP[o.stop], n_capped=int(o.n_capped),
                passes=[dict(alpha=r.alpha, ll=r.ll, n_rounds=int(r.n_rounds)) for r in rec[:o.n_outer]],
                seconds=dict(shape=s[0], sweep=s[1], step=s[2], trial=s[3], other=s[4]))


def gamma_profile(parent, blen, seq, model: ModelDesc, k=4, alpha=1.0, reps=6, device=0, sweep_reruns=False) -> np.ndarray:
    """hu_gamma_profile: seconds [reps][3] of a full sweep, a step and a trial sweep with its log-likelihood on the device"""
    o, blen, n, L, head = _gamma_args("gamma_profile", parent, blen, seq, model, k, alpha, None, None, None, None, device, False, 0, sweep_reruns=sweep_reruns)
    s = np.zeros((int(reps), 3))
    _chk(load_library().hu_gamma_profile(*head, C.c_int32(int(reps)), _p(s, C.c_double)))
    return s


def newick_write(text, blen) -> str:
    """hu_newick_parse + hu_newick_write: the tree of `text` with the lengths blen [n] (node ids of newick_parse), 17 significant digits"""
    lib = load_library()
    lib.hu_newick_write.restype = C.c_int64
    raw = text.encode() if isinstance(text, str) else bytes(text)
    h = C.c_void_p()
    _chk(lib.hu_newick_parse(raw, C.c_int64(len(raw)), C.byref(h)))
    try:
        n = C.c_int32(0)
        lib.hu_newick_size(h, C.byref(n))
        b = np.ascontiguousarray(blen, np.float64)
        if b.shape != (n.value,):
            raise EngineError("newick_write: blen [%d]" % n.value)
        k = int(lib.hu_newick_write(h, _p(b, C.c_double), None, C.c_int64(0)))
        if k < 0:
            _chk(k)
        buf = C.create_string_buffer(k + 1)
        lib.hu_newick_write(h, _p(b, C.c_double), buf, C.c_int64(k + 1))
        return buf.value.decode()
    finally:
        lib.hu_newick_free(h)


class NniRound(C.Structure):
    _fields_ = [("ll", C.c_double), ("scored", C.c_int32), ("candidates", C.c_int32), ("taken", C.c_int32), ("applied", C.c_int32)]


class NniOpts(C.Structure):
    _fields_ = [("blen", BlenOpts), ("min_gain", C.c_double), ("nni_rounds", C.c_int32), ("rounds_cap", C.c_int32),
                ("rounds", C.POINTER(NniRound)), ("swaps", C.POINTER(C.c_int32)), ("swaps_cap", C.c_int64),
                ("n_rounds", C.c_int32), ("stop", C.c_int32), ("n_swaps", C.c_int64), ("skipped", C.c_int64),
                ("ll_start", C.c_double), ("ll_final", C.c_double)]


NNI_LDS_COLS = 483
NNI_STOP = ("local optimum", "no improving swap", "max rounds")


def _nni_args(what, parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget, nni_rounds=None, min_gain=None):
    parent = np.ascontiguousarray(parent, np.int32).copy(); blen = np.ascontiguousarray(blen, np.float64).copy()
    seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError(what + ": parent [n], blen [n] and seq [n][cs_len]")
    o = NniOpts()
    load_library().hu_nni_default_opts(C.byref(o))
    for k, v in (("eps", eps), ("min_len", min_len), ("max_len", max_len)):
        if v is not None:
            setattr(o.blen, k, float(v))
    if max_rounds is not None:
        o.blen.max_rounds = int(max_rounds)
    if nni_rounds is not None:
        o.nni_rounds = int(nni_rounds)
    if min_gain is not None:
        o.min_gain = float(min_gain)
    o.blen.host = 1 if host else 0; o.blen.device = int(device); o.blen.mem_budget = int(mem_budget or 0)
    return o, parent, blen, seq


def nni_need(n_nodes: int, cs_len: int) -> int:
    """hu_nni_need: the bytes the NNI search holds for n_nodes x cs_len"""
    lib = load_library()
    lib.hu_nni_need.restype = C.c_int64
    return int(lib.hu_nni_need(C.c_int32(n_nodes), C.c_int32(cs_len)))


def tree_nni_scores(parent, blen, seq, model: ModelDesc, min_len=None, max_len=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_nni_scores: for the E eligible edges in ascending u, dict(edge_node [E], t_star [E][3], f [E][3], f0_at_blen [E], skipped):
    the optimum and the value of the edge's three arrangements (0: as it stands, 1: B and C exchanged, 2: A and C exchanged)"""
    o, parent, blen, seq = _nni_args("tree_nni_scores", parent, blen, seq, model, None, min_len, max_len, None, device, host, mem_budget)
    n, L = seq.shape
    cap = max((n - 1) // 2, 1)
    node = np.zeros(cap, np.int32); ts = np.zeros((cap, 3)); f = np.zeros((cap, 3)); f0 = np.zeros(cap)
    ne = C.c_int32(0); sk = C.c_int64(0)
    _chk(load_library().hu_tree_nni_scores(C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                           C.byref(model), C.c_int32(cap), C.byref(ne), C.byref(sk), _p(node, C.c_int32), _p(ts, C.c_double),
                                           _p(f, C.c_double), _p(f0, C.c_double)))
    e = ne.value
    return dict(edge_node=node[:e].copy(), t_star=ts[:e].copy(), f=f[:e].copy(), f0_at_blen=f0[:e].copy(), skipped=int(sk.value))


def _child_arrays(parent, child_off, child_idx):
    """the order of children: as given, or in node-id order"""
    n = len(parent)
    if child_off is not None:
        return np.ascontiguousarray(child_off, np.int32).copy(), np.ascontiguousarray(child_idx, np.int32).copy()
    off = np.zeros(n + 1, np.int32)
    for p in parent:
        if p >= 0:
            off[p + 1] += 1
    off = np.cumsum(off).astype(np.int32)
    idx = np.zeros(max(n - 1, 1), np.int32); fill = off[:-1].copy()
    for i, p in enumerate(parent):
        if p >= 0:
            idx[fill[p]] = i; fill[p] += 1
    return off, idx


def tree_nni_apply(parent, blen, u: int, q: int, t: float, child_off=None, child_idx=None) -> dict:
    """hu_tree_nni_apply: arrangement q (1: B and C exchanged, 2: A and C exchanged) of the edge above u, its central length set to t.
    dict(parent, blen, child_off, child_idx), the inputs are not changed"""
    parent = np.ascontiguousarray(parent, np.int32).copy(); blen = np.ascontiguousarray(blen, np.float64).copy()
    off, idx = _child_arrays(parent, child_off, child_idx)
    _chk(load_library().hu_tree_nni_apply(C.c_int32(len(parent)), _p(parent, C.c_int32), _p(blen, C.c_double), _p(off, C.c_int32), _p(idx, C.c_int32),
                                          C.c_int32(int(u)), C.c_int32(int(q)), C.c_double(float(t))))
    return dict(parent=parent, blen=blen, child_off=off, child_idx=idx)


def tree_nni_search(parent, blen, seq, model: ModelDesc, child_off=None, child_idx=None, nni_rounds=None, min_gain=None, eps=None, min_len=None,
                    max_len=None, max_rounds=None, device=0, host=False, mem_budget=0) -> dict:
    """hu_tree_nni_search: the hill climb over NNIs.  dict(parent, blen, child_off, child_idx, ll_start, ll_final, stop (one of NNI_STOP),
    skipped, rounds: per accepted round (ll, scored, candidates, taken, applied), swaps: per applied swap (round, u, q), seconds)"""
    o, parent, blen, seq = _nni_args("tree_nni_search", parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget,
                                     nni_rounds, min_gain)
    n, L = seq.shape
    off, idx = _child_arrays(parent, child_off, child_idx)
    cap = max(int(o.nni_rounds), 1)
    rec = (NniRound * cap)()
    scap = cap * max((n - 1) // 2, 1)
    sw = np.zeros((scap, 3), np.int32)
    o.rounds = C.cast(rec, C.POINTER(NniRound)); o.rounds_cap = cap; o.swaps = _p(sw, C.c_int32); o.swaps_cap = scap
    _chk(load_library().hu_tree_nni_search(C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                           _p(off, C.c_int32), _p(idx, C.c_int32), C.byref(model)))
    s = np.zeros(4)
    _chk(load_library().hu_nni_timing(_p(s, C.c_double)))
    return dict(parent=parent, blen=blen, child_off=off, child_idx=idx, ll_start=float(o.ll_start), ll_final=float(o.ll_final), stop=NNI_STOP[o.stop],
                skipped=int(o.skipped),
                rounds=[dict(ll=r.ll, scored=r.scored, candidates=r.candidates, taken=r.taken, applied=r.applied) for r in rec[:o.n_rounds]],
                swaps=[tuple(int(x) for x in row) for row in sw[:o.n_swaps]], seconds=dict(fit=s[0], score=s[1], trial=s[2], other=s[3]))


def newick_from_arrays(parent, child_off, child_idx, names, blen) -> str:
    """hu_newick_from_arrays: Newick text from parent, the order of children, names ("" or None for none) and blen"""
    lib = load_library()
    lib.hu_newick_from_arrays.restype = C.c_int64
    parent = np.ascontiguousarray(parent, np.int32); n = len(parent)
    off, idx = _child_arrays(parent, child_off, child_idx)
    b = np.ascontiguousarray(blen, np.float64)
    if b.shape != (n,) or len(names) != n:
        raise EngineError("newick_from_arrays: blen [n] and names [n]")
    nm = (C.c_char_p * n)(*[(x or "").encode() for x in names])
    head = (C.c_int32(n), _p(parent, C.c_int32), _p(off, C.c_int32), _p(idx, C.c_int32), nm, _p(b, C.c_double))
    k = int(lib.hu_newick_from_arrays(*head, None, C.c_int64(0)))
    if k < 0:
        _chk(k)
    buf = C.create_string_buffer(k + 1)
    lib.hu_newick_from_arrays(*head, buf, C.c_int64(k + 1))
    return buf.value.decode()


class SupportOpts(C.Structure):
    _fields_ = [("blen", BlenOpts), ("replicates", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


SUPPORT_TIE = 2.0 ** -40
SUPPORT_LDS_COLS = 4736


def support_weights(cs_len: int, replicates: int, seed: int = 1, device=None) -> np.ndarray:
    """hu_support_weights: w [replicates][cs_len] uint16, how often replicate b drew column j.  device: the table of the device's kernel
    (hu_support_weights_device) instead of the host's"""
    lib = load_library()
    if cs_len < 1 or replicates < 1:
        raise EngineError("support_weights: at least one column and one replicate")
    w = np.zeros((int(replicates), int(cs_len)), np.uint16)
    if device is None:
        _chk(lib.hu_support_weights(C.c_int32(cs_len), C.c_int32(replicates), C.c_uint64(seed), _p(w, C.c_uint16)))
    else:
        _chk(lib.hu_support_weights_device(C.c_int32(device), C.c_int32(cs_len), C.c_int32(replicates), C.c_uint64(seed), _p(w, C.c_uint16)))
    return w


def support_need(n_nodes: int, cs_len: int, replicates: int) -> int:
    """hu_support_need: the bytes the local supports hold for n_nodes x cs_len and `replicates` replicates"""
    lib = load_library()
    lib.hu_support_need.restype = C.c_int64
    return int(lib.hu_support_need(C.c_int32(n_nodes), C.c_int32(cs_len), C.c_int32(replicates)))


def tree_nni_support(parent, blen, seq, model: ModelDesc, replicates=None, seed=None, min_len=None, max_len=None, device=0, host=False,
                     mem_budget=0, with_sums=False) -> dict:
    """hu_tree_nni_support: for the E eligible edges in ascending u, dict(edge_node [E], t_star [E][3], f [E][3], alrt [E] =
    2 (f^0 - max(f^1, f^2)), count [E] the replicates that support the edge, support [E] = count / replicates, replicates, skipped,
    seconds) and, with_sums, sums [E][B][2] = (S^1_b, S^2_b)"""
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64); seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError("tree_nni_support: parent [n], blen [n] and seq [n][cs_len]")
    lib = load_library()
    o = SupportOpts()
    lib.hu_support_default_opts(C.byref(o))
    if replicates is not None:
        o.replicates = int(replicates)
    if seed is not None:
        o.seed = int(seed)
    if min_len is not None:
        o.blen.min_len = float(min_len)
    if max_len is not None:
        o.blen.max_len = float(max_len)
    o.blen.host = 1 if host else 0; o.blen.device = int(device); o.blen.mem_budget = int(mem_budget or 0)
    n, L = seq.shape
    B = int(o.replicates)
    cap = max((n - 1) // 2, 1)
    node = np.zeros(cap, np.int32); ts = np.zeros((cap, 3)); f = np.zeros((cap, 3)); cnt = np.zeros(cap, np.int32)
    sums = np.zeros((cap, B, 2)) if with_sums and 1 <= B <= 100000 else None
    ne = C.c_int32(0); sk = C.c_int64(0)
    _chk(lib.hu_tree_nni_support(C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                 C.byref(model), C.c_int32(cap), C.byref(ne), C.byref(sk), _p(node, C.c_int32), _p(ts, C.c_double),
                                 _p(f, C.c_double), _p(cnt, C.c_int32), _p(sums, C.c_double) if sums is not None else None))
    e = ne.value
    s = np.zeros(4)
    _chk(lib.hu_support_timing(_p(s, C.c_double)))
    out = dict(edge_node=node[:e].copy(), t_star=ts[:e].copy(), f=f[:e].copy(), alrt=2.0 * (f[:e, 0] - np.maximum(f[:e, 1], f[:e, 2])),
               count=cnt[:e].copy(), support=cnt[:e] / float(B) if B > 0 else np.zeros(e), replicates=B, skipped=int(sk.value),
               seconds=dict(sweep=s[0], score=s[1], weights=s[2], support=s[3]))
    if sums is not None:
        out["sums"] = sums[:e].copy()
    return out


class SprRound(C.Structure):
    _fields_ = [("ll", C.c_double), ("targets", C.c_int64), ("pruned", C.c_int32), ("candidates", C.c_int32), ("taken", C.c_int32),
                ("applied", C.c_int32)]


class SprOpts(C.Structure):
    _fields_ = [("blen", BlenOpts), ("min_gain", C.c_double), ("radius", C.c_int32), ("spr_rounds", C.c_int32), ("rounds_cap", C.c_int32),
                ("slab", C.c_int32), ("rounds", C.POINTER(SprRound)), ("moves", C.POINTER(C.c_int32)), ("moves_cap", C.c_int64),
                ("n_rounds", C.c_int32), ("stop", C.c_int32), ("n_moves", C.c_int64), ("skipped", C.c_int64),
                ("ll_start", C.c_double), ("ll_final", C.c_double)]


SPR_MAX_RADIUS = 32
SPR_STOP = ("local optimum", "no improving move", "max rounds")


def _spr_args(what, parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget, radius, slab, spr_rounds=None, min_gain=None):
    parent = np.ascontiguousarray(parent, np.int32).copy(); blen = np.ascontiguousarray(blen, np.float64).copy()
    seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError(what + ": parent [n], blen [n] and seq [n][cs_len]")
    o = SprOpts()
    load_library().hu_spr_default_opts(C.byref(o))
    for k, v in (("eps", eps), ("min_len", min_len), ("max_len", max_len)):
        if v is not None:
            setattr(o.blen, k, float(v))
    if max_rounds is not None:
        o.blen.max_rounds = int(max_rounds)
    for k, v in (("radius", radius), ("slab", slab), ("spr_rounds", spr_rounds)):
        if v is not None:
            setattr(o, k, int(v))
    if min_gain is not None:
        o.min_gain = float(min_gain)
    o.blen.host = 1 if host else 0; o.blen.device = int(device); o.blen.mem_budget = int(mem_budget or 0)
    return o, parent, blen, seq


def spr_need(n_nodes: int, cs_len: int, radius: int = 5) -> int:
    """hu_spr_need: the bytes the SPR search holds for n_nodes x cs_len at this radius"""
    lib = load_library()
    lib.hu_spr_need.restype = C.c_int64
    return int(lib.hu_spr_need(C.c_int32(n_nodes), C.c_int32(cs_len), C.c_int32(radius)))


def tree_spr_scores(parent, blen, seq, model: ModelDesc, radius=None, min_len=None, max_len=None, device=0, host=False, mem_budget=0,
                    slab=None) -> dict:
    """hu_tree_spr_scores: for the P prunable nodes in ascending v, dict(prune_node [P], v_off [P + 1], base_t [P], base_f [P] (the
    baseline with the pendant at its optimum), f_at_blen [P] (the baseline as the tree stands: the tree's log-likelihood), and per
    target in the order of the walk target_node, dist, t_star, f; skipped)"""
    o, parent, blen, seq = _spr_args("tree_spr_scores", parent, blen, seq, model, None, min_len, max_len, None, device, host, mem_budget, radius, slab)
    n, L = seq.shape
    lib = load_library()
    npr = C.c_int32(0); nt = C.c_int64(0); sk = C.c_int64(0)
    head = (C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8), C.byref(model))
    _chk(lib.hu_tree_spr_scores(*head, C.c_int32(0), C.c_int64(0), C.byref(npr), C.byref(nt), C.byref(sk), *([None] * 9)))
    P, T = max(npr.value, 1), max(nt.value, 1)
    node = np.zeros(P, np.int32); off = np.zeros(P + 1, np.int64); bt = np.zeros(P); bf = np.zeros(P); f0 = np.zeros(P)
    w = np.zeros(T, np.int32); d = np.zeros(T, np.int32); ts = np.zeros(T); f = np.zeros(T)
    _chk(lib.hu_tree_spr_scores(*head, C.c_int32(P), C.c_int64(T), C.byref(npr), C.byref(nt), C.byref(sk), _p(node, C.c_int32), _p(off, C.c_int64),
                                _p(bt, C.c_double), _p(bf, C.c_double), _p(f0, C.c_double), _p(w, C.c_int32), _p(d, C.c_int32), _p(ts, C.c_double),
                                _p(f, C.c_double)))
    P, T = npr.value, nt.value
    return dict(prune_node=node[:P].copy(), v_off=off[:P + 1].copy(), base_t=bt[:P].copy(), base_f=bf[:P].copy(), f_at_blen=f0[:P].copy(),
                target_node=w[:T].copy(), dist=d[:T].copy(), t_star=ts[:T].copy(), f=f[:T].copy(), skipped=int(sk.value))


def tree_spr_apply(parent, blen, v: int, w: int, t: float, child_off=None, child_idx=None) -> dict:
    """hu_tree_spr_apply: the subtree of v pruned and regrafted into the edge above w, that edge split in halves, the pendant set to t.
    dict(parent, blen, child_off, child_idx), the inputs are not changed"""
    parent = np.ascontiguousarray(parent, np.int32).copy(); blen = np.ascontiguousarray(blen, np.float64).copy()
    off, idx = _child_arrays(parent, child_off, child_idx)
    _chk(load_library().hu_tree_spr_apply(C.c_int32(len(parent)), _p(parent, C.c_int32), _p(blen, C.c_double), _p(off, C.c_int32), _p(idx, C.c_int32),
                                          C.c_int32(int(v)), C.c_int32(int(w)), C.c_double(float(t))))
    return dict(parent=parent, blen=blen, child_off=off, child_idx=idx)


def tree_spr_search(parent, blen, seq, model: ModelDesc, child_off=None, child_idx=None, radius=None, spr_rounds=None, min_gain=None, eps=None,
                    min_len=None, max_len=None, max_rounds=None, device=0, host=False, mem_budget=0, slab=None) -> dict:
    """hu_tree_spr_search: the hill climb over SPR moves.  dict(parent, blen, child_off, child_idx, ll_start, ll_final, stop (one of
    SPR_STOP), skipped, rounds: per accepted round (ll, pruned, targets, candidates, taken, applied), moves: per applied move (round, v,
    w_from, w_to, dist), seconds)"""
    o, parent, blen, seq = _spr_args("tree_spr_search", parent, blen, seq, model, eps, min_len, max_len, max_rounds, device, host, mem_budget,
                                     radius, slab, spr_rounds, min_gain)
    n, L = seq.shape
    off, idx = _child_arrays(parent, child_off, child_idx)
    cap = max(int(o.spr_rounds), 1)
    rec = (SprRound * cap)()
    mcap = cap * max(n, 1)
    mv = np.zeros((mcap, 5), np.int32)
    o.rounds = C.cast(rec, C.POINTER(SprRound)); o.rounds_cap = cap; o.moves = _p(mv, C.c_int32); o.moves_cap = mcap
    _chk(load_library().hu_tree_spr_search(C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                           _p(off, C.c_int32), _p(idx, C.c_int32), C.byref(model)))
    s = np.zeros(4)
    _chk(load_library().hu_spr_timing(_p(s, C.c_double)))
    return dict(parent=parent, blen=blen, child_off=off, child_idx=idx, ll_start=float(o.ll_start), ll_final=float(o.ll_final), stop=SPR_STOP[o.stop],
                skipped=int(o.skipped),
                rounds=[dict(ll=r.ll, pruned=r.pruned, targets=int(r.targets), candidates=r.candidates, taken=r.taken, applied=r.applied)
                        for r in rec[:o.n_rounds]],
                moves=[tuple(int(x) for x in row) for row in mv[:o.n_moves]], seconds=dict(fit=s[0], score=s[1], trial=s[2], other=s[3]))


class AddRound(C.Structure):
    _fields_ = [("ll", C.c_double), ("scored", C.c_int32), ("inserted", C.c_int32)]


class AddInsert(C.Structure):
    _fields_ = [("round", C.c_int32), ("query", C.c_int32), ("v", C.c_int32), ("w", C.c_int32), ("t", C.c_double), ("f", C.c_double)]


class AddOpts(C.Structure):
    _fields_ = [("blen", BlenOpts), ("slab", C.c_int32), ("tile", C.c_int32), ("rounds_cap", C.c_int32), ("reserved", C.c_int32),
                ("rounds", C.POINTER(AddRound)), ("inserts", C.POINTER(AddInsert)), ("inserts_cap", C.c_int64),
                ("n_rounds", C.c_int32), ("n_inserted", C.c_int32), ("ll_start", C.c_double), ("ll_final", C.c_double)]


ADD_TILE = 16


def _add_args(what, parent, blen, seq, queries, eps, min_len, max_len, max_rounds, device, host, mem_budget, slab, tile):
    parent = np.ascontiguousarray(parent, np.int32).copy(); blen = np.ascontiguousarray(blen, np.float64).copy()
    seq = np.ascontiguousarray(seq, np.int8)
    if seq.ndim != 2 or parent.shape != (seq.shape[0],) or blen.shape != parent.shape:
        raise EngineError(what + ": parent [n], blen [n] and seq [n][cs_len]")
    queries = np.ascontiguousarray(queries, np.int8).reshape(-1, seq.shape[1]) if len(queries) else np.zeros((0, seq.shape[1]), np.int8)
    o = AddOpts()
    load_library().hu_add_default_opts(C.byref(o))
    for k, v in (("eps", eps), ("min_len", min_len), ("max_len", max_len)):
        if v is not None:
            setattr(o.blen, k, float(v))
    if max_rounds is not None:
        o.blen.max_rounds = int(max_rounds)
    for k, v in (("slab", slab), ("tile", tile)):
        if v is not None:
            setattr(o, k, int(v))
    o.blen.host = 1 if host else 0; o.blen.device = int(device); o.blen.mem_budget = int(mem_budget or 0)
    return o, parent, blen, seq, queries


def add_need(final_nodes: int, cs_len: int, n_query: int) -> int:
    """hu_add_need: the bytes the insertion of n_query sequences holds for a grown tree of final_nodes x cs_len"""
    lib = load_library()
    lib.hu_add_need.restype = C.c_int64
    return int(lib.hu_add_need(C.c_int32(final_nodes), C.c_int32(cs_len), C.c_int32(n_query)))


def tree_add_scores(parent, blen, seq, queries, model: ModelDesc, min_len=None, max_len=None, device=0, host=False, mem_budget=0,
                    slab=None, tile=None) -> dict:
    """hu_tree_add_scores: queries [q][cs_len] against every edge of the tree.  dict(t_star [q][n], f [q][n] (the root's entries 0 and
    -inf), best_w [q], best_t [q], best_f [q]: the best edge of every query, the largest f and the smaller w among equals)"""
    o, parent, blen, seq, qs = _add_args("tree_add_scores", parent, blen, seq, queries, None, min_len, max_len, None, device, host, mem_budget, slab, tile)
    n, L = seq.shape
    q = len(qs)
    ts = np.zeros((q, n)); f = np.zeros((q, n)); bw = np.zeros(max(q, 1), np.int32); bt = np.zeros(max(q, 1)); bf = np.zeros(max(q, 1))
    _chk(load_library().hu_tree_add_scores(C.byref(o), C.c_int32(n), C.c_int32(L), _p(parent, C.c_int32), _p(blen, C.c_double), _p(seq, C.c_int8),
                                           C.byref(model), C.c_int32(q), _p(qs, C.c_int8) if q else None, _p(ts, C.c_double) if q else None,
                                           _p(f, C.c_double) if q else None, _p(bw, C.c_int32), _p(bt, C.c_double), _p(bf, C.c_double)))
    return dict(t_star=ts, f=f, best_w=bw[:q].copy(), best_t=bt[:q].copy(), best_f=bf[:q].copy())


def tree_add_apply(parent, blen, w: int, t: float, child_off=None, child_idx=None, min_len=0.0, max_len=10.0) -> dict:
    """hu_tree_add_apply: a new leaf hung into the middle of the edge above w with the pendant t: the nodes p = n and v = n + 1 are
    appended.  dict(parent [n + 2], blen [n + 2], child_off [n + 3], child_idx [n + 1]), the inputs are not changed"""
    n = len(parent)
    off, idx = _child_arrays(np.ascontiguousarray(parent, np.int32), child_off, child_idx)
    par = np.full(n + 2, -1, np.int32); par[:n] = parent
    bl = np.zeros(n + 2); bl[:n] = blen
    off2 = np.zeros(n + 3, np.int32); off2[:n + 1] = off[:n + 1]
    idx2 = np.zeros(n + 1, np.int32); idx2[:max(n - 1, 0)] = idx[:max(n - 1, 0)]
    _chk(load_library().hu_tree_add_apply(C.c_int32(n), _p(par, C.c_int32), _p(bl, C.c_double), _p(off2, C.c_int32), _p(idx2, C.c_int32),
                                          C.c_int32(int(w)), C.c_double(float(t)), C.c_double(float(min_len)), C.c_double(float(max_len))))
    return dict(parent=par, blen=bl, child_off=off2, child_idx=idx2)


def tree_add_search(parent, blen, seq, queries, model: ModelDesc, child_off=None, child_idx=None, eps=None, min_len=None, max_len=None,
                    max_rounds=None, device=0, host=False, mem_budget=0, slab=None, tile=None) -> dict:
    """hu_tree_add_search: every query inserted into the tree, round by round.  dict(parent, blen, seq, child_off, child_idx of the
    grown tree of n + 2 q nodes, query_node [q] the leaf of every query, ll_start, ll_final, rounds: per round (ll, scored, inserted),
    inserts: per insertion (round, query, v, w, t, f), seconds)"""
    o, parent, blen, seq, qs = _add_args("tree_add_search", parent, blen, seq, queries, eps, min_len, max_len, max_rounds, device, host, mem_budget,
                                         slab, tile)
    n, L = seq.shape
    q = len(qs); N = n + 2 * q
    off, idx = _child_arrays(parent, child_off, child_idx)
    par = np.full(N, -1, np.int32); par[:n] = parent
    bl = np.zeros(N); bl[:n] = blen
    sq = np.full((N, L), -2, np.int8); sq[:n] = seq
    off2 = np.zeros(N + 1, np.int32); off2[:n + 1] = off[:n + 1]
    idx2 = np.zeros(max(N - 1, 1), np.int32); idx2[:max(n - 1, 0)] = idx[:max(n - 1, 0)]
    qn = np.full(max(q, 1), -1, np.int32)
    cap = max(q, 1)
    rec = (AddRound * cap)(); ins = (AddInsert * cap)()
    o.rounds = C.cast(rec, C.POINTER(AddRound)); o.rounds_cap = cap; o.inserts = C.cast(ins, C.POINTER(AddInsert)); o.inserts_cap = cap
    _chk(load_library().hu_tree_add_search(C.byref(o), C.c_int32(n), C.c_int32(L), C.c_int32(q), _p(par, C.c_int32), _p(bl, C.c_double), _p(sq, C.c_int8),
                                           _p(off2, C.c_int32), _p(idx2, C.c_int32), _p(qs, C.c_int8) if q else None, _p(qn, C.c_int32), C.byref(model)))
    s = np.zeros(4)
    _chk(load_library().hu_add_timing(_p(s, C.c_double)))
    return dict(parent=par, blen=bl, seq=sq, child_off=off2, child_idx=idx2, query_node=qn[:q].copy(), ll_start=float(o.ll_start),
                ll_final=float(o.ll_final), rounds=[dict(ll=r.ll, scored=r.scored, inserted=r.inserted) for r in rec[:o.n_rounds]],
                inserts=[dict(round=i.round, query=i.query, v=i.v, w=i.w, t=i.t, f=i.f) for i in ins[:o.n_inserted]],
                seconds=dict(sweep=s[0], score=s[1], fit=s[2], other=s[3]))


def tree_count_mutations(parent, cs_len: int, up_ptr: int, device=0) -> np.ndarray:
    """hu_tree_count_mutations: per column, the non-root nodes whose inferred state differs from their parent's, from the DEVICE
    fixed-rate up buffer at up_ptr ([n][cs_len][4] float64, as tree_evaluate leaves it with win_len 0)"""
    parent = np.ascontiguousarray(parent, np.int32)
    cnt = np.zeros(cs_len, np.int32)
    _chk(load_library().hu_tree_count_mutations(C.c_int(device), C.c_int32(len(parent)), C.c_int32(cs_len), _p(parent, C.c_int32),
                                                C.c_void_p(int(up_ptr)), _p(cnt, C.c_int32)))
    return cnt


def dg_model(K: int, alpha: float):
    """hu_dg_model: the discrete-Gamma breaks [K + 1] and rates [K] of DiscreteGammaModel(K, alpha)"""
    b = np.zeros(K + 1); r = np.zeros(K)
    _chk(load_library().hu_dg_model(C.c_int32(K), C.c_double(alpha), _p(b, C.c_double), _p(r, C.c_double)))
    return b, r


def dg_estimate_shape(x) -> float:
    """hu_dg_estimate_shape: the moment estimate of the Gamma shape from per-site mutation counts (+inf below 2 sites)"""
    lib = load_library()
    lib.hu_dg_estimate_shape.restype = C.c_double
    x = np.ascontiguousarray(x, np.float64)
    return float(lib.hu_dg_estimate_shape(C.c_int64(len(x)), _p(x, C.c_double)))


def write_ptu(path, parent, blen, seq, up, down, height, model: ModelDesc, names=None, annos=None, anno_dist=None, model_text=None,
              dg_alpha=0.0, dg_breaks=None, msgs_on_device=False):
    """hu_ptu_write: the database file in the reference's .ptu format; up / down are [n][cs_len][4] arrays, or device pointers (ints)
    with msgs_on_device=True."""
    keep = dict(parent=np.ascontiguousarray(parent, np.int32), blen=np.ascontiguousarray(blen, np.float64), seq=np.ascontiguousarray(seq, np.int8),
                height=np.ascontiguousarray(height, np.float64))
    td = TreeDesc()
    td.n_nodes, td.cs_len = keep["seq"].shape
    td.parent = _p(keep["parent"], C.c_int32); td.blen = _p(keep["blen"], C.c_double); td.seq = _p(keep["seq"], C.c_int8); td.height = _p(keep["height"], C.c_double)
    if msgs_on_device:
        td.up = C.c_void_p(int(up)); td.down = C.c_void_p(int(down)); td.msgs_on_device = 1
    else:
        keep["up"] = np.ascontiguousarray(up, np.float64); keep["down"] = np.ascontiguousarray(down, np.float64)
        td.up = keep["up"].ctypes.data_as(C.c_void_p); td.down = keep["down"].ctypes.data_as(C.c_void_p)
    if anno_dist is not None:
        keep["ad"] = np.ascontiguousarray(anno_dist, np.float64); td.anno_dist = _p(keep["ad"], C.c_double)
    arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs]) if xs is not None else None
    br = np.ascontiguousarray(dg_breaks, np.float64) if dg_breaks is not None else None
    _chk(load_library().hu_ptu_write(path.encode(), C.byref(td), arr(names), arr(annos), C.byref(model), model_text.encode() if model_text else None,
                                     C.c_double(dg_alpha), _p(br, C.c_double) if br is not None else None))


def write_ptu_stream(path, parent, blen, seq, up, down, height, model: ModelDesc, names=None, annos=None, anno_dist=None, model_text=None,
                     dg_alpha=0.0, dg_breaks=None, msgs_on_device=False, child_off=None, child_idx=None, msa_row_of_leaf=None, staging_bytes=0):
    """hu_ptu_write_stream: write_ptu with a chosen child order (CSR child_off [n + 1], child_idx [n - 1]), the MSA index as (row, node)
    pairs (msa_row_of_leaf [n], -1 for inner nodes), and device messages packed by k_ptu_gather through two staging buffers of
    staging_bytes each (0: 256 MB)."""
    keep = dict(parent=np.ascontiguousarray(parent, np.int32), blen=np.ascontiguousarray(blen, np.float64), seq=np.ascontiguousarray(seq, np.int8),
                height=np.ascontiguousarray(height, np.float64))
    td = TreeDesc()
    td.n_nodes, td.cs_len = keep["seq"].shape
    td.parent = _p(keep["parent"], C.c_int32); td.blen = _p(keep["blen"], C.c_double); td.seq = _p(keep["seq"], C.c_int8); td.height = _p(keep["height"], C.c_double)
    if msgs_on_device:
        td.up = C.c_void_p(int(up)); td.down = C.c_void_p(int(down)); td.msgs_on_device = 1
    else:
        keep["up"] = np.ascontiguousarray(up, np.float64); keep["down"] = np.ascontiguousarray(down, np.float64)
        td.up = keep["up"].ctypes.data_as(C.c_void_p); td.down = keep["down"].ctypes.data_as(C.c_void_p)
    if anno_dist is not None:
        keep["ad"] = np.ascontiguousarray(anno_dist, np.float64); td.anno_dist = _p(keep["ad"], C.c_double)
    arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs]) if xs is not None else None
    i32 = lambda a: np.ascontiguousarray(a, np.int32) if a is not None else None
    br = np.ascontiguousarray(dg_breaks, np.float64) if dg_breaks is not None else None
    co, ci, ro = i32(child_off), i32(child_idx), i32(msa_row_of_leaf)
    _chk(load_library().hu_ptu_write_stream(path.encode(), C.byref(td), arr(names), arr(annos), C.byref(model), model_text.encode() if model_text else None,
                                            C.c_double(dg_alpha), _p(br, C.c_double) if br is not None else None,
                                            _p(co, C.c_int32) if co is not None else None, _p(ci, C.c_int32) if ci is not None else None,
                                            _p(ro, C.c_int32) if ro is not None else None, C.c_int64(int(staging_bytes))))


class TreeSweep:
    """hu_tree_sweep_*: tree_evaluate held across column windows.  The tree's arrays go to the device once; window() moves the
    [n][win_len] bytes of its columns and fills the DEVICE buffers at up_ptr / down_ptr ([n][win_len][4] float64).  seq: the int8
    array [n][cs_len] with the leaf rows, whose inner rows window() fills in place.  down_ptr None: the post-order levels only."""

    def __init__(self, parent, blen, cs_len: int, device=0):
        self.parent = np.ascontiguousarray(parent, np.int32); self.blen = np.ascontiguousarray(blen, np.float64)
        self.n, self.cs_len = len(self.parent), int(cs_len)
        self.h = C.c_void_p()
        _chk(load_library().hu_tree_sweep_create(C.c_int32(self.n), C.c_int32(self.cs_len), _p(self.parent, C.c_int32), _p(self.blen, C.c_double),
                                                 C.c_int(device), C.byref(self.h)))

    def window(self, seq, model: ModelDesc, win_start: int, win_len: int, up_ptr: int, down_ptr=None):
        if seq.dtype != np.int8 or not seq.flags.c_contiguous or seq.shape != (self.n, self.cs_len):
            raise ValueError("seq must be a contiguous int8 array [n][cs_len]")
        _chk(load_library().hu_tree_sweep_window(self.h, C.byref(model), _p(seq, C.c_int8), C.c_int64(win_start), C.c_int64(win_len),
                                                 C.c_void_p(int(up_ptr)), C.c_void_p(int(down_ptr)) if down_ptr is not None else None))

    def heights(self) -> np.ndarray:
        h = np.zeros(self.n)
        _chk(load_library().hu_tree_sweep_heights(self.h, _p(h, C.c_double)))
        return h

    def close(self):
        if self.h:
            lib = load_library()
            lib.hu_tree_sweep_destroy.restype = None
            lib.hu_tree_sweep_destroy(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PtuWriter:
    """hu_ptu_writer_*: write_ptu_stream fed a column window at a time, in any order; the file is byte for byte write_ptu_stream's.
    window(): up / down are [n][win_len][4] arrays, or device pointers (ints) with on_device=True.  close() takes the rows and heights,
    refuses unless the windows tiled [0, cs_len) exactly once, and ends the writer; a refusal, a failed write and abort() leave no file."""

    def __init__(self, path, parent, blen, cs_len: int, names=None, annos=None, anno_dist=None, child_off=None, child_idx=None, msa_row_of_leaf=None,
                 staging_bytes=0):
        keep = dict(parent=np.ascontiguousarray(parent, np.int32), blen=np.ascontiguousarray(blen, np.float64))
        td = TreeDesc()
        td.n_nodes, td.cs_len = len(keep["parent"]), int(cs_len)
        td.parent = _p(keep["parent"], C.c_int32); td.blen = _p(keep["blen"], C.c_double)
        if anno_dist is not None:
            keep["ad"] = np.ascontiguousarray(anno_dist, np.float64); td.anno_dist = _p(keep["ad"], C.c_double)
        arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs]) if xs is not None else None
        i32 = lambda a: np.ascontiguousarray(a, np.int32) if a is not None else None
        co, ci, ro = i32(child_off), i32(child_idx), i32(msa_row_of_leaf)
        self.n, self.cs_len = td.n_nodes, td.cs_len
        self.h = C.c_void_p()
        _chk(load_library().hu_ptu_writer_open(path.encode(), C.byref(td), arr(names), arr(annos), _p(co, C.c_int32) if co is not None else None,
                                               _p(ci, C.c_int32) if ci is not None else None, _p(ro, C.c_int32) if ro is not None else None,
                                               C.c_int64(int(staging_bytes)), C.byref(self.h)))

    def window(self, win_start: int, win_len: int, up, down, on_device=False):
        if on_device:
            u, d = C.c_void_p(int(up)), C.c_void_p(int(down))
            keep = None
        else:
            keep = (np.ascontiguousarray(up, np.float64), np.ascontiguousarray(down, np.float64))
            if keep[0].shape != (self.n, win_len, 4) or keep[1].shape != (self.n, win_len, 4):
                raise ValueError("up / down must be [n][win_len][4]")
            u, d = keep[0].ctypes.data_as(C.c_void_p), keep[1].ctypes.data_as(C.c_void_p)
        _chk(load_library().hu_ptu_writer_window(self.h, C.c_int64(win_start), C.c_int64(win_len), u, d, C.c_int(1 if on_device else 0)))

    def close(self, seq, height, model: ModelDesc, model_text=None, dg_alpha=0.0, dg_breaks=None):
        seq = np.ascontiguousarray(seq, np.int8); height = np.ascontiguousarray(height, np.float64)
        if seq.shape != (self.n, self.cs_len) or height.shape != (self.n,):
            raise ValueError("seq must be [n][cs_len], height [n]")
        br = np.ascontiguousarray(dg_breaks, np.float64) if dg_breaks is not None else None
        h, self.h = self.h, C.c_void_p()                  # the handle ends here whatever happens
        _chk(load_library().hu_ptu_writer_close(h, _p(seq, C.c_int8), _p(height, C.c_double), C.byref(model), model_text.encode() if model_text else None,
                                                C.c_double(dg_alpha), _p(br, C.c_double) if br is not None else None))

    def abort(self):
        if self.h:
            lib = load_library()
            lib.hu_ptu_writer_abort.restype = None
            lib.hu_ptu_writer_abort(self.h); self.h = C.c_void_p()

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


def build_window_need(n_nodes: int, win_len: int, with_var: bool) -> int:
    """hu_build_window_need: the device bytes of a windowed build at window width win_len"""
    lib = load_library()
    lib.hu_build_window_need.restype = C.c_int64
    return int(lib.hu_build_window_need(C.c_int32(n_nodes), C.c_int32(win_len), C.c_int(int(bool(with_var)))))


def build_window_plan(n_nodes: int, cs_len: int, with_var: bool, budget_bytes: int):
    """hu_build_window_plan: (window width, bytes needed at it) of the widest windowed build within budget_bytes; EngineError -4 when
    not even one column fits"""
    W = C.c_int32(0); need = C.c_int64(0)
    _chk(load_library().hu_build_window_plan(C.c_int32(n_nodes), C.c_int32(cs_len), C.c_int(int(bool(with_var))), C.c_int64(int(budget_bytes)),
                                             C.byref(W), C.byref(need)))
    return int(W.value), int(need.value)


def tree_info(ptu_path: str) -> dict:
    """hu_tree_info_*: the tree of a .ptu without its messages (host only): parent, blen, anno_dist, is_leaf, names, annos, and every
    node's children in the order their parent -> child edges stand in the file"""
    lib = load_library()
    h = C.c_void_p()
    _chk(lib.hu_tree_info_load(ptu_path.encode(), C.byref(h)))
    try:
        n = C.c_int32(0); L = C.c_int32(0); root = C.c_int32(0); md = ModelDesc()
        _chk(lib.hu_tree_info_get(h, C.byref(n), C.byref(L), C.byref(root), C.byref(md)))
        n = n.value
        out = dict(n_nodes=n, cs_len=L.value, root=root.value, model=md, parent=np.zeros(n, np.int32), blen=np.zeros(n), anno_dist=np.zeros(n),
                   is_leaf=np.zeros(n, bool), names=[], annos=[], children=[])
        for i in range(n):
            p = C.c_int32(0); b = C.c_double(0); d = C.c_double(0); lf = C.c_int32(0); nm = C.c_char_p(); an = C.c_char_p()
            _chk(lib.hu_tree_info_node(h, C.c_int32(i), C.byref(p), C.byref(b), C.byref(d), C.byref(lf), C.byref(nm), C.byref(an)))
            out["parent"][i] = p.value; out["blen"][i] = b.value; out["anno_dist"][i] = d.value; out["is_leaf"][i] = bool(lf.value)
            out["names"].append(nm.value.decode()); out["annos"].append(an.value.decode())
            ch = C.POINTER(C.c_int32)()
            k = int(lib.hu_tree_info_children(h, C.c_int32(i), C.byref(ch)))
            out["children"].append([int(ch[j]) for j in range(k)])
        return out
    finally:
        lib.hu_tree_info_free(h)


def newick_parse(text) -> dict:
    """hu_newick_parse: parent, blen, names with the reference's node ids, and every node's children in file order (children: list of
    arrays; child_off / child_idx: the same as a CSR).  Raises EngineError with the byte offset on malformed text."""
    lib = load_library()
    lib.hu_newick_name.restype = C.c_char_p
    b = text.encode() if isinstance(text, str) else bytes(text)
    h = C.c_void_p()
    _chk(lib.hu_newick_parse(b, C.c_int64(len(b)), C.byref(h)))
    try:
        n = C.c_int32(0)
        _chk(lib.hu_newick_size(h, C.byref(n)))
        n = n.value
        out = dict(parent=np.zeros(n, np.int32), blen=np.zeros(n), child_off=np.zeros(n + 1, np.int32), child_idx=np.zeros(max(n - 1, 0), np.int32))
        _chk(lib.hu_newick_get(h, _p(out["parent"], C.c_int32), _p(out["blen"], C.c_double), _p(out["child_off"], C.c_int32),
                               _p(out["child_idx"], C.c_int32) if n > 1 else None))
        out["names"] = [lib.hu_newick_name(h, C.c_int32(i)).decode() for i in range(n)]
        out["children"] = [out["child_idx"][out["child_off"][i]:out["child_off"][i + 1]] for i in range(n)]
        return out
    finally:
        lib.hu_newick_free(h)


def tree_annotate(parent, blen, names, anno_text=None, root_name=None):
    """hu_tree_annotate: loadAnnotation (anno_text: the "name<TAB>annotation" lines, or None), formatName and annotate of the build.
    Returns (names, annotations, anno_dist)."""
    lib = load_library()
    lib.hu_tree_anno_name.restype = C.c_char_p; lib.hu_tree_anno_anno.restype = C.c_char_p
    parent = np.ascontiguousarray(parent, np.int32); blen = np.ascontiguousarray(blen, np.float64)
    n = len(parent)
    nm = (C.c_char_p * n)(*[x.encode() for x in names])
    at = (anno_text.encode() if isinstance(anno_text, str) else bytes(anno_text)) if anno_text is not None else None
    h = C.c_void_p()
    _chk(lib.hu_tree_annotate(C.c_int32(n), _p(parent, C.c_int32), _p(blen, C.c_double), nm, at, C.c_int64(len(at) if at is not None else 0),
                              root_name.encode() if root_name is not None else None, C.byref(h)))
    try:
        d = np.zeros(n)
        _chk(lib.hu_tree_anno_dist(h, _p(d, C.c_double)))
        return ([lib.hu_tree_anno_name(h, C.c_int32(i)).decode() for i in range(n)],
                [lib.hu_tree_anno_anno(h, C.c_int32(i)).decode() for i in range(n)], d)
    finally:
        lib.hu_tree_anno_free(h)


def tree_loglik(n_nodes: int, cs_len: int, root: int, model: ModelDesc, up_ptr: int, device=0):
    """hu_tree_loglik: (per-column log-likelihoods [cs_len], their serial sum) of the root message at up_ptr[root] (DEVICE buffer
    [n_nodes][cs_len][4] as tree_evaluate leaves it)"""
    per = np.zeros(cs_len); s = C.c_double(0)
    _chk(load_library().hu_tree_loglik(C.c_int(device), C.c_int32(n_nodes), C.c_int32(cs_len), C.c_int32(root), C.byref(model),
                                       C.c_void_p(int(up_ptr)), _p(per, C.c_double), C.byref(s)))
    return per, float(s.value)


class SeedIndex:
    """Host k-mer index standing in for the CSFM lookup of alignSeq (hu_seed_index_*)."""

    def __init__(self, parent, seq, hmm, seed_len=20, csfm=None):
        """from the leaf rows of a tree (parent, seq), or — csfm=<path> — from the reference's own <DB>.csfm (hu_seed_index_load_csfm)"""
        self.p2cs = np.ascontiguousarray(hmm.p2cs, np.int32)
        self.h = C.c_void_p()
        if csfm is not None:
            _chk(load_library().hu_seed_index_load_csfm(str(csfm).encode(), C.c_int32(int(hmm.K)), _p(self.p2cs, C.c_int32), C.c_int32(seed_len), C.byref(self.h)))
        else:
            self.parent = np.ascontiguousarray(parent, np.int32); self.seq = np.ascontiguousarray(seq, np.int8)
            n, L = self.seq.shape
            _chk(load_library().hu_seed_index_create(C.c_int32(n), C.c_int32(L), _p(self.parent, C.c_int32), _p(self.seq, C.c_int8),
                                                     C.c_int32(int(hmm.K)), _p(self.p2cs, C.c_int32), C.c_int32(seed_len), C.byref(self.h)))
        lib = load_library(); lib.hu_seed_index_size.restype = C.c_int64; lib.hu_seed_index_bytes.restype = C.c_int64
        lib.hu_seed_index_occurrences.restype = C.c_int64
        self.size = int(lib.hu_seed_index_size(self.h))
        npos = C.c_int64(0)
        self.bytes = int(lib.hu_seed_index_bytes(self.h, C.byref(npos)))
        self.positions = int(npos.value)

    def occurrences(self, kmer: str, cap=4096):
        """all occurrences of one seed in index order: (sequence number, offset in it, first CS column)"""
        a = np.zeros(cap, np.int32); b = np.zeros(cap, np.int32); c = np.zeros(cap, np.int32)
        n = int(load_library().hu_seed_index_occurrences(self.h, kmer.encode(), _p(a, C.c_int32), _p(b, C.c_int32), _p(c, C.c_int32), C.c_int64(cap)))
        m = min(n, cap)
        return n, a[:m], b[:m], c[:m]

    def locate_first(self, kmer: str):
        """CSFMIndex::locateFirst + count: (csStart, csEnd) 1-based of the first hit (0, 0 = none), number of hits"""
        a = C.c_int32(0); b = C.c_int32(0); n = C.c_int64(0)
        load_library().hu_seed_index_locate_first(self.h, kmer.encode(), C.byref(a), C.byref(b), C.byref(n))
        return int(a.value), int(b.value), int(n.value)

    def lookup(self, reads, seed_region=50, align_mode=0):
        n = len(reads)
        cat = "".join(reads).encode("latin1")
        offs = np.zeros(n + 1, np.int64); offs[1:] = np.cumsum([len(r) for r in reads])
        vp = np.zeros((n, 2, 6), np.int32)
        _chk(load_library().hu_seed_index_lookup(self.h, C.c_int(n), cat, _p(offs, C.c_int64), C.c_int(seed_region), C.c_int(align_mode),
                                                 _p(vp, C.c_int32)))
        return vp

    def lookup_random(self, reads, seed, first_read=0, seed_region=50, align_mode=0):
        """CSFMIndex::locateOne's hit choice (hu_seed_index_lookup_random): a member of each seed's hit range drawn from a hash of
        (seed, number of the read = first_read + index, seed position)"""
        n = len(reads)
        cat = "".join(reads).encode("latin1")
        offs = np.zeros(n + 1, np.int64); offs[1:] = np.cumsum([len(r) for r in reads])
        vp = np.zeros((n, 2, 6), np.int32)
        _chk(load_library().hu_seed_index_lookup_random(self.h, C.c_int(n), cat, _p(offs, C.c_int64), C.c_int(seed_region), C.c_int(align_mode),
                                                        C.c_uint64(seed), C.c_int64(first_read), _p(vp, C.c_int32)))
        return vp

    def lookup_packed(self, cat, offs, seed_region=50, align_mode=0):
        """the same on reads that are already one byte buffer + offsets [n + 1] (what a FASTA parser holds)"""
        offs = np.ascontiguousarray(offs, np.int64); n = len(offs) - 1
        vp = np.zeros((n, 2, 6), np.int32)
        _chk(load_library().hu_seed_index_lookup(self.h, C.c_int(n), cat.ctypes.data_as(C.c_char_p) if isinstance(cat, np.ndarray) else cat,
                                                 _p(offs, C.c_int64), C.c_int(seed_region), C.c_int(align_mode), _p(vp, C.c_int32)))
        return vp

    def __del__(self):
        try:
            load_library().hu_seed_index_destroy(self.h)
        except Exception:
            pass


class Database:
    """Profile + pre-evaluated tree packed once into HBM (hu_db)."""

    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep
        K = C.c_int32(); L = C.c_int32(); n = C.c_int32(); r = C.c_int32(); hb = C.c_int64()
        _chk(load_library().hu_db_info(self.h, C.byref(K), C.byref(L), C.byref(n), C.byref(r), C.byref(hb)))
        self.K, self.cs_len, self.n_nodes, self.root, self.hbm_bytes = K.value, L.value, n.value, r.value, hb.value

    @classmethod
    def from_arrays(cls, hmm, parent, blen, seq, up, down, height, model: ModelDesc, anno_id=None, anno_dist=None,
                    win_start=0, win_len=0, device=0, msgs_on_device=False):
        lib = load_library()
        keep = dict(EM=np.ascontiguousarray(hmm.EM, np.float64), EI=np.ascontiguousarray(hmm.EI, np.float64),
                    T=np.ascontiguousarray(hmm.T, np.float64), p2cs=np.ascontiguousarray(hmm.p2cs, np.int32),
                    parent=np.ascontiguousarray(parent, np.int32), blen=np.ascontiguousarray(blen, np.float64),
                    seq=np.ascontiguousarray(seq, np.int8), height=np.ascontiguousarray(height, np.float64))
        pd = ProfileDesc(int(hmm.K), int(hmm.L), _p(keep["EM"], C.c_double), _p(keep["EI"], C.c_double), _p(keep["T"], C.c_double),
                         _p(keep["p2cs"], C.c_int32))
        td = TreeDesc()
        td.n_nodes, td.cs_len = keep["seq"].shape
        td.parent = _p(keep["parent"], C.c_int32); td.blen = _p(keep["blen"], C.c_double); td.seq = _p(keep["seq"], C.c_int8)
        td.height = _p(keep["height"], C.c_double)
        if msgs_on_device:
            td.up = C.c_void_p(int(up)); td.down = C.c_void_p(int(down)); td.msgs_on_device = 1
        else:
            keep["up"] = np.ascontiguousarray(up, np.float64); keep["down"] = np.ascontiguousarray(down, np.float64)
            td.up = keep["up"].ctypes.data_as(C.c_void_p); td.down = keep["down"].ctypes.data_as(C.c_void_p)
        if anno_id is not None:
            keep["anno"] = np.ascontiguousarray(anno_id, np.int32); td.anno_id = _p(keep["anno"], C.c_int32)
        if anno_dist is not None:
            keep["annod"] = np.ascontiguousarray(anno_dist, np.float64); td.anno_dist = _p(keep["annod"], C.c_double)
        td.win_start = int(win_start); td.win_len = int(win_len)
        h = C.c_void_p()
        _chk(lib.hu_db_create(C.byref(pd), C.byref(td), C.byref(model), C.c_int(device), C.byref(h)))
        return cls(h, keep if msgs_on_device else None)

    @classmethod
    def from_synth(cls, db, device=0):
        md = model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k > 0 else None)
        return cls.from_arrays(db.hmm, db.parent, db.blen, db.seq, db.up, db.down, db.height, md, db.anno_id, db.anno_dist, device=device)

    @classmethod
    def load(cls, hmm_path: str, ptu_path: str, device=0, win_start=0, win_len=0):
        """hu_db_load / hu_db_load_window (win_len > 0: only the messages of the CS columns [win_start, win_start + win_len) stay on the device)"""
        h = C.c_void_p()
        _chk(load_library().hu_db_load_window(hmm_path.encode(), ptu_path.encode(), C.c_int(device), C.c_int64(win_start), C.c_int64(win_len), C.byref(h)))
        return cls(h)

    def model_pr(self, t):
        t = np.ascontiguousarray(t, np.float64).ravel()
        P = np.zeros((len(t), 4, 4))
        _chk(load_library().hu_db_model_pr(self.h, C.c_int(len(t)), _p(t, C.c_double), _p(P, C.c_double)))
        return P

    def build_align_path(self, cs_start, cs_end, cs: str, cs_from, cs_to):
        out = np.zeros(6, np.int32)
        _chk(load_library().hu_build_align_path(self.h, C.c_int(cs_start), C.c_int(cs_end), cs.encode(), C.c_int(cs_from), C.c_int(cs_to),
                                                _p(out, C.c_int32)))
        return out

    def profile(self):
        K = self.K
        out = dict(EM=np.zeros((K + 1, 4)), EI=np.zeros((K + 1, 4)), T=np.zeros((K + 1, 7)), p2cs=np.zeros(K + 1, np.int32),
                   entry_cost=np.zeros(K + 1), exit_cost=np.zeros(K + 1))
        _chk(load_library().hu_db_get_profile(self.h, _p(out["EM"], C.c_double), _p(out["EI"], C.c_double), _p(out["T"], C.c_double),
                                              _p(out["p2cs"], C.c_int32), _p(out["entry_cost"], C.c_double), _p(out["exit_cost"], C.c_double)))
        return out

    def num_leaves(self) -> int:
        """PTUnrooted::numLeaves: nodes with one neighbour, a root with a single child included"""
        v = C.c_int64()
        _chk(load_library().hu_db_num_leaves(self.h, C.byref(v)))
        return int(v.value)

    def anneal(self, primers, identity=0.9, strand=3, batch=4096):
        """hmmufotu-anneal (src/hmmufotu-anneal.cpp:246-290): per primer (IUPAC letters in either case, kept as given), its strand ('+', '-'),
        the CS region and alignment of the chosen strand, and the hit counts of nodes and leaves at `identity`; None for a primer with no
        alignment (a letter outside IUPAC included).  Strand choice on the host: the reverse complement (case kept letter by letter)
        replaces the forward alignment only at a strictly lower cost.  The Viterbi scores use the upper-cased bases; a matched lower-case
        base stays lower-case in the alignment, as the reference writes it."""
        max_dist = 1 - float(identity)
        if not max_dist >= 0:
            raise ValueError("-i|--identity must between 0 and 1")
        if strand not in (1, 2, 3):
            raise ValueError("-s|--strand must be 1, 2 or 3")
        opts = default_opts(align_mode="global")
        n_leaves = self.num_leaves()
        out = []
        for i0 in range(0, len(primers), batch):
            part = list(primers[i0:i0 + batch])
            n = len(part)
            seqs = (part if strand & 1 else []) + ([revcom_as_read(p) for p in part] if strand & 2 else [])
            b = Batch(self, len(seqs))
            try:
                b.set_reads([t.upper() for t in seqs], None)
                b.align(opts)
                recs = b.alignments(want_align=False)["recs"]
                chosen = np.full(n, -1, np.int32)
                strands = ["."] * n
                for i in range(n):
                    cost, rev0 = np.inf, 0
                    if strand & 1:
                        strands[i] = "+"
                        if recs[i]["status"] == 1:
                            chosen[i], cost = i, recs[i]["cost"]
                        rev0 = n
                    if strand & 2 and recs[rev0 + i]["status"] == 1 and recs[rev0 + i]["cost"] < cost:
                        chosen[i], strands[i] = rev0 + i, "-"
                hn, hl = b.anneal(chosen, max_dist, [seqs[r] if r >= 0 else None for r in chosen])
                rows = b.alignments()["align"]      # after the scan: in the case the primers were read
            finally:
                b.close()
            for i in range(n):
                r = int(chosen[i])
                if r < 0:
                    out.append(None)
                    continue
                s0, s1 = int(recs[r]["cs_start"]), int(recs[r]["cs_end"])
                out.append(dict(strand=strands[i], cs_start=s0, cs_end=s1, alignment=rows[r][s0 - 1:s1], n_nodes=self.n_nodes,
                                n_leaves=n_leaves, hit_nodes=int(hn[i]), hit_leaves=int(hl[i])))
        return out

    def tree(self) -> dict:
        """hu_db_get_tree: parent, blen, height of every node and the node rows seq [n][cs_len]"""
        out = dict(parent=np.zeros(self.n_nodes, np.int32), blen=np.zeros(self.n_nodes), height=np.zeros(self.n_nodes),
                   seq=np.zeros((self.n_nodes, self.cs_len), np.int8))
        _chk(load_library().hu_db_get_tree(self.h, _p(out["parent"], C.c_int32), _p(out["blen"], C.c_double), _p(out["seq"], C.c_int8), _p(out["height"], C.c_double)))
        return out

    def sim_plan(self, n: int, seed: int, **kw) -> dict:
        """sim_plan on this database's tree (hmmufotu-sim's choice of branch, branch point and columns for n reads)"""
        t = self.tree()
        return sim_plan(t["parent"], t["blen"], t["height"], self.cs_len, n, seed, **kw)

    def sim_gap_frac(self, msa=None) -> np.ndarray:
        """hu_sim_gap_frac: MSA::gapWFrac of every column, from the alignment msa (rows as for msa_stats; its columns with a residue must
        be this database's) or, without one, from the database's own leaf rows in node-id order"""
        out = np.zeros(self.cs_len)
        if msa is None:
            _chk(load_library().hu_sim_gap_frac(self.h, C.c_int64(0), C.c_int64(0), None, _p(out, C.c_double)))
        else:
            a = _msa_rows(msa, "sim_gap_frac")
            _chk(load_library().hu_sim_gap_frac(self.h, C.c_int64(a.shape[0]), C.c_int64(a.shape[1]), a.ctypes.data_as(C.c_char_p), _p(out, C.c_double)))
        return out

    def sim_reads(self, plan, gap_frac, seed: int, read0=0, mate=False) -> dict:
        """hu_sim_reads: the reads of a plan (node, rc, start, end as sim_plan returns them), read r being global read read0 + r of the
        seed.  aligned: per read its columns as a str of ACGT-; seq: the same without '-'; mate (mate=True): the reverse complement of
        seq; seq_len [n]."""
        node = np.ascontiguousarray(plan["node"], np.int32); rc = np.ascontiguousarray(plan["rc"], np.float64)
        st = np.ascontiguousarray(plan["start"], np.int32); en = np.ascontiguousarray(plan["end"], np.int32)
        gf = np.ascontiguousarray(gap_frac, np.float64)
        n = len(node)
        if len(rc) != n or len(st) != n or len(en) != n or len(gf) != self.cs_len:
            raise EngineError("sim_reads: a plan of %d reads needs %d entries per array, and gap_frac one per column" % (n, n))
        cols = np.maximum(en.astype(np.int64) - st + 1, 0)
        off = np.concatenate([[0], np.cumsum(cols)]).astype(np.int64)
        total = max(int(off[-1]), 1)
        al = np.zeros(total, np.uint8); sq = np.zeros(total, np.uint8); mt = np.zeros(total if mate else 1, np.uint8); ln = np.zeros(max(n, 1), np.int32)
        _chk(load_library().hu_sim_reads(self.h, C.c_int64(n), _p(node, C.c_int32), _p(rc, C.c_double), _p(st, C.c_int32), _p(en, C.c_int32), _p(gf, C.c_double),
                                         C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(read0)), C.c_int(int(mate)), al.ctypes.data_as(C.c_char_p),
                                         sq.ctypes.data_as(C.c_char_p), mt.ctypes.data_as(C.c_char_p), _p(ln, C.c_int32)))
        ab, sb, mb = al.tobytes(), sq.tobytes(), mt.tobytes()
        out = dict(aligned=[ab[off[r]:off[r + 1]].decode() for r in range(n)], seq=[sb[off[r]:off[r] + ln[r]].decode() for r in range(n)], seq_len=ln[:n].copy())
        if mate:
            out["mate"] = [mb[off[r]:off[r] + ln[r]].decode() for r in range(n)]
        return out

    def otu_consensus(self):
        """hu_otucs_create: the accumulator of the OTU consensus sequences of hmmufotu-sum -c on this database"""
        return OtuConsensus(self)

    def anno_dist(self, node: int) -> float:
        v = C.c_double()
        _chk(load_library().hu_db_get_anno_dist(self.h, C.c_int32(node), C.byref(v)))
        return float(v.value)

    def close(self):
        if self.h:
            load_library().hu_db_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SUM_DTYPE = np.dtype([("in_main", "i4"), ("taxon", "i4"), ("q_taxon", "f8"), ("n_cols", "i4"), ("n_sym", "i4"), ("n_match", "i4"),
                      ("n_match_sym", "i4")])


def sum_accept(recs, min_q=0.0, min_aln=0.0, min_hmm=0.0) -> np.ndarray:
    """hu_sum_accept (host only): which records of Batch.summary() hmmufotu-amd-sum would accept from the reads' assignment lines: in the main
    output, a taxon, Q_taxon (through its six printed digits) >= min_q, and the two identities (a threshold of 0 is off; 0 / 0 rejects)"""
    recs = np.ascontiguousarray(recs, SUM_DTYPE)
    out = np.zeros(len(recs), np.uint8)
    _chk(load_library().hu_sum_accept(recs.ctypes.data_as(C.c_void_p), C.c_int(len(recs)), C.c_double(min_q), C.c_double(min_aln), C.c_double(min_hmm),
                                      _p(out, C.c_uint8)))
    return out


def otucs_description(db_name: str, taxonomy: str, anno_dist: float, read_count: int, sample_hits: int) -> str:
    """hu_otucs_description (host only): the description of an OTU's FASTA record as hmmufotu-sum -c writes it"""
    lib = load_library()
    lib.hu_otucs_description.restype = C.c_int64
    args = (db_name.encode(), taxonomy.encode(), C.c_double(anno_dist), C.c_int64(read_count), C.c_int64(sample_hits))
    need = int(lib.hu_otucs_description(*args, None, C.c_int64(0)))
    if need < 0:
        _chk(need)
    buf = C.create_string_buffer(need + 1)
    lib.hu_otucs_description(*args, buf, C.c_int64(need + 1))
    return buf.value.decode()


class OtuConsensus:
    """Per-OTU column counts of accepted alignment rows and the consensus inferred from them (hu_otucs_*): the loop of
    src/hmmufotu-sum.cpp:391-397 and PTUnrooted::inferPostCS.  The counts stay on the device of the database."""

    def __init__(self, db: Database):
        self.db = db
        self.h = C.c_void_p()
        _chk(load_library().hu_otucs_create(db.h, C.byref(self.h)))

    def add(self, nodes, rows):
        """nodes [n]: the rows' OTUs (node ids); rows: n alignment strings (str / bytes) of cs_len columns, or a uint8 [n][cs_len] array"""
        nodes = np.ascontiguousarray(nodes, np.int32).ravel()
        L = self.db.cs_len
        if isinstance(rows, np.ndarray):
            a = np.ascontiguousarray(rows, np.uint8)
            if a.ndim != 2 or a.shape[1] != L:
                raise EngineError("otu_consensus.add: rows must be [n][%d], got %s" % (L, a.shape,))
        else:
            b = [r.encode("latin1") if isinstance(r, str) else bytes(r) for r in rows]
            for i, r in enumerate(b):
                if len(r) != L:
                    raise EngineError("otu_consensus.add: row %d has %d columns, the database %d" % (i, len(r), L))
            a = np.frombuffer(b"".join(b), np.uint8).reshape(len(b), L)
        if len(nodes) != a.shape[0]:
            raise EngineError("otu_consensus.add: %d nodes for %d rows" % (len(nodes), a.shape[0]))
        _chk(load_library().hu_otucs_add(self.h, C.c_int64(len(nodes)), _p(nodes, C.c_int32), a.ctypes.data_as(C.c_char_p)))

    def add_batch(self, batch: "Batch", accept):
        """hu_otucs_add_batch: the reads of a finished batch with accept[i] != 0, each under the taxon of its best placement; the rows are
        read where they lie on the device"""
        acc = np.ascontiguousarray(accept, np.uint8).ravel()
        if len(acc) != batch.n:
            raise EngineError("otu_consensus.add_batch: %d flags for %d reads" % (len(acc), batch.n))
        _chk(load_library().hu_otucs_add_batch(self.h, batch.h, _p(acc, C.c_uint8)))

    def add_counts(self, node: int, freq, gap):
        """hu_otucs_add_counts: freq [4][cs_len] and gap [cs_len] added to the counts of one OTU (the inverse of counts())"""
        L = self.db.cs_len
        freq = np.ascontiguousarray(freq, np.uint32); gap = np.ascontiguousarray(gap, np.uint32)
        if freq.shape != (4, L) or gap.shape != (L,):
            raise EngineError("otu_consensus.add_counts: freq must be [4][%d] and gap [%d]" % (L, L))
        _chk(load_library().hu_otucs_add_counts(self.h, C.c_int32(node), _p(freq, C.c_uint32), _p(gap, C.c_uint32)))

    def counts(self, node: int):
        """(freq [4][cs_len], gap [cs_len]) of one OTU, uint32"""
        L = self.db.cs_len
        freq = np.zeros((4, L), np.uint32); gap = np.zeros(L, np.uint32)
        _chk(load_library().hu_otucs_counts(self.h, C.c_int32(node), _p(freq, C.c_uint32), _p(gap, C.c_uint32)))
        return freq, gap

    def infer(self, nodes, eff_n=2.0):
        """the consensus of each OTU, a str of cs_len characters of ACGT and '-'"""
        nodes = np.ascontiguousarray(nodes, np.int32).ravel()
        L = self.db.cs_len
        out = np.zeros((len(nodes), L), np.uint8)
        _chk(load_library().hu_otucs_infer(self.h, C.c_int32(len(nodes)), _p(nodes, C.c_int32), C.c_double(eff_n), out.ctypes.data_as(C.c_char_p)))
        return [bytes(r).decode("ascii") for r in out]

    def close(self):
        if self.h:
            load_library().hu_otucs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


OtuCs = OtuConsensus


class Window(C.Structure):
    _fields_ = [("win_start", C.c_int64), ("win_len", C.c_int64)]


def windows_plan(cs_len: int, n_win: int, overlap: int):
    """hu_windows_plan: n_win column windows [(start, len)] covering [0, cs_len), neighbours overlapping by `overlap` columns"""
    w = (Window * n_win)()
    _chk(load_library().hu_windows_plan(C.c_int64(cs_len), C.c_int(n_win), C.c_int64(overlap), w))
    return [(int(x.win_start), int(x.win_len)) for x in w]


class WindowedDatabase:
    """Column-window sharding (last row; include/hmmufotu_amd.h): one database held as W column windows — one hu_db per window,
    usually one per device — for message sets beyond one GPU's HBM.  PTUnrooted::load keeps every column of every edge (src/PhyloTreeUnrooted.cpp:496-535);
    here a read is routed to the window that holds the columns its seeds point at, and re-routed ONCE by its exact region when it comes back
    HU_READ_OUT_OF_WINDOW.  The windows never exchange anything."""

    def __init__(self, dbs, windows):
        assert len(dbs) == len(windows) >= 1
        self.dbs = list(dbs); self.windows = [(int(a), int(b)) for a, b in windows]
        self._w = (Window * len(windows))(*[Window(a, b) for a, b in self.windows])
        self.last = {}

    @classmethod
    def from_synth(cls, db, n_win, overlap, devices=None):
        md = model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r if db.dg_k > 0 else None)
        wins = windows_plan(db.cs_len, n_win, overlap)
        dbs = [Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, db.up[:, a:a + l], db.down[:, a:a + l], db.height, md, db.anno_id, db.anno_dist,
                                    win_start=a, win_len=l, device=(devices[i] if devices else 0)) for i, (a, l) in enumerate(wins)]
        return cls(dbs, wins)

    @classmethod
    def load(cls, hmm_path, ptu_path, cs_len, n_win, overlap, devices=None):
        wins = windows_plan(cs_len, n_win, overlap)
        return cls([Database.load(hmm_path, ptu_path, devices[i] if devices else 0, a, l) for i, (a, l) in enumerate(wins)], wins)

    def route_by_seeds(self, lens, vpaths, mate_lens=None, mvpaths=None):
        n = len(lens)
        lens = np.ascontiguousarray(lens, np.int32); vp = np.ascontiguousarray(vpaths, np.int32).reshape(n, 12)
        ml = np.ascontiguousarray(mate_lens, np.int32) if mate_lens is not None else None
        mv = np.ascontiguousarray(mvpaths, np.int32).reshape(n, 12) if mvpaths is not None else None
        out = np.zeros(n, np.int32)
        _chk(load_library().hu_route_by_seeds(self.dbs[0].h, C.c_int(len(self.windows)), self._w, C.c_int(n), _p(lens, C.c_int32), _p(vp, C.c_int32),
                                              _p(ml, C.c_int32) if ml is not None else None, _p(mv, C.c_int32) if mv is not None else None, _p(out, C.c_int32)))
        return out

    def route_by_region(self, cs_start, cs_end):
        s_ = np.ascontiguousarray(cs_start, np.int32); e_ = np.ascontiguousarray(cs_end, np.int32)
        out = np.zeros(len(s_), np.int32)
        _chk(load_library().hu_route_by_region(C.c_int(len(self.windows)), self._w, C.c_int(len(s_)), _p(s_, C.c_int32), _p(e_, C.c_int32), _p(out, C.c_int32)))
        return out

    def assign(self, reads, vpaths, opts, mates=None, mvpaths=None, first_window=None, ids=None, annos=None):
        """The whole per-read task over the windows: route by seeds, one batch per window, re-route the reads that came back out of their window by
        their region, merge in read order.  Returns (placements [n], alignment records [n]); self.last holds the routing (window per read, reads
        re-routed, reads no window holds) and, with ids, the TSV lines per read.  first_window: a routing to use instead of the seeds' (tests)."""
        n = len(reads)
        vp = np.ascontiguousarray(vpaths, np.int32).reshape(n, 2, 6)
        mvp = np.ascontiguousarray(mvpaths, np.int32).reshape(n, 2, 6) if mvpaths is not None else None
        win = np.asarray(first_window, np.int32) if first_window is not None else \
            self.route_by_seeds([len(r) for r in reads], vp, [len(r) for r in mates] if mates is not None else None, mvp)
        best = np.zeros(n, PLACE_DTYPE); recs = np.zeros(n, ALIGN_DTYPE); lines = [None] * n
        final = win.copy(); rerouted = np.zeros(n, bool)

        def run(w, idx):
            B = Batch(self.dbs[w], len(idx))
            B.set_reads([reads[i] for i in idx], vp[idx], [mates[i] for i in idx] if mates is not None else None, mvp[idx] if mvp is not None else None)
            B.assign(opts)
            b_, r_ = B.placements().copy(), B.alignments(want_align=False)["recs"].copy()
            t_ = None
            if ids is not None:     # a read that is not placed has no line: keyed by the read id at the head of each line
                txt = B.format_tsv([ids[i] for i in idx], None, annos).strip("\n")
                t_ = {l.split("\t", 1)[0]: l for l in txt.split("\n")} if txt else {}
            B.close()
            return b_, r_, t_

        def take(idx, b_, r_, t_):
            best[idx] = b_; recs[idx] = r_
            if t_ is not None:
                for i in idx:
                    lines[i] = t_.get(ids[i])
        for w in range(len(self.dbs)):
            idx = np.nonzero(win == w)[0]
            if len(idx):
                take(idx, *run(w, idx))
        out = np.nonzero(recs["status"] == READ_OUT_OF_WINDOW)[0]
        if len(out):
            w2 = self.route_by_region(recs["cs_start"][out], recs["cs_end"][out])
            for w in range(len(self.dbs)):
                idx = out[(w2 == w) & (win[out] != w)]
                if len(idx):
                    take(idx, *run(w, idx)); final[idx] = w; rerouted[idx] = True
        self.last = dict(first_window=win, window=final, rerouted=rerouted, unplaceable=(recs["status"] == READ_OUT_OF_WINDOW), lines=lines)
        return best, recs

    def close(self):
        for d in self.dbs:
            d.close()


class Batch:
    """One batch of reads in flight on one HIP stream (hu_batch)."""

    def __init__(self, db: Database, max_reads: int):
        self.db = db
        self.h = C.c_void_p()
        self.n = 0
        _chk(load_library().hu_batch_create(db.h, C.c_int(max_reads), C.byref(self.h)))

    # ---- inputs
    def set_reads(self, reads, vpaths, mates=None, mvpaths=None):
        n = len(reads)
        self.n = n
        cat = "".join(reads).encode("latin1")
        offs = np.zeros(n + 1, np.int64); offs[1:] = np.cumsum([len(r) for r in reads])
        vp = np.ascontiguousarray(vpaths, np.int32).reshape(n, 2, 6) if vpaths is not None else None
        if mates is not None:
            mcat = "".join(mates).encode("latin1")
            moffs = np.zeros(n + 1, np.int64); moffs[1:] = np.cumsum([len(r) for r in mates])
            mvp = np.ascontiguousarray(mvpaths, np.int32).reshape(n, 2, 6) if mvpaths is not None else None
        _chk(load_library().hu_batch_set_reads(self.h, C.c_int(n), cat, _p(offs, C.c_int64), _p(vp, C.c_int32) if vp is not None else None,
                                               mcat if mates is not None else None, _p(moffs, C.c_int64) if mates is not None else None,
                                               _p(mvp, C.c_int32) if mates is not None and mvp is not None else None))

    def set_reads_packed(self, cat, offs, vpaths):
        """SE reads as one uint8 buffer + offsets [n + 1] (relative to the buffer's start): no per-read Python objects"""
        offs = np.ascontiguousarray(offs, np.int64); n = len(offs) - 1
        self.n = n
        vp = np.ascontiguousarray(vpaths, np.int32).reshape(n, 2, 6)
        _chk(load_library().hu_batch_set_reads(self.h, C.c_int(n), cat.ctypes.data_as(C.c_char_p), _p(offs, C.c_int64), _p(vp, C.c_int32), None, None, None))

    def format_tsv_bytes(self, id_array, desc_array=None, anno_array=None) -> int:
        """formats the batch's assignment lines (hu_batch_format_tsv_ptr) from prepared (c_char_p * n) arrays and returns their length;
        the text stays in the batch's buffer"""
        lib = load_library()
        lib.hu_batch_format_tsv_ptr.restype = C.c_int64
        txt = C.c_char_p()
        need = lib.hu_batch_format_tsv_ptr(self.h, id_array, desc_array, anno_array, None, C.c_int(0), C.c_int(0), C.byref(txt))
        if need < 0:
            _chk(int(need))
        return int(need)

    def set_aligned(self, codes, start, end):
        codes = np.ascontiguousarray(codes, np.int8)
        n = codes.shape[0]
        self.n = n
        s = np.ascontiguousarray(start, np.int32); e = np.ascontiguousarray(end, np.int32)
        _chk(load_library().hu_batch_set_aligned(self.h, C.c_int(n), _p(codes, C.c_int8), _p(s, C.c_int32), _p(e, C.c_int32)))

    # ---- stages (reference names in the docstrings of include/hmmufotu_amd.h)
    def align(self, opts): _chk(load_library().hu_align_batch(self.h, C.byref(opts)))
    def get_seed(self, opts): _chk(load_library().hu_seed_batch(self.h, C.byref(opts)))
    def estimate_seq(self, opts): _chk(load_library().hu_estimate_batch(self.h, C.byref(opts)))
    def filter_placements(self, opts): _chk(load_library().hu_filter_batch(self.h, C.byref(opts)))
    def place_seq(self, opts): _chk(load_library().hu_place_batch(self.h, C.byref(opts)))
    def calc_q_values(self, opts): _chk(load_library().hu_finish_batch(self.h, C.byref(opts)))
    def assign(self, opts): _chk(load_library().hu_assign_batch(self.h, C.byref(opts)))
    def sync(self): _chk(load_library().hu_batch_sync(self.h))
    def profile(self, enable=True): _chk(load_library().hu_batch_profile(self.h, C.c_int(int(enable))))

    def set_knob(self, name: str, value: int = 1):
        """hu_batch_set_knob: pick an alternative kernel / diagnostic for this batch (tests force every kernel path with it)."""
        _chk(load_library().hu_batch_set_knob(self.h, name.encode(), C.c_int(int(value))))

    def refsort_stats(self):
        """(reads of the last seed stage in the reference's order that the device sort left to the host, whole batch on the host path?)"""
        a = C.c_int32(0); w = C.c_int32(0)
        _chk(load_library().hu_batch_refsort_stats(self.h, C.byref(a), C.byref(w)))
        return int(a.value), bool(w.value)

    def wall(self):
        ms = np.zeros(4)
        _chk(load_library().hu_batch_wall(self.h, _p(ms, C.c_double)))
        return dict(align=ms[0], seed_estimate_filter=ms[1], place=ms[2], finish=ms[3])

    def timings(self):
        ms = np.zeros(8, np.float32)
        _chk(load_library().hu_batch_timings(self.h, _p(ms, C.c_float)))
        return {T_NAMES[i]: float(ms[i]) for i in range(6)}

    # ---- results
    def alignments(self, want_align=True, want_trace=False, trace_stride=0):
        n, L = self.n, self.db.cs_len
        recs = np.zeros(n, ALIGN_DTYPE)
        rows = np.zeros((n, L), np.uint8) if want_align else None
        tr = np.zeros((n, trace_stride), np.uint8) if want_trace else None
        _chk(load_library().hu_batch_get_alignments(self.h, recs.ctypes.data_as(C.c_void_p),
                                                    rows.ctypes.data_as(C.c_char_p) if rows is not None else None,
                                                    tr.ctypes.data_as(C.c_char_p) if tr is not None else None, C.c_int(trace_stride)))
        out = dict(recs=recs)
        if rows is not None:
            out["align"] = [rows[i].tobytes().decode("latin1") for i in range(n)]
        if tr is not None:
            out["trace"] = [tr[i].tobytes().split(b"\0")[0].decode() for i in range(n)]
        return out

    def codes(self):
        n, L = self.n, self.db.cs_len
        cd = np.zeros((n, L), np.int8); s = np.zeros(n, np.int32); e = np.zeros(n, np.int32)
        _chk(load_library().hu_batch_get_codes(self.h, _p(cd, C.c_int8), _p(s, C.c_int32), _p(e, C.c_int32)))
        return cd, s, e

    def anneal(self, row_of_primer, max_dist, as_read=None):
        """hu_anneal_batch: (hit_nodes, hit_leaves) per primer for its chosen aligned row (negative: skipped, -1).  as_read: per primer the
        text of its row in the case it was read (None: the row's upper-case bases); the rows take that case."""
        rows = np.ascontiguousarray(row_of_primer, np.int32)
        n = len(rows)
        hn = np.zeros(n, np.int64); hl = np.zeros(n, np.int64)
        txt = (C.c_char_p * n)(*[t.encode("latin1") if t is not None else None for t in as_read]) if as_read is not None else None
        _chk(load_library().hu_anneal_batch(self.h, _p(rows, C.c_int32), C.c_int(n), txt, C.c_double(max_dist), _p(hn, C.c_int64), _p(hl, C.c_int64)))
        return hn, hl

    def pdist(self, read: int):
        d = np.zeros(self.db.n_nodes, np.int32); N = np.zeros(self.db.n_nodes, np.int32)
        _chk(load_library().hu_batch_get_pdist(self.h, C.c_int(read), _p(d, C.c_int32), _p(N, C.c_int32)))
        return d, N

    def seeds(self):
        n = self.n
        cnt = np.zeros(n, np.int32); ids = np.zeros((n, HU_MAX_SEEDS), np.int32); d = np.zeros_like(ids); N = np.zeros_like(ids)
        _chk(load_library().hu_batch_get_seeds(self.h, _p(cnt, C.c_int32), _p(ids, C.c_int32), _p(d, C.c_int32), _p(N, C.c_int32)))
        return cnt, ids, d, N

    def seeds_strided(self, stride: int, guard: int = 0):
        """hu_batch_get_seeds_strided into [n][stride] buffers followed by `guard` sentinel entries (ABI test)."""
        n = self.n
        cnt = np.zeros(n, np.int32)
        bufs = [np.full(n * stride + guard, -777, np.int32) for _ in range(3)]
        _chk(load_library().hu_batch_get_seeds_strided(self.h, _p(cnt, C.c_int32), *[_p(b, C.c_int32) for b in bufs], C.c_int(stride)))
        return (cnt,) + tuple(bufs)

    def estimates_strided(self, stride: int, guard: int = 0):
        n = self.n
        bufs = [np.full(n * stride + guard, -777.0) for _ in range(3)]
        _chk(load_library().hu_batch_get_estimates_strided(self.h, *[_p(b, C.c_double) for b in bufs], C.c_int(stride)))
        return tuple(bufs)

    def estimates(self):
        n = self.n
        r = np.zeros((n, HU_MAX_SEEDS)); w = np.zeros_like(r); ll = np.zeros_like(r)
        _chk(load_library().hu_batch_get_estimates(self.h, _p(r, C.c_double), _p(w, C.c_double), _p(ll, C.c_double)))
        return r, w, ll

    def candidates(self):
        offs = np.zeros(self.n + 1, np.int64)
        _chk(load_library().hu_batch_get_candidates(self.h, _p(offs, C.c_int64), None, None, None, None, None))
        m = int(offs[-1])
        c = np.zeros(m, np.int32); r = np.zeros(m); w = np.zeros(m); e = np.zeros(m); it = np.zeros(m, np.int32)
        _chk(load_library().hu_batch_get_candidates(self.h, _p(offs, C.c_int64), _p(c, C.c_int32), _p(r, C.c_double), _p(w, C.c_double),
                                                    _p(e, C.c_double), _p(it, C.c_int32)))
        return dict(offs=offs, c_node=c, ratio=r, wnr=w, est_loglik=e, iters=it)

    def placements(self):
        out = np.zeros(self.n, PLACE_DTYPE)
        _chk(load_library().hu_batch_get_placements(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def candidate_places(self):
        """Every candidate's placement record after calc_q_values, in filterPlacements order."""
        offs = np.zeros(self.n + 1, np.int64)
        _chk(load_library().hu_batch_get_candidates(self.h, _p(offs, C.c_int64), None, None, None, None, None))
        out = np.zeros(int(offs[-1]), PLACE_DTYPE)
        _chk(load_library().hu_batch_get_candidate_places(self.h, out.ctypes.data_as(C.c_void_p)))
        return offs, out

    def set_candidates(self, offs, recs, placed=False):
        """hu_batch_set_candidates: the candidates of every read given by the caller (records of PLACE_DTYPE in the order the later stages
        are to see them); placed: they carry placeSeq's results and calc_q_values may follow, else place_seq may follow"""
        offs = np.ascontiguousarray(offs, np.int64); recs = np.ascontiguousarray(recs, PLACE_DTYPE)
        assert len(offs) == self.n + 1 and offs[-1] == len(recs)
        _chk(load_library().hu_batch_set_candidates(self.h, _p(offs, C.c_int64), recs.ctypes.data_as(C.c_void_p), C.c_int(int(placed))))

    def get_seed_given(self, n_seeds, ids, dist_ids=None):
        """Segment form of the seed stage: given node ids, distances over the current regions (src/hmmufotu.cpp:662-665)."""
        n_seeds = np.ascontiguousarray(n_seeds, np.int32); ids = np.ascontiguousarray(ids, np.int32)
        assert ids.ndim == 2 and ids.shape[0] == self.n == len(n_seeds)
        di = None
        if dist_ids is not None:
            di = np.ascontiguousarray(dist_ids, np.int32); assert di.shape == ids.shape
        _chk(load_library().hu_seed_batch_given(self.h, _p(n_seeds, C.c_int32), _p(ids, C.c_int32), _p(di, C.c_int32) if di is not None else None,
                                                C.c_int(ids.shape[1])))

    def check_chimera(self, work: "Batch", opts, num_seg=2, max_chimera_error=None, min_chimera_lod=0.0):
        """-C of the per-read task (src/hmmufotu.cpp:653-691) for a batch that is at least seeded; `work` is a second batch
        on the same database whose contents are overwritten."""
        co = ChimeraOpts(num_seg, 0, opts.max_error / num_seg if max_chimera_error is None else max_chimera_error, min_chimera_lod)
        out = np.zeros(self.n, CHIMERA_DTYPE)
        _chk(load_library().hu_chimera_batch(self.h, work.h, C.byref(opts), C.byref(co), out.ctypes.data_as(C.c_void_p)))
        return out

    def summary(self, chimera=None) -> np.ndarray:
        """hu_batch_get_summary of a finished batch: per read whether its line stands in the main output, its taxon and Q_taxon, and the
        integers behind the two identities, counted on the device (records of SUM_DTYPE).  chimera: the records of check_chimera, or None"""
        cp = None
        if chimera is not None:
            chimera = np.ascontiguousarray(chimera, CHIMERA_DTYPE); assert len(chimera) == self.n
            cp = chimera.ctypes.data_as(C.c_void_p)
        out = np.zeros(self.n, SUM_DTYPE)
        _chk(load_library().hu_batch_get_summary(self.h, cp, out.ctypes.data_as(C.c_void_p)))
        return out

    def format_tsv(self, ids, descs=None, annos=None) -> str:
        return self.format_tsv_chimera(ids, descs, annos, None, False, 0)

    def format_tsv_chimera(self, ids, descs=None, annos=None, chimera=None, chimera_info=False, which=0) -> str:
        """Assignment lines: which=0 the main file, which=1 --chimera-out, which=2 --align-only (src/hmmufotu.cpp:693-747)."""
        lib = load_library()
        lib.hu_batch_format_tsv_ptr.restype = C.c_int64
        arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs]) if xs is not None else None
        a_ids, a_desc, a_anno = arr(ids), arr(descs), arr(annos)
        cp = None
        if chimera is not None:
            chimera = np.ascontiguousarray(chimera, CHIMERA_DTYPE); assert len(chimera) == self.n
            cp = chimera.ctypes.data_as(C.c_void_p)
        txt = C.c_char_p()
        need = lib.hu_batch_format_tsv_ptr(self.h, a_ids, a_desc, a_anno, cp, C.c_int(int(chimera_info)), C.c_int(which), C.byref(txt))
        if need < 0:
            _chk(int(need))
        return C.string_at(txt, need).decode("latin1") if need else ""

    def format_tsv_copy(self, ids, descs=None, annos=None) -> str:
        """the (buf, cap) form of the ABI: size first, then the copy"""
        lib = load_library()
        lib.hu_batch_format_tsv.restype = C.c_int64
        arr = lambda xs: (C.c_char_p * len(xs))(*[x.encode() for x in xs]) if xs is not None else None
        a_ids, a_desc, a_anno = arr(ids), arr(descs), arr(annos)
        need = lib.hu_batch_format_tsv(self.h, a_ids, a_desc, a_anno, None, C.c_int64(0))
        if need < 0:
            _chk(int(need))
        buf = C.create_string_buffer(int(need) + 1)
        lib.hu_batch_format_tsv(self.h, a_ids, a_desc, a_anno, buf, C.c_int64(need))
        return buf.raw[:need].decode("latin1")

    def close(self):
        if self.h:
            load_library().hu_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
