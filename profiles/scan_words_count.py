"""How many of the 32-site words that the seed scan runs hold a base of any read of their tile (pair scan).
The scan's tile is sixteen reads in order of region start; k_tile_lists names the quads (128 scan positions, four words) in which
a read of the tile has a base, and the scan kernels ran all four words of every listed quad.  For the first batch of bench.py's
workload (database seed 97, reads seed 1; --leaves=N for a smaller tree: the tiling does not depend on the tree's size, only on
the profile and the reads) this counts, per tile,
    (a) the words of the listed quads,
    (b) the words in which at least one read of the tile has a base,
from Batch.codes() after the alignment and the scan order of the columns (profile columns first, HuDbDev::posCol), with the
reads' bases on non-profile columns treated as planes_of_codes treats them (up to HU_MAX_INS of them travel as a list and are
in no word).  Three workloads: the headline (SE 250 bp on one amplicon), --uniform-starts and --paired --read-len 250.
(b) / (a) is the share of the scan's (node, read, 32 sites) steps that a per-quad word mask leaves.  --out=DIR: where the JSON goes."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from hmmufotu_amd import engine as E, synth, synth_gpu

T, MAX_INS = 16, 24          # HU_READ_TILE, HU_MAX_INS


def arg(name, default):
    return next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--%s=" % name)), default)


def count(codes, start, end, p2cs, K):
    """(a), (b) summed over the tiles, tiles, and the histogram of listed words per tile"""
    n, L = codes.shape
    WQ, QM = (L + 127) // 128, (K + 127) // 128
    prof = np.asarray(p2cs[1:K + 1], np.int64) - 1
    rest = np.setdiff1d(np.arange(L), prof)
    pos_col = np.concatenate([prof, rest])                         # scan position -> column
    col = np.arange(L)
    has = (codes >= 0) & (col[None, :] >= start[:, None]) & (col[None, :] <= end[:, None])
    at = np.zeros((n, WQ * 128), bool)
    at[:, :L] = has[:, pos_col]
    listed = at[:, QM * 128:].sum(1) <= MAX_INS                     # their non-profile bases travel as a list
    at[listed, QM * 128:] = False
    words = at.reshape(n, WQ * 4, 32).any(2)
    key = np.where(end >= start, start.astype(np.int64) + 1, 0x7fffffff)
    order = np.argsort(key, kind="stable")
    tiles = (n + T - 1) // T
    tw = np.zeros((tiles * T, WQ * 4), bool)
    tw[:n] = words[order]
    tw = tw.reshape(tiles, T, WQ * 4).any(1)
    b = tw.sum(1)
    a = 4 * tw.reshape(tiles, WQ, 4).any(2).sum(1)
    return int(a.sum()), int(b.sum()), tiles, np.bincount(a).tolist(), np.bincount(b).tolist()


def main():
    out_dir = arg("out", os.path.join(ROOT, "profiles"))
    leaves, cs_len, batch = int(arg("leaves", 99322)), int(arg("cs-len", 7682)), int(arg("batch", 8192))
    if E.device_count() < 1:
        sys.exit("scan_words_count: no gfx950 device")
    dev = "cuda:0"
    db, up, down = synth_gpu.make_db_gpu(leaves, cs_len, "GTR", dg_k=4, seed=97, win=None, device=dev, log=lambda *a: None)
    amp_start = 1000 if cs_len > 4000 else 30
    sets = {}
    for name, paired, uniform in (("headline", False, False), ("uniform_starts", False, True), ("paired_250", True, False)):
        ins_len = int(round(250 * 1.84)) if paired else 250
        amp_cols = int(round(ins_len * cs_len / 1400.0))
        reads = synth_gpu.simulate_reads_gpu(db, up, down, batch, 100000 if paired else 250, seed=1, amplicon_start=amp_start, amplicon_cols=amp_cols,
                                             device=dev, uniform=uniform)
        if paired:
            fw, mt = zip(*[synth.split_pair(r, 250) for r in reads])
            sets[name] = ([r.seq for r in fw], np.stack([synth.read_vpaths(db.hmm, r) for r in fw]),
                          [r.seq for r in mt], np.stack([synth.read_vpaths(db.hmm, r) for r in mt]))
        else:
            sets[name] = ([r.seq for r in reads], np.stack([synth.read_vpaths(db.hmm, r) for r in reads]))
    md = E.model_desc(db.model.type_id, db.model.pi, db.model.par, db.dg_r)
    D = E.Database.from_arrays(db.hmm, db.parent, db.blen, db.seq, up.data_ptr(), down.data_ptr(), db.height, md, db.anno_id, device=0, msgs_on_device=True)
    out = dict(leaves=leaves, cs_len=cs_len, K=int(db.hmm.K), batch=batch, read_tile=T)
    for name, rd in sets.items():
        B = E.Batch(D, batch)
        B.set_reads(*rd)
        B.align(E.default_opts()); B.sync()
        cd, st, en = B.codes()
        a, b, tiles, ha, hb = count(cd, st, en, db.hmm.p2cs, db.hmm.K)
        out[name] = dict(tiles=tiles, aligned=int((en >= st).sum()), words_of_listed_quads=a, words_with_a_base=b, ratio=b / a,
                         words_of_listed_quads_per_tile=a / tiles, words_with_a_base_per_tile=b / tiles,
                         tiles_by_words_of_listed_quads=ha, tiles_by_words_with_a_base=hb)
        print(name, {k: v for k, v in out[name].items() if not k.startswith("tiles_by")}, flush=True)
        B.close()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "scan_words_count.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
