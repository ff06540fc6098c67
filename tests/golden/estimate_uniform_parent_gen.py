"""Writes tests/golden/estimate_uniform_parent.npz: what every launch of tests/test_estimate_uniform.py gives on the commit this script runs on.

Run once on the MI355X, on the commit BEFORE a change that must not move a bit (copy this file and tests/test_estimate_uniform.py into that
checkout, build it, run `python tests/golden/estimate_uniform_parent_gen.py`), and commit the file it writes with the change.  The file
holds, per launch (a width class or the width-split batch, unweighted and weighted), every read's seed count and every (read, seed) slot's
node, (d, N), ratio, wnr and loglik.  The exact copy's unweighted wnr must come out as 0 on every one of its seeds."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: conftest.py puts the repository root on the path

import test_estimate_uniform as T                              # noqa: E402


def main():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    db = T.make_db()
    res = T.run_cases(E, db, T.make_cases(db))
    for M in T.CLASSES:
        k = int(res["c%d.w0.seed_cnt" % M][T.I_EXACT])
        assert k > 0 and (res["c%d.w0.est_wnr" % M][T.I_EXACT, :k] == 0.0).all(), (M, res["c%d.w0.est_wnr" % M][T.I_EXACT, :k])
    out = os.path.join(HERE, "estimate_uniform_parent.npz")
    np.savez_compressed(out, **res)
    print("%s: %d arrays, %d bytes" % (out, len(res), os.path.getsize(out)))


if __name__ == "__main__":
    main()
