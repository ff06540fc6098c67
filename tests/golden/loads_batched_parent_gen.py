"""Writes tests/golden/loads_batched_parent.npz: what every launch of tests/test_loads_batched.py gives on the commit this script runs on.

Run once on the MI355X, on the commit BEFORE a change that must not move a bit (copy this file and tests/test_loads_batched.py into that
checkout, build it, run `python tests/golden/loads_batched_parent_gen.py`), and commit the file it writes with the change.  The file
holds, per launch, every (read, seed) slot's ratio / wnr / loglik and every candidate's node, ratio, wnr, estimated loglik and
iteration counts (outer iterations and EM steps, packed as the engine returns them)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: conftest.py puts the repository root on the path

import test_loads_batched as T                                 # noqa: E402


def main():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    db = T.make_db()
    res = T.run_cases(E, db, T.make_cases(db))
    out = os.path.join(HERE, "loads_batched_parent.npz")
    np.savez_compressed(out, **res)
    print("%s: %d arrays, %d bytes" % (out, len(res), os.path.getsize(out)))


if __name__ == "__main__":
    main()
