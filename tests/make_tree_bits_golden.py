"""Writes tests/golden/tree_bits/<case>.npz: what the tree family (branch step, NNI scores, supports, SPR scores, insertion scores and
the three searches) gives for the cases of tests/tree_bits_cases.py, as raw integers (a float as its 64 bits).  Run it on an MI355X at
the commit whose results are to be pinned; tests/test_tree_bits_gpu.py then holds every later build of the kernels to these bits.

    python3 tests/make_tree_bits_golden.py [case ...]
    python3 tests/make_tree_bits_golden.py --host --out=DIR [case ...]

--host runs the same cases on the library's host path and needs no device; its archives serve a before / after comparison on one
machine (exp and log of the host's libm need not agree between machines), so --out is required with it and nothing of it is committed.

It refuses to write a case that does not reach what it is there for: a t_star that left its start, a t_star inside the bounds, and for
a search an accepted round."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))

import tree_bits_cases as TB  # noqa: E402


def main():
    from hmmufotu_amd import engine as E
    args = sys.argv[1:]
    host = "--host" in args
    out = [a[len("--out="):] for a in args if a.startswith("--out=")]
    names = [a for a in args if not a.startswith("--")]
    if host and not out:
        raise SystemExit("--host needs --out=DIR: the host path's bits are no committed golden")
    if not host and E.device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    root = out[0] if out else TB.GOLDEN
    os.makedirs(root, exist_ok=True)
    for name in names or TB.CASE_IDS:
        got = TB.run_case(E, name, host)
        why = TB.reaches(name, got)
        if why:
            raise SystemExit("%s: %s" % (name, why))
        np.savez_compressed(TB.golden_path(name, root), **got)
        print("%s: %s" % (name, ", ".join("%s %s" % (k, "x".join(map(str, v.shape))) for k, v in got.items())))


if __name__ == "__main__":
    main()
