"""Writes tests/golden/place_bits/<case>.npz: what the placement stage gives for every candidate of the cases of
tests/place_bits_cases.py, as raw integers (ratio and wnr as their 64 bits, iters = outer | EM << 8).  Run it on an MI355X at the commit
whose results are to be pinned; tests/test_place_bits_gpu.py then holds every later build of k_place_blk to these bits.

    python3 tests/make_place_bits_golden.py [case ...]

It refuses to write a case that does not reach what it is there for: the expected instance, a second outer iteration and a second EM step,
and for the edge set the zero-length branch and the clamp."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))

import place_bits_cases as PB  # noqa: E402


def reaches(name, got, zero):
    """why the case does not reach its code paths, or None"""
    outer, em = got["iters"] & 0xff, got["iters"] >> 8
    if len(outer) < PB.MIN_CANDIDATES:
        return "only %d candidates" % len(outer)
    if not ((outer > 1) & (em > 1)).any():
        return "no candidate with a second outer iteration and a second EM step"
    if zero is not None:
        if not (got["c_node"] == zero).any():
            return "no candidate on the zero-length branch"
        if not (got["wnr"].view(np.float64) == 1.0).any():
            return "no wnr at the clamp"
    return None


def main():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        raise SystemExit("needs a gfx950 device")
    os.makedirs(PB.GOLDEN, exist_ok=True)
    for name in sys.argv[1:] or PB.CASE_IDS:
        zero = PB.make_case(name)[6]
        got = PB.run_case(E, name)
        why = reaches(name, got, zero)
        if why:
            raise SystemExit("%s: %s" % (name, why))
        np.savez_compressed(PB.golden_path(name), **got)
        outer, em = got["iters"] & 0xff, got["iters"] >> 8
        print("%s: %d candidates, outer %d..%d, EM steps %d..%d" % (name, len(outer), outer.min(), outer.max(), em.min(), em.max()))


if __name__ == "__main__":
    main()
