"""k_place_blk bit for bit: ratio, wnr and the iteration counts of every candidate of a few small batches against what the placement gave
when tests/golden/place_bits/ was written (tests/make_place_bits_golden.py), as integers.  The kernel's table builds and the start of its EM
calls may be rescheduled, never recomputed differently: a change that keeps every operation and its order leaves these bits alone, where
the 50-digit pins of tests/test_hiprec_gpu.py allow a last bit to move.

A case per instance (tests/place_bits_cases.py): the twelve-site split-slot instance, the four-wave all-register instance and the instance
with v in LDS, each without dGamma and with four rate categories; the split-slot instance also with 8 and 16 categories, where a build's
exponentials and the EM's starting one no longer fit the workgroup's first trip; and a set with a branch of length 0 (the EM's degenerate
path) and a read whose every base is a transversion away from its leaf's (q falls to 0 in one step and wnr ends at the clamp).  Every case must hold a candidate that ran a second outer iteration and a second EM step, so that the second table build and a
rebuilt first one are among what is compared."""
import numpy as np
import pytest

import place_bits_cases as PB

pytestmark = pytest.mark.gpu


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


@pytest.mark.parametrize("name", PB.CASE_IDS)
def test_place_bits(capfd, name):
    E = _engine()
    with np.load(PB.golden_path(name)) as z:
        want = {k: z[k] for k in z.files}
    kernel, zero = PB.make_case(name)[5:7]
    capfd.readouterr()
    got = PB.run_case(E, name)
    assert PB.placed_by(capfd.readouterr().err) == [kernel]
    # the archive reaches what the case is there for
    outer, em = want["iters"] & 0xff, want["iters"] >> 8
    assert len(outer) >= PB.MIN_CANDIDATES and ((outer > 1) & (em > 1)).any()
    if zero is not None:
        assert (want["c_node"] == zero).any() and (want["wnr"].view(np.float64) == 1.0).any()
    # every candidate, every field, as integers
    assert sorted(got) == sorted(want)
    for key in ("offs", "c_node", "iters", "wnr", "ratio"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        bad = np.flatnonzero(got[key] != want[key])
        assert bad.size == 0, (key, bad[:8], got[key][bad[:8]], want[key][bad[:8]])
