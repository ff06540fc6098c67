"""The tree family bit for bit: every result of k_blen_step, k_nni_score, k_nni_support, k_spr_score, k_add_score / k_add_best and of
one small NNI, SPR and insertion search against what the device gave when tests/golden/tree_bits/ was written
(tests/make_tree_bits_golden.py), as integers.  The family's code may be shared and moved, never recomputed differently: a change that
keeps every operation and its order leaves these bits alone, where the device-against-host tests of tests/test_tree_*.py allow a last
bit to move.

The cases (tests/tree_bits_cases.py) are the smallest shapes of those tests on either side of every switch between two kernel
instances.  Every archive must hold a t_star that left its start and one inside the bounds, every search an accepted round, so that a
Newton loop that iterated and a committed round are among what is compared."""
import numpy as np
import pytest

import tree_bits_cases as TB

pytestmark = pytest.mark.gpu


def _engine():
    from hmmufotu_amd import engine as E
    if E.device_count() < 1:
        pytest.fail("no gfx950 device: GPU tests must run on the MI355X box (no CPU fallback exists)")
    return E


@pytest.mark.parametrize("name", TB.CASE_IDS)
def test_tree_bits(name):
    E = _engine()
    with np.load(TB.golden_path(name)) as z:
        want = {k: z[k] for k in z.files}
    got = TB.run_case(E, name, host=False)
    # the archive reaches what the case is there for
    assert TB.reaches(name, want) is None
    # every field as integers
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert np.issubdtype(want[key].dtype, np.integer), key
        bad = np.flatnonzero(got[key] != want[key])
        assert bad.size == 0, (key, bad[:8], got[key].reshape(-1)[bad[:8]], want[key].reshape(-1)[bad[:8]])
