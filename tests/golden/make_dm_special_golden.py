"""Writes tests/golden/dm_special.npz: lgamma and digamma at the points tests/test_train_dm.py pins its numpy restatements and the
training kernel's special functions to, evaluated with mpmath at 50 digits and rounded once to double.  The 50-digit context is the
one of make_hiprec_golden.py, the project's one importer of mpmath (tests/test_hiprec_oracle.py keeps it the only one).

Points: 181 log-spaced from 1e-5 to 1e4 (20 per decade), and 41 around digamma's positive root 1.4616321449683623, from 2^-40 to
2^-1 away on either side and the nearest double to the root itself.  Run: python tests/golden/make_dm_special_golden.py"""
import os

import numpy as np

from make_hiprec_golden import mp, mpf

assert mp.dps == 50
ROOT = 1.4616321449683623
x = np.concatenate([np.logspace(-5, 4, 181), [ROOT], ROOT + 2.0 ** -np.arange(1, 41, 2), ROOT - 2.0 ** -np.arange(1, 41, 2)])
x = np.unique(x.astype(np.float64))
lg = np.array([float(mp.loggamma(mpf(float(v)))) for v in x])
dg = np.array([float(mp.digamma(mpf(float(v)))) for v in x])
np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dm_special.npz"), x=x, lgamma=lg, digamma=dg)
print("%d points, lgamma in [%g, %g], digamma in [%g, %g]" % (len(x), lg.min(), lg.max(), dg.min(), dg.max()))
