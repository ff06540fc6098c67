"""Writes tests/golden/tree_gamma/rates.json: the category rates of the discrete Gamma of rates (Yang 1994) that hu_gamma_rates is held
to (tests/test_tree_gamma.py reads the file alone).  K equally probable categories of Gamma(shape alpha, rate alpha), each rate the
mean of its category: with q_i the i/K quantile of Gamma(shape alpha, scale 1) and P the regularised incomplete gamma function,
rate_i = K [P(alpha + 1, q_{i+1}) - P(alpha + 1, q_i)].  scipy's gammaincinv and gammainc; the last category through gammaincc, so that
no rate is a difference from 1.  Run from the repository root: python tests/golden/make_tree_gamma_golden.py"""
import json
import os

import numpy as np
from scipy.special import gammainc, gammaincc, gammaincinv

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tree_gamma", "rates.json")
rec = []
for k in (1, 2, 4, 8, 16):
    for alpha in (0.05, 0.3, 1.0, 7.0, 100.0):
        q = gammaincinv(alpha, np.arange(1, k) / k)
        p = np.concatenate([[0.0], gammainc(alpha + 1, q)])
        rates = np.concatenate([k * np.diff(p), [k * gammaincc(alpha + 1, q[-1]) if k > 1 else 1.0]])
        rec.append(dict(k=k, alpha=alpha, rates=[float(x) for x in rates]))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
print("%d records -> %s" % (len(rec), OUT))
