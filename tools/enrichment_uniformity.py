#!/usr/bin/env python3
"""How uniform is the keyed bijection sigma_p of csrc/enrichment.hip on small domains?  Host only (the numpy restatement of
tests/enrichment_numpy.py): chi-square of the position of cell 0 over 20 000 permutations, and of the positions of cells 0 and 1 jointly over
40 000, for a few n; and the longest cycle walk seen.  DESIGN.md section 14 quotes the output."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enrichment_numpy as EN  # noqa: E402

for n in (4, 5, 7, 16, 17, 25, 100):
    one, two = np.zeros(n), np.zeros((n, n))
    for p in range(40000):
        s = EN.sigma(n, 0, 0, p)
        if p < 20000:
            one[s[0]] += 1
        two[s[0], s[1]] += 1
    e1, e2 = 20000 / n, 40000 / (n * (n - 1))
    chi1 = ((one - e1) ** 2 / e1).sum()
    off = ~np.eye(n, dtype=bool)
    chi2 = ((two[off] - e2) ** 2 / e2).sum()
    d1, d2 = n - 1, n * (n - 1) - 1
    print(f"n = {n}: position of one cell chi2 {chi1:.0f} on {d1} dof ({(chi1 - d1) / np.sqrt(2 * d1):+.1f} sigma); "
          f"of two cells jointly chi2 {chi2:.0f} on {d2} dof ({(chi2 - d2) / np.sqrt(2 * d2):+.1f} sigma)")
for n in (257, 1000, 4097, 100000):
    print(f"n = {n}: longest walk over 4 permutations {max(EN.sigma(n, 0, 0, p, want_passes=True)[1] for p in range(4))} passes")
