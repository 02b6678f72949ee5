#!/usr/bin/env python3
"""Regenerates multiplexed-image-annotator_amd/diverging_u8.csv: matplotlib's 256-entry RdBu_r table, components truncated to int(c * 255) as
tools/make_viridis_table.py does, written as text (one "r,g,b" line per entry) so that the package ships no new binary file.  It stands in for seaborn's 'vlag' of the reference's heat maps (model.py:720), which neither matplotlib nor
the reference carries; replacing the file changes the colours of Annotator.generate_heatmap and nothing else."""
import os

import matplotlib
import numpy as np

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

cmap = plt.get_cmap("RdBu_r")
lut = np.array([[int(c * 255) for c in cmap(i)[:3]] for i in range(256)], np.uint8)
np.savetxt(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multiplexed-image-annotator_amd", "diverging_u8.csv"), lut, fmt="%d",
           delimiter=",")
print(lut.shape, lut[0], lut[127], lut[-1])
