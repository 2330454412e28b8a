"""tests/golden/buckled_bar_12x2x2.npz: the start state of tests/buckled_bar.py, 117 x 3 positions.  Run
    python tests/golden/make_buckled_bar.py
and, when numpy's generator stream has moved, put the printed first deviate into tests/buckled_bar.FIRST_DEVIATE."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))
from dot_amd.workloads import load_workload  # noqa: E402
from tests import buckled_bar as B  # noqa: E402

sc, ep, n = load_workload(B.MESH)
x = B.start_state(sc.x0, sc.fixed)
np.savez(B.FIXTURE, x=x)
print(B.FIXTURE, x.shape, os.path.getsize(B.FIXTURE), "bytes; first deviate",
      repr(float(np.random.default_rng(B.SEED).standard_normal())))
