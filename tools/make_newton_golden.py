"""tests/golden/newton_bunny5K.npz: the oracle's exact one-subdomain Newton (dor_step_newton) on bunny5K_LTSS, two scripted steps --
per step (status, iterations, halvings) and the positions.  About a minute of CPU per step, hence a fixture (tests/test_gpu_newton_pcg.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from dot_amd.workloads import load_workload  # noqa: E402
from tests import oracle_py as O  # noqa: E402

sc, _, _ = load_workload("bunny5K_LTSS")
cfg = sc.cfg
orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0,
                  np.zeros(sc.T.shape[0], dtype=np.int32), 1, cfg.with_gravity)
stats, xs = [], []
for k in range(2):
    idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
    orc.move(idx, pos)
    so = orc.step_newton()
    stats.append((so.status, so.iters, so.ls_halvings))
    xs.append(orc.state()[0].copy())
    print(k, stats[-1])
out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "newton_bunny5K.npz")
np.savez_compressed(out, stats=np.array(stats, dtype=np.int32), x=np.array(xs))
print(out, os.path.getsize(out))
