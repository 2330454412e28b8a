"""Variable-step BDF2 restated through the unchanged CPU oracle (tests/oracle_py.py), which knows backward Euler only.

With w = dt / dt_prev, gamma = (1 + w) / (1 + 2 w), c0 = (1 + w)^2 / (1 + 2 w), c1 = w^2 / (1 + 2 w) and
    x^ = c0 x_n - c1 x_{n-1},   v^ = c0 v_n - c1 v_{n-1},   dt_e = gamma dt
a BDF2 step minimises exactly the incremental potential a backward-Euler step of size dt_e minimises from (x^, v^).  So a step here is:
one OracleSim per distinct dt_e; refactor(x_n) (the device refreshes its factors at the end of the step before, at x_n and the new dt_e);
set_state(x^, v^, None); the fixed vertices back to their positions (set_state put them at x^) and the scripted ones moved; the oracle's
own step function -- `step`, `step_newton` or `step_gsdd`; v+ = (x+ - x^) / dt_e.  The first step, and the first one after `restart`, has
no level n-1 and is a backward-Euler step at dt.

The coefficient expressions are those of dot_amd/csrc/time_integration.hpp operation by operation, so `coefficients`, `hat` and
`x_tilde` agree with the library bit for bit (Python floats and numpy float64 do not contract)."""
from __future__ import annotations

import os

import numpy as np

from dot_amd.scene import synthetic_bar
from tests import oracle_py as O

GRAVITY = np.array([0.0, -9.80665, 0.0])


def coefficients(dt, dt_prev, levels=1):
    """(c0, c1, gamma, dt_e) -- tit_plan of time_integration.hpp"""
    if levels < 1:
        return 1.0, 0.0, 1.0, dt
    w = dt / dt_prev
    den = 1.0 + 2.0 * w
    c0 = 1.0 + (w * w) / den
    gamma = (1.0 + w) / den
    return c0, c0 - 1.0, gamma, gamma * dt


def closed_form(w):
    """(c0, c1, gamma) as the issue states them"""
    return (1 + w) ** 2 / (1 + 2 * w), w * w / (1 + 2 * w), (1 + w) / (1 + 2 * w)


def hat(c0, c1, a_n, a_nm1):
    return c0 * a_n - c1 * a_nm1


def x_tilde(fixed, x, xhat, vhat, dte, gravity):
    """x^ + (v^ dt_e + dt_e^2 g) on free vertices, x on fixed ones"""
    gd = (dte * dte) * np.asarray(gravity)
    xt = xhat + (vhat * dte + gd[None, :])
    fx = np.asarray(fixed).astype(bool)
    xt[fx] = x[fx]
    return xt


class Restated:
    """make_sim(dt) -> a fresh OracleSim of the scene at time step dt (its own initial state is overwritten before every step)"""

    def __init__(self, make_sim, x0, fixed, dt, gravity=GRAVITY, step="step", bdf2=True, v0=None):
        self.make_sim, self.step_name, self.bdf2 = make_sim, step, bdf2
        self.fixed = np.asarray(fixed).astype(bool)
        self.fixed_idx = np.flatnonzero(self.fixed).astype(np.int32)
        self.gravity = np.asarray(gravity, dtype=np.float64)
        self.dt = float(dt)
        self.sims = {}
        self.restart(x0, np.zeros_like(x0) if v0 is None else v0)

    def close(self):
        for s in self.sims.values():
            s.close()
        self.sims = {}

    def _sim(self, dte):
        if dte not in self.sims:
            self.sims[dte] = self.make_sim(dte)
        return self.sims[dte]

    def restart(self, x, v):
        """a state without level n-1: the next step is a start step"""
        self.x, self.v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
        self.x_prev = self.v_prev = None
        self.dt_prev = 0.0

    def set_history(self, x_prev, v_prev, dt_prev):
        self.x_prev, self.v_prev, self.dt_prev = np.array(x_prev), np.array(v_prev), float(dt_prev)

    def set_dt(self, dt):
        self.dt = float(dt)

    @property
    def levels(self):
        return 1 if (self.bdf2 and self.x_prev is not None) else 0

    def plan(self):
        return coefficients(self.dt, self.dt_prev, self.levels)

    def predictor(self):
        """(x^, v^, x~, dt_e) of the next step"""
        c0, c1, _, dte = self.plan()
        if self.levels:
            xh, vh = hat(c0, c1, self.x, self.x_prev), hat(c0, c1, self.v, self.v_prev)
        else:
            xh, vh = self.x.copy(), self.v.copy()
        return xh, vh, x_tilde(self.fixed, self.x, xh, vh, dte, self.gravity), dte

    def step(self, move=None):
        """move: (idx, pos) of the scripted vertices for this step -> the oracle's statistics"""
        xh, vh, _, dte = self.predictor()
        sim = self._sim(dte)
        sim.refactor(self.x)
        sim.set_state(xh, vh, None)
        if self.fixed_idx.size:
            sim.move(self.fixed_idx, self.x[self.fixed_idx])
        if move is not None and len(move[0]):
            sim.move(move[0], move[1])
        st = getattr(sim, self.step_name)()
        xp = sim.state()[0]
        vp = (xp - xh) / dte
        if self.bdf2:
            self.x_prev, self.v_prev, self.dt_prev = self.x, self.v, self.dt
        self.x, self.v = xp, vp
        return st


# ---- the bar of the accuracy study: synthetic_bar(8, 2, 2) hanging from x = 0 under gravity -------------------------------------------
BAR_T = 0.48


def bar():
    """(V, T, fixed, epart): Stable Neo-Hookean, YM 2e4, PR 0.4, rho 1, two subdomains split by the element centroid at x = 2"""
    V, T = synthetic_bar(8, 2, 2)
    fixed = (V[:, 0] == 0.0).astype(np.uint8)
    epart = (V[T].mean(axis=1)[:, 0] >= 2.0).astype(np.int32)
    return V, T, fixed, epart


def bar_sim_factory(rel_tol=1e-9):
    V, T, fixed, epart = bar()
    return lambda dt: O.OracleSim(V, T, 2e4, 0.4, 1.0, 1, dt, fixed, V, epart, 2, True, rel_tol=rel_tol)


def run_bar(dts, bdf2=True, step="step", keep=False):
    """the bar from rest over the step sizes dts -> x at the end (keep: the list of (x, v) after every step)"""
    V, _, fixed, _ = bar()
    r = Restated(bar_sim_factory(), V, fixed, dts[0], bdf2=bdf2, step=step)
    out = []
    try:
        for dt in dts:
            r.set_dt(dt)
            r.step()
            if keep:
                out.append((r.x.copy(), r.v.copy()))
    finally:
        r.close()
    return out if keep else r.x


# ---- the fine solution, recorded: the device's accuracy test reads it instead of running 1536 oracle steps on the GPU machine ---------
FINE_STEPS = 1536
FINE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bdf2_bar_fine.npz")


def write_golden():
    """python -c "from tests import bdf2_reference as B; B.write_golden()" -- tests/test_bdf2_reference.py checks the file against a fresh run"""
    x = run_bar([BAR_T / FINE_STEPS] * FINE_STEPS)
    np.savez(FINE_PATH, x=x, steps=FINE_STEPS, T=BAR_T)


def load_golden():
    with np.load(FINE_PATH) as f:
        assert int(f["steps"]) == FINE_STEPS and float(f["T"]) == BAR_T
        return f["x"].copy()
