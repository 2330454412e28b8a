"""A start state from which one DOT step accepts trials whose pair is not stored (y . s <= 0: DOTTimeStepper.cpp:474-494,
dot_amd/csrc/lbfgs_history.hpp): synbar:12x2x2:4 -- 117 vertices, 288 tets, 18 fixed vertices, four subdomains of 72 tets, Stable
Neo-Hookean, dt = 0.025, gravity -- compressed to 0.4 of its length along its long axis about the mean, every vertex, the fixed ones
included, then 0.01 x Gaussian noise on the free vertices; zero velocity, x_n = x, the factors those of the rest state (a handle or an
oracle created at x0 that gets set_state(x, 0, x) and no refactor).  Capped at 48 iterations the oracle's step accepts six trials
in a row with y . s < 0, iterations 30 to 35, with the window of five pairs full (tests/test_no_pair_reference.py pins that).

The tests load the committed positions, tests/golden/buckled_bar_12x2x2.npz (written by tests/golden/make_buckled_bar.py), so that
they do not depend on numpy's generator stream; start_state() is how the file came about.  TEST INFRASTRUCTURE."""
import os

import numpy as np

from dot_amd.workloads import load_workload

MESH = "synbar:12x2x2:4"
SCALE, NOISE, SEED = 0.4, 0.01, 4
ITER_CAP = 48
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "buckled_bar_12x2x2.npz")
# the first normal deviate of default_rng(SEED) when the fixture was written: where numpy still draws it, start_state() is the fixture's bits
FIRST_DEVIATE = -0.6517911526116896


def start_state(x0, fixed):
    """the designed positions from the rest positions x0 (nV, 3) and the fixed flags (nV,)"""
    x = np.array(x0, dtype=np.float64)
    free = ~np.asarray(fixed, dtype=bool)
    ax = int(np.argmax(x.max(axis=0) - x.min(axis=0)))
    mean = x[:, ax].mean()
    x[:, ax] = mean + SCALE * (x[:, ax] - mean)
    x[free] += NOISE * np.random.default_rng(SEED).standard_normal((int(free.sum()), 3))
    return x


def load():
    """-> (scene, element partition, subdomains, the fixture's positions)"""
    sc, ep, n = load_workload(MESH)
    x = np.load(FIXTURE)["x"]
    assert x.shape == sc.x0.shape and x.dtype == np.float64
    return sc, ep, n, x


def cosine(s, y):
    """y . s / (|y| |s|)"""
    s, y = np.ravel(s), np.ravel(y)
    return float(s @ y) / (float(np.linalg.norm(s)) * float(np.linalg.norm(y)))


def exact_alpha(a, alpha_min=0.1):
    """a step length that is no estimate: 1 or the clamp alpha_min, or one of them halved (the line search's alpha /= 2 is exact)"""
    for top in (1.0, alpha_min):
        h = top
        for _ in range(1100):
            if a == h:
                return True
            if h < a:
                break
            h /= 2.0
    return False


def compare_logs(got, want, tag):
    """per-iteration logs (alpha, E, |g|^2) of a run against the reference run's: as many iterations; alpha equal where the reference's
    is 1, the clamp or one of them halved, within 1e-9 relative where it is an estimate; E within 1e-9 relative, |g|^2 within 1e-6
    (the bounds of tests/test_gpu_round2.py's teacher-forced steps).  Prints and returns the maxima (alpha, E, |g|^2)"""
    (a, e, g), (ar, er, gr) = got, want
    assert len(a) == len(ar) == len(e) == len(er) == len(g) == len(gr), (tag, len(a), len(ar))
    exact = np.array([exact_alpha(v) for v in ar], dtype=bool)
    da = float((np.abs(a - ar) / ar)[~exact].max()) if (~exact).any() else 0.0
    de = float((np.abs(e - er) / np.abs(er)).max())
    dg = float((np.abs(g - gr) / gr).max())
    print(f"{tag}: {int(exact.sum())} of {len(ar)} step lengths are 1, the clamp or halvings; estimates {da:.2e}, E {de:.2e}, |g|^2 {dg:.2e} relative")
    assert np.array_equal(a[exact], ar[exact]), (tag, np.flatnonzero(exact & (a != ar)) + 1)
    assert da <= 1e-9, (tag, da)
    assert de <= 1e-9, (tag, de)
    assert dg <= 1e-6, (tag, dg)
    return da, de, dg


def _oracle_at_the_state():
    from tests import oracle_py as O
    sc, ep, n, x = load()
    cfg = sc.cfg
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)
    orc.set_state(x, np.zeros_like(x), x)      # (no refactor: the factors stay those of x0)
    return sc, ep, n, orc


_runs = {}


def oracle_run():
    """the oracle's step from the state, stopped after ITER_CAP iterations (step_begin, ITER_CAP x step_iterate, step_end), once:
    -> dict(iters, halvings, x: the end positions, xs: the ITER_CAP + 1 iterates x_0 .. x_cap, gs: their gradients, m: pairs stored in
    front of every iteration, stored: per iteration whether the newest stored s is x_{k+1} - x_k afterwards, log: (alpha, E, |g|^2))"""
    if "oracle" not in _runs:
        sc, ep, n, orc = _oracle_at_the_state()
        try:
            orc.step_begin()
            x, g, S, _, _ = orc.lbfgs_state()
            xs, gs, m, stored = [x], [g], [], []
            for k in range(ITER_CAP):
                m.append(len(S))
                assert orc.step_iterate() == 0, k              # (neither converged nor failed before the cap)
                x, g, S, _, _ = orc.lbfgs_state()
                s = (x - xs[-1]).ravel()
                # s is stored as alpha p, x as x + alpha p: equal to the rounding of the sum; another pair's s is nowhere near
                stored.append(len(S) > 0 and bool(np.abs(S[-1] - s).max() <= 1e-9 * np.abs(s).max()))
                xs.append(x)
                gs.append(g)
            st = orc.step_end()
            _runs["oracle"] = dict(iters=st.iters, halvings=st.ls_halvings, x=orc.state()[0].copy(), xs=xs, gs=gs, m=m, stored=stored,
                                   log=orc.iter_log())
        finally:
            orc.close()
    return _runs["oracle"]


def restated_run(hist=5, coarse=False):
    """the numpy restatement's step (tests/dot_coarse_reference.DotStepper on an oracle's operators) from the state, capped alike, with
    `hist` pairs and without or with the rigid-mode coarse term (Z at the state's positions, A0 on the rest state's H -- what
    dotmi_set_dot_coarse builds when it is called after dotmi_set_state); once per case -> DotStepper.step's dict + x, active"""
    key = ("restated", hist, coarse)
    if key not in _runs:
        from tests import dot_coarse_reference as DR
        sc, ep, n, orc = _oracle_at_the_state()
        try:
            fixed = np.asarray(sc.fixed, dtype=bool)
            st = DR.DotStepper(orc, fixed, sc.cfg.dt, (0.0, -9.80665 if sc.cfg.with_gravity else 0.0, 0.0))
            M, active = None, False
            if coarse:
                M, active = DR.m_prime(orc, orc.dup(), [np.asarray(orc.part_verts(p)) for p in range(n)], fixed)
            r = st.step(M, hist=hist, iter_cap=ITER_CAP)
            r["x"], r["active"] = orc.state()[0].copy(), active
            _runs[key] = r
        finally:
            orc.close()
    return _runs[key]
