"""BDF2 beside backward Euler on the device (dotmi_set_time_integration, include/dotmi.h; dot_amd/csrc/time_integration.hpp, k_timeint.hip).

Two references:
  - tests/bdf2_reference.py: BDF2 restated through the unchanged CPU oracle (one backward-Euler oracle per effective step).  Steps must
    agree in (status, iterations, halvings), and x, v and the next step's x~ to 1e-9, the project's band.
  - a SECOND HANDLE on backward Euler at dt_e, given dotmi_set_state(x^, v^, NULL) -- x^, v^ formed in numpy by the header's expression --
    the fixed vertices put back to their positions and dotmi_refactor(x_n): its step must be numpy.array_equal in positions to the BDF2
    handle's.  That is the definition of the feature: every loop, factor, coarse term and collective sees only dt_e.
Shapes: the 8 x 2 x 2 hanging bar of the accuracy study (81 vertices, two subdomains, one patch), synbar:16x5x5:4 (about ten element
patches, several vertex patches, both ends scripted), bunny5K / 8 (fixed-corotational, scripted)."""
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd import scene
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from tests import bdf2_reference as B
from tests import oracle_py as O
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR, SYNBAR, BUNNY = "bar:8x2x2:2", "synbar:16x5x5:4", "bunny5K_LTSS"


def load(name, dt=None):
    """-> (scene, epart, nparts, rel_tol)"""
    if name == BAR:
        V, T, fixed, epart = B.bar()
        cfg = scene.Config(energy="SNH", size=1.0, duration=B.BAR_T, dt=B.BAR_T / 48, rho=1.0, YM=2e4, PR=0.4, script="null")
        scr = scene.AnimScripter("null", V, scene.find_border_verts(V, cfg.handle_ratio))
        scr.fixed = fixed.copy()
        sc, ep, n, tol = scene.Scene(cfg=cfg, V_rest=V, T=np.ascontiguousarray(T, dtype=np.int32), scripter=scr, x0=V.copy()), epart, 2, 1e-9
    else:
        sc, ep, n = load_workload(name)
        tol = 1e-5
    if dt is not None:
        sc.cfg.dt = dt
    return sc, ep, n, tol


def script_move(sc, x, dt):
    if sc.cfg.script == "null":
        return np.zeros(0, dtype=np.int32), np.zeros((0, 3))
    return sc.scripter.step(x, dt)


def gravity(sc):
    return np.array([0.0, -9.80665 if sc.cfg.with_gravity else 0.0, 0.0])


def restated(sc, ep, n, tol, step="step", alpha_min=None, bdf2=True):
    cfg = sc.cfg

    def make(dt):
        o = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity, rel_tol=tol)
        if alpha_min is not None:
            o.set_alpha_min(alpha_min)
        return o
    return B.Restated(make, sc.x0, sc.fixed, cfg.dt, gravity=gravity(sc), step=step, bdf2=bdf2)


def same_counts(st, so):
    return (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings)


def step_both(sc, ts, r, k, dt=None):
    """script move, one step of the handle and of the restatement; the standing comparison"""
    dt = sc.cfg.dt if dt is None else dt
    idx, pos = script_move(sc, ts.getResult(), dt)
    if idx.size:
        ts.setDirichlet(idx, pos)
    kind, levels, dte, dtp = ts.timeIntegrationInfo()
    assert kind == dl.TIT_BDF2 and levels == r.levels and dte == r.plan()[3], (k, kind, levels, dte, r.plan())
    assert dtp == (r.dt_prev if r.levels else 0.0)
    assert ts.targetGRes > 0
    st, so = ts.step(), r.step((idx, pos))
    x, v, xt = ts.getState()
    ex, ev, ext = (float(np.abs(a - b).max()) for a, b in ((x, r.x), (v, r.v), (xt, r.predictor()[2])))
    print(f"step {k}: dt_e {dte:.6g} device {(st.status, st.iters, st.ls_halvings)} restated {(so.status, so.iters, so.ls_halvings)} "
          f"max|dx| {ex:.2e} max|dv| {ev:.2e} max|dx~| {ext:.2e}")
    assert same_counts(st, so), k
    assert st.status == 0
    assert ex < 1e-9 and ev < 1e-9 and ext < 1e-9, (k, ex, ev, ext)
    kind, levels, dte, dtp = ts.timeIntegrationInfo()
    assert levels == 1 and dtp == dt and dte == B.coefficients(dt, dt, 1)[3]
    return st


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, dl.FLAG_HOST_LOOP], ids=["device-loop", "host-loop"])
@pytest.mark.parametrize("name", [BAR, SYNBAR, BUNNY])
def test_six_steps_match_the_restatement(name, flags):
    """(SYNBAR and BUNNY have scripted moving ends: the restatement moves them after its set_state)"""
    sc, ep, n, tol = load(name)
    ts = DOTTimeStepper(sc, ep, n, flags=flags, rel_tol=tol)
    r = restated(sc, ep, n, tol)
    try:
        assert ts.timeIntegration() == dl.TIT_BE
        ts.setTimeIntegration(dl.TIT_BDF2)
        assert ts.timeIntegration() == dl.TIT_BDF2
        for k in range(6):
            step_both(sc, ts, r, k)
    finally:
        ts.close()
        r.close()


def test_newton_steps_match_the_restatement():
    sc, _, _, tol = load("synbar:16x5x5:1")
    ep = np.zeros(sc.T.shape[0], dtype=np.int32)
    ts = DOTTimeStepper(sc, ep, 1, flags=dl.FLAG_NEWTON)
    r = restated(sc, ep, 1, tol, step="step_newton")
    try:
        ts.setTimeIntegration(dl.TIT_BDF2)
        for k in range(6):
            step_both(sc, ts, r, k)
    finally:
        ts.close()
        r.close()


def test_gsdd_steps_match_the_restatement():
    sc, ep, n, tol = load("synbar:12x4x4:6")
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_GSDD)
    r = restated(sc, ep, n, tol, step="step_gsdd")
    try:
        ts.setTimeIntegration(dl.TIT_BDF2)
        for k in range(6):
            step_both(sc, ts, r, k)
    finally:
        ts.close()
        r.close()


# ---- 2. bit identity with a backward-Euler handle at dt_e, per stepper and form ------------------------------------------------------
def whole(flag):
    return dict(ep=None, n=1, kw=dict(alpha_min=1.0, flags=flag))


STEPPERS = {
    # id: (workload, environment, constructor arguments or None for the workload's own partition, flags, coarse mode, refactor the second handle)
    "dot": (SYNBAR, {}, None, 0, 0, True),
    "dot-bunny": (BUNNY, {}, None, 0, 0, True),
    "host-loop": (SYNBAR, {}, None, dl.FLAG_HOST_LOOP, 0, True),
    "vertex-patches": (SYNBAR, {"DOTMI_VERTEX_PATCHES": "1"}, None, 0, 0, True),
    "element-patches": (SYNBAR, {"DOTMI_VERTEX_PATCHES": "0"}, None, 0, 0, True),
    "lbfgs-pd": (SYNBAR, {}, whole(dl.FLAG_LBFGS_PD), 0, 0, False),   # (dotmi_refactor is refused on LBFGS-PD: L is built from dt alone)
    "lbfgs-hi": (SYNBAR, {}, whole(dl.FLAG_LBFGS_HI), 0, 0, True),
    "newton-pcg": (SYNBAR, {}, None, dl.FLAG_NEWTON_PCG, 0, True),
    "force-dist-replicated": (SYNBAR, {"DOTMI_SHARD_ELEMS": "0", "DOTMI_SHARD_HESS": "0"}, None, dl.FLAG_FORCE_DIST, 0, True),
    "force-dist-sharded": (SYNBAR, {"DOTMI_SHARD_ELEMS": "1", "DOTMI_SHARD_HESS": "1"}, None, dl.FLAG_FORCE_DIST, 0, True),
    "owner-exchange": (SYNBAR, {}, None, dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE, 0, True),
    "async-refresh": (SYNBAR, {}, None, dl.FLAG_ASYNC_REFRESH, 0, True),   # (the update stays queued behind the refresh)
    "dot-coarse-1": (SYNBAR, {}, None, 0, 1, True),
    "dot-coarse-2": (SYNBAR, {}, None, 0, 2, True),
}


def make_handle(sc, ep, n, args, flags, coarse):
    if args is None:
        ts = DOTTimeStepper(sc, ep, n, flags=flags)
    else:
        ts = DOTTimeStepper(sc, args["ep"], args["n"], **args["kw"])
    if coarse:
        ts.setDotCoarseMode(coarse)
    return ts


@pytest.mark.parametrize("case", list(STEPPERS), ids=list(STEPPERS))
def test_step_four_is_the_backward_euler_step_at_the_effective_step(case, monkeypatch):
    name, env, args, flags, coarse, refactor = STEPPERS[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, ep, n, _ = load(name)
    dt = sc.cfg.dt
    a = make_handle(sc, ep, n, args, flags, coarse)
    b = None
    try:
        a.setTimeIntegration(dl.TIT_BDF2)
        for k in range(3):
            idx, pos = script_move(sc, a.getResult(), dt)
            a.setDirichlet(idx, pos)
            assert a.step().status == 0
        x_n, v_n, xt_a = a.getState()
        x_p, v_p, dt_p = a.getHistory()
        _, levels, dte, _ = a.timeIntegrationInfo()
        c0, c1, _, dte_np = B.coefficients(dt, dt_p, 1)
        assert levels == 1 and dt_p == dt and dte == dte_np
        xh, vh = B.hat(c0, c1, x_n, x_p), B.hat(c0, c1, v_n, v_p)
        assert np.array_equal(xt_a, B.x_tilde(sc.fixed, x_n, xh, vh, dte, gravity(sc)))   # (the header's expression, in numpy)
        # the backward-Euler handle at dt_e
        sc_b, _, _, _ = load(name, dt=dte)
        b = make_handle(sc_b, ep, n, args, flags, coarse)
        b.setState(xh, vh)
        fx = np.flatnonzero(sc.fixed).astype(np.int32)
        b.setDirichlet(fx, x_n[fx])                     # (set_state put the fixed vertices at x^)
        if refactor:
            b.updatePrecondMtrAndFactorize(x_n)
        assert b.timeIntegration() == dl.TIT_BE and b.targetGRes == a.targetGRes
        idx, pos = script_move(sc, x_n, dt)
        a.setDirichlet(idx, pos)
        b.setDirichlet(idx, pos)
        sa, sb = a.step(), b.step()
        xa, xb = a.getResult(), b.getResult()
        print(f"{case}: BDF2 {(sa.status, sa.iters, sa.ls_halvings)} backward Euler at dt_e {(sb.status, sb.iters, sb.ls_halvings)} "
              f"max|dx| {np.abs(xa - xb).max():.2e}")
        assert same_counts(sa, sb) and sa.status == 0
        assert np.array_equal(xa, xb)
        # and the update: v+ = (x+ - x^) / dt_e on every vertex, as the backward-Euler handle forms it from x_n = x^
        assert np.array_equal(a.getState()[1], (xa - xh) / dte)
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- 3. live changes ---------------------------------------------------------------------------------------------------------------
def test_set_time_step_is_the_variable_step_rule():
    """dt changes after two steps (w = 1/2), and again after two more (w = 3): BDF2 steps with the coefficients of w, not start steps"""
    sc, ep, n, tol = load(SYNBAR)
    ts = DOTTimeStepper(sc, ep, n)
    r = restated(sc, ep, n, tol)
    try:
        ts.setTimeIntegration(dl.TIT_BDF2)
        dt = sc.cfg.dt
        k = 0
        for dt_k in (dt, dt, dt / 2, dt / 2, 1.5 * dt, 1.5 * dt):
            if dt_k != r.dt:
                ts.setTime(sc.cfg.duration, dt_k)
                r.set_dt(dt_k)
                _, levels, dte, dtp = ts.timeIntegrationInfo()
                assert levels == 1 and dte == B.coefficients(dt_k, dtp, 1)[3] and dtp != dt_k
                assert np.abs(ts.getState()[2] - r.predictor()[2]).max() < 1e-9
            step_both(sc, ts, r, k, dt=dt_k)
            k += 1
    finally:
        ts.close()
        r.close()


def test_set_state_makes_the_next_step_a_start_step():
    sc, ep, n, tol = load(SYNBAR)
    ts = DOTTimeStepper(sc, ep, n)
    r = restated(sc, ep, n, tol)
    try:
        ts.setTimeIntegration(dl.TIT_BDF2)
        for k in range(2):
            step_both(sc, ts, r, k)
        x, v, _ = ts.getState()
        ts.setState(x, v)
        r.restart(x, v)
        kind, levels, dte, dtp = ts.timeIntegrationInfo()
        assert (kind, levels, dte, dtp) == (dl.TIT_BDF2, 0, sc.cfg.dt, 0.0)
        assert ts.getHistory() is None
        for k in range(2, 4):
            step_both(sc, ts, r, k)
    finally:
        ts.close()
        r.close()


@pytest.mark.parametrize("flags", [0, dl.FLAG_HOST_LOOP], ids=["device-loop", "host-loop"])
def test_restart_with_history_continues_the_run(flags):
    """get_state + get_history after four steps into a fresh handle: its next two steps are the uninterrupted run's, bit for bit"""
    sc, ep, n, _ = load(SYNBAR)
    dt = sc.cfg.dt
    a = DOTTimeStepper(sc, ep, n, flags=flags)
    b = None
    try:
        a.setTimeIntegration(dl.TIT_BDF2)
        for k in range(4):
            idx, pos = script_move(sc, a.getResult(), dt)
            a.setDirichlet(idx, pos)
            assert a.step().status == 0
        x, v, xt = a.getState()
        hist = a.getHistory()
        sc_b, _, _, _ = load(SYNBAR)
        b = DOTTimeStepper(sc_b, ep, n, flags=flags)
        b.setTimeIntegration(dl.TIT_BDF2)
        b.setState(x, v)
        assert b.timeIntegrationInfo()[1] == 0
        b.setHistory(*hist)
        assert b.timeIntegrationInfo() == a.timeIntegrationInfo()
        assert np.array_equal(b.getState()[2], xt)
        for k in range(2):
            idx, pos = script_move(sc, a.getResult(), dt)
            a.setDirichlet(idx, pos)
            b.setDirichlet(idx, pos)
            sa, sb = a.step(), b.step()
            assert same_counts(sa, sb) and sa.status == 0
            for u, w in zip(a.getState(), b.getState()):
                assert np.array_equal(u, w), k
    finally:
        a.close()
        if b is not None:
            b.close()


def test_switching_bdf2_be_bdf2():
    """two BDF2 steps, two backward-Euler steps at dt, two BDF2 steps (the first a start step): each leg against the restatement"""
    sc, ep, n, tol = load(SYNBAR)
    ts = DOTTimeStepper(sc, ep, n)
    r = restated(sc, ep, n, tol)
    try:
        ts.setTimeIntegration(dl.TIT_BDF2)
        for k in range(2):
            step_both(sc, ts, r, k)
        ts.setTimeIntegration(dl.TIT_BE)
        assert ts.timeIntegrationInfo() == (dl.TIT_BE, 0, sc.cfg.dt, 0.0)
        x, v, xt = ts.getState()
        be = restated(sc, ep, n, tol, bdf2=False)
        be.restart(x, v)
        assert np.abs(xt - be.predictor()[2]).max() < 1e-9
        for k in range(2, 4):
            idx, pos = script_move(sc, ts.getResult(), sc.cfg.dt)
            ts.setDirichlet(idx, pos)
            st, so = ts.step(), be.step((idx, pos))
            assert same_counts(st, so) and st.status == 0
            assert np.abs(ts.getResult() - be.x).max() < 1e-9 and np.abs(ts.getState()[1] - be.v).max() < 1e-9
        be.close()
        ts.setTimeIntegration(dl.TIT_BDF2)
        r.restart(*ts.getState()[:2])
        for k in range(4, 6):
            step_both(sc, ts, r, k)
    finally:
        ts.close()
        r.close()


# ---- 4. backward Euler untouched -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [SYNBAR, BUNNY])
def test_setting_backward_euler_changes_nothing(name):
    sc, ep, n, _ = load(name)
    sc2, _, _, _ = load(name)
    a, b = DOTTimeStepper(sc, ep, n), DOTTimeStepper(sc2, ep, n)
    try:
        b.setTimeIntegration(dl.TIT_BE)
        for k in range(4):
            idx, pos = script_move(sc, a.getResult(), sc.cfg.dt)
            a.setDirichlet(idx, pos)
            b.setDirichlet(idx, pos)
            if k == 2:
                b.setTimeIntegration(dl.TIT_BE)
            sa, sb = a.step(), b.step()
            assert same_counts(sa, sb)
            for u, w in zip(a.getState(), b.getState()):
                assert np.array_equal(u, w), k
        assert b.timeIntegrationInfo() == (dl.TIT_BE, 0, sc.cfg.dt, 0.0) and b.getHistory() is None
    finally:
        a.close()
        b.close()


# ---- 5. accuracy on the device ---------------------------------------------------------------------------------------------------------
def test_bdf2_is_more_accurate_on_the_device():
    """the 48-step bar run of tests/test_bdf2_reference.py on the device, against the recorded CPU-restated fine run (BDF2, 1536 steps):
    BDF2's error is at most a fifth of backward Euler's (CPU: 2.35e-3 against 2.38e-2)"""
    fine = B.load_golden()
    e = {}
    for kind in (dl.TIT_BE, dl.TIT_BDF2):
        sc, ep, n, tol = load(BAR)
        ts = DOTTimeStepper(sc, ep, n, rel_tol=tol)
        try:
            ts.setTimeIntegration(kind)
            for _ in range(48):
                assert ts.step().status == 0
            e[kind] = float(np.abs(ts.getResult() - fine).max())
        finally:
            ts.close()
    print(f"48 steps on the device: backward Euler {e[dl.TIT_BE]:.3e}  BDF2 {e[dl.TIT_BDF2]:.3e}")
    assert e[dl.TIT_BDF2] <= e[dl.TIT_BE] / 5


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sc, ep, n, _ = load(BAR)
    ts = DOTTimeStepper(sc, ep, n)
    L, h = ts._L, ts._h
    try:
        x, v, xt = ts.getState()
        for bad in (2, -1, 7):
            with pytest.raises(DotmiError, match=r"failed \(-1\)"):
                ts.setTimeIntegration(bad)
        assert ts.timeIntegration() == dl.TIT_BE
        with pytest.raises(DotmiError, match="backward Euler keeps no level"):
            ts.setHistory(x, v, sc.cfg.dt)
        ts.setTimeIntegration(dl.TIT_BDF2)
        for bad in (0.0, -0.01, float("nan"), float("inf")):
            with pytest.raises(DotmiError, match="dt_prev must be positive and finite"):
                ts.setHistory(x, v, bad)
        assert L.dotmi_set_history(h, None, dl.dp(v), 0.01) == -1 and L.dotmi_set_history(h, dl.dp(x), None, 0.01) == -1
        assert L.dotmi_time_integration_info(h, None, None, None, None) == 0     # (any output may be NULL)
        assert L.dotmi_get_history(h, None, None, None) == 0                      # (no level yet)
        # nothing of this changed the handle
        assert ts.timeIntegrationInfo() == (dl.TIT_BDF2, 0, sc.cfg.dt, 0.0)
        assert all(np.array_equal(u, w) for u, w in zip(ts.getState(), (x, v, xt)))
    finally:
        ts.close()


def test_config_bdf2_switches_the_stepper():
    sc, ep, n, _ = load(BAR)
    sc.cfg.bdf2 = True
    ts = DOTTimeStepper(sc, ep, n)
    try:
        assert ts.timeIntegration() == dl.TIT_BDF2
        assert ts.solve(2) == 0 and ts.timeIntegrationInfo()[1] == 1
    finally:
        ts.close()


# ---- 7. the runner ---------------------------------------------------------------------------------------------------------------------
def test_headless_runner_takes_bdf2(tmp_path):
    """dot_hip --bdf2 on a small script: steps; frame 0 is the backward-Euler start step, bit for bit the plain run's; the next frames are
    not; config.txt is the plain run's (the reference's token lookup knows only BE: the option stands beside the script)"""
    from tests.test_host_logic import _write_msh
    exe = os.path.join(ROOT, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dot_amd", "host")])
    V, T = scene.synthetic_bar(8, 3, 3)
    _write_msh(tmp_path / "bar.msh", V, T)
    (tmp_path / "bar.txt").write_text("energy SNH\ntimeStepper DOT 4\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\nstiffness 100000 0.4\n"
                                      "script stretch\nshape input bar.msh\n")
    E, cfg = {}, {}
    for tag, extra in (("be", []), ("bdf2", ["--bdf2"])):
        res = subprocess.run([exe, "100", str(tmp_path / "bar.txt"), "--mesh-root", str(tmp_path), "--frames", "3", "--out",
                              str(tmp_path / tag)] + extra, capture_output=True, timeout=300)
        assert res.returncode == 0, res.stderr.decode()
        frames = [l.split() for l in res.stdout.decode().splitlines() if l.startswith("FRAME")]
        assert len(frames) == 3 and all(f[-1] == "0" for f in frames)
        E[tag] = [f[f.index("E") + 1] for f in frames]
        cfg[tag] = (tmp_path / tag / "config.txt").read_text()
        assert (b"time integration: BDF2" in res.stdout) == bool(extra)
        assert (tmp_path / tag / "status2").exists()
    assert E["bdf2"][0] == E["be"][0] and E["bdf2"][1] != E["be"][1] and E["bdf2"][2] != E["be"][2]
    assert cfg["bdf2"] == cfg["be"] and "BDF2" not in cfg["be"].upper()
