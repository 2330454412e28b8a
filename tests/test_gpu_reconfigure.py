"""Tolerance, time step and materials changed on a live handle (dotmi_set_rel_tol, dotmi_set_time_step, dotmi_set_lame; include/dotmi.h).

The definition every test here stands on: after a setter the handle is the one dotmi_create would have built from the new value,
brought to the same state with dotmi_set_state(x, v) and dotmi_refactor(h, NULL).  So the references are
  - a FRESH handle: built with the new value, setState(x, v) of the live handle taken right after a step (x_n == x), refactor at x.
    What is a deterministic function of (inputs, state) -- tolerance, x~, energy, gradient, element Hessians, a subdomain matrix, one
    application of the preconditioner -- must be EQUAL (numpy.array_equal): anything less means a slot, a copy of a patch table or a
    cached value kept the old material or time step;
  - the CPU oracle (dor_set_lame on the running oracle; a fresh oracle for a new tolerance or time step, which it cannot change at
    run time) for steps, under the standing bounds of tests/test_gpu_materials.py::_steps_against_oracle: identical
    (status, iters, ls_halvings), status 0, g2 <= targetGRes, max|dx| < 1e-9.
Shapes: synbar:8x3x3:4 (432 tets: two 256-element patches, one padded), synbar:16x5x5:4 (2400 tets: about ten patches, several vertex
patches, elements carried twice), bunny5K_LTSS (fixed-corotational forms), and one bar17K_twist case for the 512-element patch set of a
speculating step, which smaller meshes do not build."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd import scene
from dot_amd.scene import lame
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from tests import oracle_py as O
from tests.materials import field
from tests.test_gpu_materials import FORMS as MATERIAL_FORMS
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = [("synbar:16x5x5:4", "SNH"), ("bunny5K_LTSS", "FCR")]
# the forms of the element pass (tests/test_gpu_materials.py::FORMS): default, element patches, vertex patches forced, host loop,
# sharded; and a speculating step, whose patch set is the default one's tables on these meshes
FORMS = [f for f in MATERIAL_FORMS if f[0] in ("default", "element-patches", "vertex-patches", "spec-step", "host-loop", "sharded")]


def load(name, energy=None, dt=None):
    sc, ep, n = load_workload(name)
    if energy is not None:
        sc.cfg.energy = energy
    if dt is not None:
        sc.cfg.dt = dt
    return sc, ep, n


def uniform(sc):
    mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
    nT = sc.T.shape[0]
    return np.full(nT, mu0), np.full(nT, lam0)


def oracle(sc, ep, n, dt=None, rel_tol=1e-5, mu=None, lam=None):
    cfg = sc.cfg
    return O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt if dt is None else dt, sc.fixed, sc.x0, ep, n,
                       cfg.with_gravity, rel_tol=rel_tol, mu=mu, lam=lam)


def step_once(sc, ts, orc=None, dt=None, oracle_step="step"):
    """script move + one step on the handle (and the oracle) -> their statistics"""
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt if dt is None else dt)
    ts.setDirichlet(idx, pos)
    if orc is None:
        return ts.step(), None
    orc.move(idx, pos)
    return ts.step(), getattr(orc, oracle_step)()


def steps_against_oracle(sc, ts, orc, nsteps, dt=None, oracle_step="step"):
    """the standing bounds (tests/test_gpu_materials.py::_steps_against_oracle) -> the iteration counts"""
    iters = []
    for k in range(nsteps):
        st, so = step_once(sc, ts, orc, dt, oracle_step)
        dx = np.abs(ts.getResult() - orc.state()[0]).max()
        print(f"step {k}: device {(st.status, st.iters, st.ls_halvings)} oracle {(so.status, so.iters, so.ls_halvings)} "
              f"g2 {st.g2:.3e} target {ts.targetGRes:.3e} max|dx| {dx:.2e}")
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert dx < 1e-9, (k, dx)
        iters.append(st.iters)
    return iters


def bring_to_state(fresh, ts):
    """the fresh handle at the live one's state: set_state(x, v) right after a step, refactor at x"""
    x, v, _ = ts.getState()
    fresh.setState(x, v)
    if not fresh._pd:
        fresh.updatePrecondMtrAndFactorize()
    return x, v


def quantities(ts, sc):
    """what is a deterministic function of the handle's inputs and state"""
    rng = np.random.default_rng(5)
    x = ts.getResult() + 1e-3 * rng.standard_normal(sc.x0.shape)
    r = rng.standard_normal(sc.x0.shape)
    r[sc.fixed.astype(bool)] = 0
    q = {"targetGRes": np.float64(ts.targetGRes), "x_tilde": ts.getState()[2], "E": np.float64(ts.computeEnergyVal(x)),
         "g": ts.computeGradient(x), "H": ts.computeElemHessians(x), "precond": ts.applyPrecond(r)}
    if not ts._pd:
        q["part0"], q["l2g"] = ts.partMatrix(0)
    return q


def assert_same_handle(ts, fresh, sc):
    a, b = quantities(ts, sc), quantities(fresh, sc)
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()))


def make(sc, ep, n, flags=0, pd=False, **kw):
    if pd:
        ts = DOTTimeStepper(sc, None, 1, alpha_min=1.0, flags=dl.FLAG_LBFGS_PD | flags, **kw)
    else:
        ts = DOTTimeStepper(sc, ep, n, flags=flags, **kw)
    ts._pd = pd
    return ts


# ---- 1. set_lame: the handle is the fresh handle ------------------------------------------------------------------------------
def _set_lame_against_fresh(name, energy, flags=0, pd=False):
    sc, ep, n = load(name, energy)
    ts = make(sc, ep, n, flags, pd)
    fresh = None
    try:
        st, _ = step_once(sc, ts)
        assert st.status == 0
        mu, lam = field(sc, "random")
        ts.setLame(mu, lam)
        sc2, _, _ = load(name, energy)
        fresh = make(sc2, ep, n, flags, pd, mu=mu, lam=lam)
        bring_to_state(fresh, ts)
        assert_same_handle(ts, fresh, sc)
        # the forms the step itself runs (this rank's own patches, vertex patches, a speculating step's set): one step of both,
        # two runs of the same iteration, under the standing bounds
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        fresh.setDirichlet(idx, pos)
        sa, sb = ts.step(), fresh.step()
        assert (sa.status, sa.iters, sa.ls_halvings) == (sb.status, sb.iters, sb.ls_halvings)
        assert sa.status == 0 and sa.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - fresh.getResult()).max() < 1e-9
    finally:
        ts.close()
        if fresh is not None:
            fresh.close()


@pytest.mark.parametrize("name,energy", WORKLOADS, ids=[w[0] for w in WORKLOADS])
@pytest.mark.parametrize("form,env,flags", FORMS, ids=[f[0] for f in FORMS])
def test_set_lame_gives_the_fresh_handle(form, env, flags, name, energy, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _set_lame_against_fresh(name, energy, flags)


def test_set_lame_gives_the_fresh_handle_lbfgs_pd():
    _set_lame_against_fresh("synbar:16x5x5:4", "SNH", pd=True)


def test_set_lame_gives_the_fresh_handle_gsdd():
    _set_lame_against_fresh("bunny5K_LTSS", "FCR", flags=dl.FLAG_GSDD)


def test_set_lame_reaches_the_512_element_patches_of_a_speculating_step(monkeypatch):
    """bar17K_twist with DOTMI_SPEC_STEP=1: the only workload of the suite whose speculating step gets a patch set of its own"""
    monkeypatch.setenv("DOTMI_SPEC_STEP", "1")
    _set_lame_against_fresh("bar17K_twist", None)


# ---- 2. set_lame: steps against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,energy", WORKLOADS, ids=[w[0] for w in WORKLOADS])
@pytest.mark.parametrize("kind", ["random", "one-off", "one-off-first"])
def test_set_lame_steps_match_oracle(name, energy, kind):
    """one-off is the LAST element (a padded patch's last used slot), one-off-first element 0 (the tolerance's element)"""
    sc, ep, n = load(name, energy)
    ts, orc = make(sc, ep, n), oracle(sc, ep, n)
    try:
        steps_against_oracle(sc, ts, orc, 2)
        mu, lam = field(sc, kind, 4)
        ts.setLame(mu, lam)
        orc.set_lame(mu, lam)
        assert abs(ts.targetGRes - orc.target_gres) <= 1e-15 * orc.target_gres
        steps_against_oracle(sc, ts, orc, 2)
    finally:
        ts.close(); orc.close()


# ---- 3. back to one material; a second field ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,energy", [("synbar:8x3x3:4", "SNH")] + WORKLOADS, ids=["synbar:8x3x3:4"] + [w[0] for w in WORKLOADS])
def test_back_to_one_material_is_the_uniform_handle(name, energy):
    sc, ep, n = load(name, energy)
    ts = make(sc, ep, n)
    sc2, _, _ = load(name, energy)
    fresh = make(sc2, ep, n)
    try:
        assert step_once(sc, ts)[0].status == 0
        ts.setLame(*field(sc, "random"))
        ts.setLame(*uniform(sc))
        bring_to_state(fresh, ts)
        assert_same_handle(ts, fresh, sc)
    finally:
        ts.close(); fresh.close()


def test_a_second_field_reuses_the_slot_arrays():
    name, energy = "synbar:16x5x5:4", "SNH"
    sc, ep, n = load(name, energy)
    ts = make(sc, ep, n)
    fresh = None
    try:
        assert step_once(sc, ts)[0].status == 0
        ts.setLame(*field(sc, "random", 1))
        bytes1 = ts._L.dotmi_factor_storage_bytes(ts._h)
        mu, lam = field(sc, "random", 2)
        ts.setLame(mu, lam)
        assert ts._L.dotmi_factor_storage_bytes(ts._h) == bytes1
        sc2, _, _ = load(name, energy)
        fresh = make(sc2, ep, n, mu=mu, lam=lam)
        assert fresh._L.dotmi_factor_storage_bytes(fresh._h) == bytes1
        bring_to_state(fresh, ts)
        assert_same_handle(ts, fresh, sc)
    finally:
        ts.close()
        if fresh is not None:
            fresh.close()


# ---- 4. set_time_step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,energy", WORKLOADS, ids=[w[0] for w in WORKLOADS])
def test_set_time_step(name, energy):
    sc, ep, n = load(name, energy)
    ts = make(sc, ep, n)
    fresh = orc = None
    try:
        assert step_once(sc, ts)[0].status == 0
        dt = sc.cfg.dt / 2
        ts.setTime(sc.cfg.duration, dt)
        assert ts.dt == dt and ts.frameAmt == int(sc.cfg.duration / dt)
        sc2, _, _ = load(name, energy, dt)
        fresh = make(sc2, ep, n)
        x, v = bring_to_state(fresh, ts)
        assert_same_handle(ts, fresh, sc)       # (targetGRes and x~ are two of its quantities)
        orc = oracle(sc, ep, n, dt=dt)
        orc.set_state(x, v)
        orc.refactor(x)
        assert abs(ts.targetGRes - orc.target_gres) <= 1e-15 * orc.target_gres
        steps_against_oracle(sc, ts, orc, 2, dt=dt)
    finally:
        ts.close()
        for o in (fresh, orc):
            if o is not None:
                o.close()


def test_set_time_step_lbfgs_pd_refactors_the_laplacian():
    """L = M + sum_e dt^2 vol_e (2 mu_e + lambda_e) D_e^T D_e holds dt: the apply is the dense solve of the NEW L at 1e-10
    (tests/test_gpu_lbfgs_pd.py::check_apply)"""
    from tests.test_gpu_lbfgs_pd import check_apply, dense_L
    sc, ep, n = load("synbar:16x5x5:1")
    ts = make(sc, ep, n, pd=True)
    fresh = None
    try:
        assert step_once(sc, ts)[0].status == 0
        dt = sc.cfg.dt / 2
        ts.setTime(sc.cfg.duration, dt)
        sc2, _, _ = load("synbar:16x5x5:1", dt=dt)
        check_apply(ts, dense_L(ts, sc2, sc.fixed))
        fresh = make(sc2, ep, n, pd=True)
        bring_to_state(fresh, ts)
        assert_same_handle(ts, fresh, sc)
    finally:
        ts.close()
        if fresh is not None:
            fresh.close()


# ---- 5. set_rel_tol and the script's schedule ---------------------------------------------------------------------------------
TOLS = [1e-3, 1e-5, 1e-6]


def test_set_rel_tol_is_the_fresh_handles_tolerance():
    sc, ep, n = load("synbar:8x3x3:4")
    ts = make(sc, ep, n)
    try:
        for t in TOLS:
            ts.setRelGL2Tol(t)
            fresh = make(sc, ep, n, rel_tol=t)
            assert ts.targetGRes == fresh.targetGRes, t
            fresh.close()
    finally:
        ts.close()


def test_each_tolerance_takes_the_fresh_oracles_step():
    """bunny5K_LTSS: two steps at 1e-5, then the third step once per tolerance from the same saved state, each against the oracle
    built with that tolerance and brought to that state.  (The oracle alone takes 1, 9 and 14 iterations.)"""
    sc, ep, n = load("bunny5K_LTSS")
    ts, orc = make(sc, ep, n), oracle(sc, ep, n)
    try:
        steps_against_oracle(sc, ts, orc, 2)
        orc.close()
        x, v, _ = ts.getState()
        idx, pos = sc.scripter.step(x, sc.cfg.dt)
        iters = []
        for t in TOLS:
            ts.setState(x, v)
            ts.updatePrecondMtrAndFactorize()
            ts.setRelGL2Tol(t)
            orc = oracle(sc, ep, n, rel_tol=t)
            orc.set_state(x, v)
            orc.refactor(x)
            assert abs(ts.targetGRes - orc.target_gres) <= 1e-15 * orc.target_gres
            ts.setDirichlet(idx, pos)
            orc.move(idx, pos)
            st, so = ts.step(), orc.step()
            dx = np.abs(ts.getResult() - orc.state()[0]).max()
            print(f"relTol {t:g}: device {(st.status, st.iters, st.ls_halvings)} oracle {(so.status, so.iters, so.ls_halvings)} "
                  f"max|dx| {dx:.2e}")
            assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), t
            assert st.status == 0 and st.g2 <= ts.targetGRes
            assert dx < 1e-9, (t, dx)
            iters.append(st.iters)
            orc.close()
        assert len(set(iters)) == 3, iters
    finally:
        ts.close(); orc.close()


def test_solve_follows_the_scripts_tolerance_list():
    """main.cpp:108-118: step k runs at tol[k], beyond the list's end at its last entry"""
    sc, ep, n = load("synbar:8x3x3:4")
    sc.cfg.tol = [1e-3, 1e-5]
    ts = make(sc, ep, n)
    want = {}
    try:
        for t in sc.cfg.tol:
            sc2, _, _ = load("synbar:8x3x3:4")
            fresh = make(sc2, ep, n, rel_tol=t)
            want[t] = fresh.targetGRes
            fresh.close()
        assert want[1e-3] != want[1e-5]
        seen = []
        for k in range(3):
            assert ts.solve(1) == 0
            seen.append(ts.targetGRes)
            assert ts.last_stats.g2 <= seen[-1]
        assert seen == [want[1e-3], want[1e-5], want[1e-5]]
    finally:
        ts.close()


# ---- 6. the runner ------------------------------------------------------------------------------------------------------------
def test_runner_applies_the_tolerance_schedule(tmp_path):
    """dot_hip on a script with `tol 3`: log.txt carries the three tolerances in the script's order, then the last one again
    (Optimizer::setRelGL2Tol writes "<n>th tol: <targetGRes>", Optimizer.cpp:227)"""
    from tests.test_host_logic import _write_msh
    from tests.workloads import MESH_DIR
    exe = os.path.join(ROOT, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    (tmp_path / "bunny.txt").write_text("energy FCR\ntimeStepper DOT 8\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\n"
                                        "stiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n"
                                        "tol 3\n1e-3\n1e-5\n1e-6\n")
    sc, ep, n = load_workload("bunny5K_LTSS")
    ep.astype(np.int32).tofile(tmp_path / "epart.i32")
    out = subprocess.check_output([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--epart",
                                   str(tmp_path / "epart.i32"), "--frames", "5", "--out", str(tmp_path / "out")]).decode()
    frames = [l.split() for l in out.splitlines() if l.startswith("FRAME")]
    assert len(frames) == 5 and all(f[-1] == "0" for f in frames)
    log = [l.split() for l in (tmp_path / "out" / "log.txt").read_text().splitlines() if "th tol:" in l]
    assert [l[0] for l in log] == [f"{k}th" for k in range(5)]
    tols = [l[2] for l in log]
    ts = DOTTimeStepper(sc, ep, n)
    want = []
    for t in TOLS:
        ts.setRelGL2Tol(t)
        want.append("%g" % ts.targetGRes)
    ts.close()
    assert len(set(want)) == 3
    assert tols == want + [want[2], want[2]]


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def test_bad_arguments_change_nothing():
    sc, ep, n = load("synbar:8x3x3:4")
    ts = make(sc, ep, n)
    try:
        assert step_once(sc, ts)[0].status == 0
        mu, lam = field(sc, "random")
        ts.setLame(mu, lam)                       # (a field, so that a half-applied material change would show)
        rng = np.random.default_rng(2)
        r = rng.standard_normal(sc.x0.shape)
        tol0, p0, xt0 = ts.targetGRes, ts.applyPrecond(r), ts.getState()[2]
        L, h = ts._L, ts._h
        bad_mu = mu.copy(); bad_mu[len(mu) // 2] = 0.0
        neg_lam = lam.copy(); neg_lam[-1] = -1.0
        nan_mu = mu.copy(); nan_mu[0] = np.nan
        inf_lam = lam.copy(); inf_lam[1] = np.inf
        calls = [("relTol nan", lambda: L.dotmi_set_rel_tol(h, float("nan"))), ("relTol 0", lambda: L.dotmi_set_rel_tol(h, 0.0)),
                 ("relTol < 0", lambda: L.dotmi_set_rel_tol(h, -1e-5)), ("relTol inf", lambda: L.dotmi_set_rel_tol(h, float("inf"))),
                 ("dt nan", lambda: L.dotmi_set_time_step(h, float("nan"))), ("dt 0", lambda: L.dotmi_set_time_step(h, 0.0)),
                 ("dt < 0", lambda: L.dotmi_set_time_step(h, -0.01)), ("dt inf", lambda: L.dotmi_set_time_step(h, float("inf"))),
                 ("mu with a zero", lambda: L.dotmi_set_lame(h, dl.dp(bad_mu), dl.dp(lam))),
                 ("lambda < 0", lambda: L.dotmi_set_lame(h, dl.dp(mu), dl.dp(neg_lam))),
                 ("mu nan", lambda: L.dotmi_set_lame(h, dl.dp(nan_mu), dl.dp(lam))),
                 ("lambda inf", lambda: L.dotmi_set_lame(h, dl.dp(mu), dl.dp(inf_lam))),
                 ("mu NULL", lambda: L.dotmi_set_lame(h, None, dl.dp(lam))), ("lambda NULL", lambda: L.dotmi_set_lame(h, dl.dp(mu), None)),
                 ("handle NULL", lambda: L.dotmi_set_rel_tol(None, 1e-5)), ("handle NULL", lambda: L.dotmi_set_time_step(None, 0.01)),
                 ("handle NULL", lambda: L.dotmi_set_lame(None, dl.dp(mu), dl.dp(lam)))]
        for what, call in calls:
            assert call() == -1, what             # DOTMI_E_INVALID
            if "handle" not in what:
                assert L.dotmi_last_error(h).decode() != "", what
            assert ts.targetGRes == tol0, what
            assert np.array_equal(ts.applyPrecond(r), p0), what
            assert np.array_equal(ts.getState()[2], xt0), what
        with pytest.raises(DotmiError):
            ts.setLame(bad_mu, lam)
        with pytest.raises(DotmiError):
            ts.setRelGL2Tol(0.0)
        with pytest.raises(DotmiError):
            ts.setTime(sc.cfg.duration, 0.0)
        assert ts.dt == sc.cfg.dt and ts.rel_tol == 1e-5
        # a wrong shape never reaches the library
        ts._L = None
        with pytest.raises(ValueError):
            ts.setLame(mu[:-1], lam)
        with pytest.raises(ValueError):
            ts.setLame(mu, np.stack([lam, lam]))
        ts._L = L
    finally:
        ts._L = dl.load()
        ts.close()


def _pending_refresh_worker(q):
    """in a process of its own, on the fault-injection build (tests/test_gpu_round4.py::_async_failure_worker): the refresh at the
    end of step 1 fails; every setter called directly after that step must report it and change nothing"""
    sys.path.insert(0, ROOT)
    from dot_amd import lib as dl_
    from dot_amd.timestepper import DOTTimeStepper as TS
    from tests.materials import field as field_
    from tests.workloads import load_workload as lw
    out = {}
    try:
        for name in ("rel_tol", "time_step", "lame"):
            sc, ep, n = lw("synbar:8x3x3:4")
            ts = TS(sc, ep, n, flags=dl_.FLAG_ASYNC_REFRESH)
            sc.scripter.track(sc.x0)
            for k in range(2):
                idx, pos = sc.scripter.step(None, sc.cfg.dt)
                ts.setDirichlet(idx, pos)
                out[f"{name} status{k}"] = ts.step().status    # step 1 returns with its (failing) refresh still queued
            mu, lam = field_(sc, "random")
            call = {"rel_tol": lambda: ts.setRelGL2Tol(1e-3), "time_step": lambda: ts.setTime(sc.cfg.duration, sc.cfg.dt / 2),
                    "lame": lambda: ts.setLame(mu, lam)}[name]
            tol0 = ts.targetGRes
            try:
                call()
                out[name] = "no error"
            except dl_.DotmiError as e:
                out[name] = str(e)
            out[f"{name} unchanged"] = ts.targetGRes == tol0
            call()                                             # the verdict has been delivered: now the value is taken ...
            out[f"{name} changed"] = ts.targetGRes != tol0
            if name == "rel_tol":
                ts.updatePrecondMtrAndFactorize()              # (no refresh of its own: a good factorisation heals the handle)
            idx, pos = sc.scripter.step(None, ts.dt)
            ts.setDirichlet(idx, pos)
            out[f"{name} healed"] = ts.step().status           # ... and the refreshing setters have healed the handle
            ts.close()
    except Exception as e:   # noqa: BLE001
        out["exception"] = repr(e)
    q.put(out)


def test_a_setter_reports_a_pending_refresh_first():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_pending_refresh_worker, args=(q,))
    # 1 = the factorisation in dotmi_create, 2 = the refresh at the end of step 0, 3 = the one at the end of step 1
    hook = {"DOTMI_LIBRARY": os.path.join(ROOT, "dot_amd", "libdotmi_testhooks.so"), "DOTMI_TEST_FAIL_REFRESH": "3"}
    os.environ.update(hook)
    try:
        p.start()
    finally:
        for k in hook:
            del os.environ[k]
    out = q.get(timeout=300)
    p.join(timeout=60)
    assert "exception" not in out, out
    for name in ("rel_tol", "time_step", "lame"):
        assert out[f"{name} status0"] == 0 and out[f"{name} status1"] == 0, out
        assert "-3" in out[name], out                          # DOTMI_E_NOTSPD, the synchronous path's error
        assert out[f"{name} unchanged"] and out[f"{name} changed"], out
        assert out[f"{name} healed"] == 0, out
