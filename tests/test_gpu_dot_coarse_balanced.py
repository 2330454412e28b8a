"""The balanced form of DOT's coarse term on the device (dotmi_set_dot_coarse_mode, mode 2; dot_amd/csrc/k_coarse.hip, dotmi_coarse.hip,
dotmi_loop.hip, dotmi_devloop.hip): one application, exactness on the coarse space, the probe and whole steps against the numpy
restatement (tests/dot_coarse_balanced_reference.py); the forms of the block solve and of the merge the mode runs under; determinism;
switching between the modes; one build per refresh; a dropped subdomain; the iteration count against mode 1; refusals; the runner.

Shapes: synbar:16x5x5:4 (nc = 24: one mostly padded tile), synbar:48x4x4:12 (nc = 72: a row block boundary inside A0),
synbar:96x4x4:32 (nc = 192: three full blocks), bunny5K_LTSS / 8 (fixed-corotational, dup <= 5).

The inactive fallback (a non-positive pivot of A0) is not provoked on the device: tests/test_dot_coarse_balanced_host.py covers it in
the restatement; on the device it is `active = h_info == 0` in coarse_finish, which dot_coarse_balanced() reads."""
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import dot_coarse_balanced_reference as BR
from tests import dot_coarse_reference as DR
from tests import pcg_reference as R
from tests.test_dot_coarse_balanced_host import balanced_run
from tests.test_dot_coarse_host import gravity, make_oracle

pytestmark = pytest.mark.gpu

BAR4, BAR12, BAR32, BUNNY = "synbar:16x5x5:4", "synbar:48x4x4:12", "synbar:96x4x4:32", "bunny5K_LTSS"
SHAPES = [BAR4, BAR12, BAR32, BUNNY]
STEPS = 4
_runs = {}


def scripted(sc, ts, orc=None):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    if orc is not None:
        orc.move(idx, pos)


def part_verts(T, ep, n):
    T, ep = np.asarray(T), np.asarray(ep)
    return [np.unique(T[ep == s]) for s in range(n)]


def random_free(fixed, seed):
    v = np.random.default_rng(seed).standard_normal((fixed.size, 3))
    v[fixed] = 0.0
    return v


def device_run(name, modes, flags=0, steps=STEPS):
    """`steps` scripted steps on a fresh handle after switching through `modes` in turn -> (per step (iterations, halvings, status),
    positions after every step, the dotCoarseInfo after every step, per step backsolve_stopped: 0 in the q-based order of the device
    loop and in the host loop, halvings + 1 or more in the early order)"""
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n, flags=flags)
    for m in modes:
        ts.setDotCoarseMode(m)
    assert ts.dotCoarseMode() == (modes[-1] if modes else 0)
    counts, xs, infos, stopped = [], [], [], []
    for _ in range(steps):
        scripted(sc, ts)
        st = ts.step()
        counts.append((st.iters, st.ls_halvings, st.status))
        xs.append(ts.getResult().copy())
        infos.append(ts.dotCoarseInfo())
        stopped.append(st.backsolve_stopped)
    ts.close()
    return counts, xs, infos, stopped


def cached_run(name, modes):
    """the default form's run, once per (shape, modes)"""
    if (name, modes) not in _runs:
        _runs[(name, modes)] = device_run(name, modes)
    return _runs[(name, modes)]


def two_steps_in(name):
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n)
    for _ in range(2):
        scripted(sc, ts)
        assert ts.step().status == 0
    scripted(sc, ts)
    ts.updatePrecondMtrAndFactorize()
    return sc, ep, n, ts


# ---- 1. one application, 2. exactness -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_application_is_the_restated_balanced_form_and_exact_on_the_coarse_space(name):
    """dotmi_apply_precond in mode 2 against M'' restated on the handle's own dotmi_spmv, its mode-0 dotmi_apply_precond and its
    positions: 1e-10 of the largest entry, the standing bound of tests/test_gpu_dot_coarse.py.  apply_precond(spmv(Z y)) against Z y
    for four random y: 1e-10 of the largest entry"""
    sc, ep, n, ts = two_steps_in(name)
    nV = sc.V_rest.shape[0]
    fixed = np.asarray(sc.fixed, dtype=bool)
    r = random_free(fixed, 11)
    off = ts.applyPrecond(r)
    Z, A0, W, live = BR.parts(ts.getResult(), R.dup_of(sc.T, ep, nV), part_verts(sc.T, ep, n), fixed, ts.multiply)
    assert live.all()
    # (the plain applications the restatement needs are taken with the mode off, all before it is switched on)
    rng = np.random.default_rng(7)
    ys = [rng.standard_normal(6 * n) for _ in range(4)]
    solve = lambda c: np.linalg.solve(A0, c)
    y1 = solve(Z.T @ r.ravel())
    u = ts.applyPrecond((r.ravel() - W @ y1).reshape(-1, 3)).ravel()
    want = (u + Z @ (y1 - solve(W.T @ u))).reshape(-1, 3)
    builds0 = ts.dotCoarseInfo()[3]
    ts.setDotCoarseMode(2)
    dim, dropped, active, builds, ms = ts.dotCoarseInfo()
    assert (dim, dropped, active, builds) == (6 * n, 0, 1, builds0 + 1) and ms > 0.0 and ts.dotCoarseMode() == 2
    on = ts.applyPrecond(r)
    err = np.abs(on - want).max() / np.abs(want).max()
    worst = 0.0
    for y in ys:
        zy = (Z @ y).reshape(-1, 3)
        worst = max(worst, np.abs(ts.applyPrecond(ts.multiply(zy)) - zy).max() / np.abs(zy).max())
    print(f"{name}: nc {dim}, application against the restatement {err:.2e}; M'' H Z y against Z y {worst:.2e}; the correction is "
          f"{np.abs(on - off).max() / np.abs(on).max():.2e} of the result; build {ms:.3f} ms")
    assert err <= 1e-10
    assert worst <= 1e-10
    assert np.array_equal(ts.applyPrecond(r), on)                # two applications: the same bits
    assert ts.dotCoarseInfo()[3] == builds0 + 1                  # nothing refreshed: no build
    ts.setDotCoarse(0)
    assert ts.dotCoarseInfo()[:3] == (0, 0, 0) and ts.dotCoarseMode() == 0
    assert np.array_equal(ts.applyPrecond(r), off)
    ts.close()


# ---- 3. the probe ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR12, BUNNY])
def test_probe_direction_uses_the_balanced_form(name):
    """dotmi_probe_direction from the restatement's iterate and history in front of iterations 0 (m = 0) and 3 (m = 3) of the first
    step: p and alpha_0 within 1e-9 of the restatement's direction on the oracle's operators with M''"""
    sc, ep, n = load_workload(name)
    fixed = np.asarray(sc.fixed, dtype=bool)
    ts = DOTTimeStepper(sc, ep, n)
    run, ops = make_oracle(sc, ep, n), make_oracle(sc, ep, n)    # one oracle takes the step, the other keeps the step's operators
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    run.move(idx, pos)
    ops.move(idx, pos)
    dup = run.dup()
    verts = [np.asarray(run.part_verts(p)) for p in range(n)]
    st = DR.DotStepper(run, fixed, sc.cfg.dt, gravity(sc.cfg))
    M_run, act = BR.m_second(run, dup, verts, fixed)
    r = st.step(M_run, keep=True)
    assert act and r["status"] == 0 and len(st.snapshots) > 3
    M_ops, _ = BR.m_second(ops, dup, verts, fixed)
    ts.setDotCoarseMode(2)
    assert ts.dotCoarseInfo()[2] == 1
    for k in (0, 3):
        x, S, Y = st.snapshots[k]
        assert len(S) == k
        _, _, p, a0 = DR.direction(ops.gradient(x), S, Y, M_ops, ops.spmv)
        got = ts.probeDirection(x, S if k else None, Y if k else None)
        print(f"{name}, m = {k}: |p| {np.abs(p).max():.3e}, p {np.abs(got['p'] - p).max():.2e}, alpha_0 {got['alpha0']} / {a0}")
        assert np.abs(got["p"] - p).max() < 1e-9 and abs(got["alpha0"] - a0) < 1e-9
    ts.setDotCoarse(1)
    x, S, Y = st.snapshots[3]
    additive = ts.probeDirection(x, S, Y)
    assert np.abs(additive["p"] - got["p"]).max() > 1e-6          # (the two forms do not differ by rounding)
    ts.close()
    run.close()
    ops.close()


# ---- 4. steps, in every form the mode runs under ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_four_steps_take_the_restatements_iterations_and_halvings_in_the_q_based_order(name):
    want, xr, active = balanced_run(name)
    got, xs, infos, stopped = cached_run(name, (2,))
    err = max(np.abs(a - b).max() for a, b in zip(xs, xr))
    print(f"{name}: device {got}, restatement {want}, positions {err:.2e}, builds {[i[3] for i in infos]}, stopped {stopped}")
    assert active and all(i[2] == 1 and i[1] == 0 for i in infos)
    assert stopped == [0] * STEPS                                 # the default device loop runs the q-based order while the mode is active
    assert got == want
    assert err < 1e-9


FORMS = [("host loop", {}, dl.FLAG_HOST_LOOP), ("split merge", {"DOTMI_SPLIT_MERGE": "1"}, 0), ("two-level", {"DOTMI_TWO_LEVEL": "1"}, 0),
         ("split merge, host loop", {"DOTMI_SPLIT_MERGE": "1"}, dl.FLAG_HOST_LOOP)]


@pytest.mark.parametrize("form,env,flags", FORMS, ids=[f[0] for f in FORMS])
def test_every_form_takes_the_restatements_steps(form, env, flags, monkeypatch):
    """synbar:96x4x4:32, four steps in mode 2: merge_tiles_kernel and merge_kernel without their division in front of the finishing
    kernel, in the device loop and the host loop; the two-level block solve behind the deflated right-hand side"""
    want, xr, _ = balanced_run(BAR32)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, xs, infos, stopped = device_run(BAR32, (2,), flags=flags)
    err = max(np.abs(a - b).max() for a, b in zip(xs, xr))
    print(f"{form}: {got}, restatement {want}, positions {err:.2e}")
    assert all(i[2] == 1 for i in infos) and stopped == [0] * STEPS
    assert got == want
    assert err < 1e-9


# ---- 5. determinism, 6. switching ------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    c0, x0, _, _ = cached_run(BAR32, (2,))
    c1, x1, _, _ = device_run(BAR32, (2,))
    assert c1 == c0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


def test_mode_two_then_off_steps_like_a_handle_that_never_enabled_it_in_the_early_order():
    c0, x0, i0, s0 = cached_run(BAR32, ())
    c1, x1, i1, s1 = device_run(BAR32, (2, 0))
    assert c1 == c0 and s1 == s0
    assert all(s == c[1] + 1 for s, c in zip(s1, c1))             # the early order is back: halvings + 1 stopped back-solves
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    assert all(i[:4] == (0, 0, 0, 0) for i in i0) and all(i[:4] == (0, 0, 0, 1) for i in i1)


def test_mode_two_then_one_steps_like_a_handle_that_only_had_mode_one():
    c0, x0, i0, s0 = cached_run(BAR32, (1,))
    c1, x1, i1, s1 = device_run(BAR32, (2, 1))
    assert c1 == c0 and s1 == s0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    assert [i[:3] for i in i1] == [i[:3] for i in i0]
    assert [i[3] for i in i1] == [i[3] for i in i0]               # 2 -> 1 keeps the build


def test_mode_one_then_two_steps_like_a_handle_that_only_had_mode_two():
    c0, x0, i0, _ = cached_run(BAR32, (2,))
    c1, x1, i1, _ = device_run(BAR32, (1, 2))
    assert c1 == c0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    assert [i[3] for i in i1] == [i[3] + 1 for i in i0]           # 1 -> 2 rebuilds: W = H Z comes with A0


# ---- 7. one build per refresh ---------------------------------------------------------------------------------------------------------------
def test_builds_advance_once_per_refresh():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    assert ts.dotCoarseInfo()[:4] == (0, 0, 0, 0)
    ts.setDotCoarseMode(2)                                           # the refresh of create built nothing: the setter does
    assert ts.dotCoarseInfo()[:4] == (24, 0, 1, 1)
    ts.setDotCoarseMode(2)
    assert ts.dotCoarseInfo()[3] == 1
    builds = 1
    for k in range(2):
        scripted(sc, ts)
        assert ts.step().status == 0
        builds += 1                                              # the step's refresh, and nothing at the start of the next step
        assert ts.dotCoarseInfo()[2:4] == (1, builds), k
    r = random_free(np.asarray(sc.fixed, dtype=bool), 3)
    ts.applyPrecond(r)
    assert ts.dotCoarseInfo()[3] == builds
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed[np.flatnonzero(fixed == 0)[:5]] = 1
    ts.refix(fixed)
    builds += 1
    assert ts.dotCoarseInfo()[2:4] == (1, builds)
    ts.setTime(sc.cfg.duration, 0.5 * sc.cfg.dt)
    builds += 1
    assert ts.dotCoarseInfo()[2:4] == (1, builds)
    ts.updatePrecondMtrAndFactorize()
    builds += 1
    assert ts.dotCoarseInfo()[2:4] == (1, builds)
    ts.setDotCoarse(0)
    scripted(sc, ts)
    assert ts.step().status == 0
    assert ts.dotCoarseInfo()[:4] == (0, 0, 0, builds)           # the mode off: no build behind the refresh
    ts.setDotCoarseMode(2)                                           # ... so switching it on again builds
    assert ts.dotCoarseInfo()[2:4] == (1, builds + 1)
    ts.close()


# ---- 8. a dropped subdomain ------------------------------------------------------------------------------------------------------------------
def test_subdomain_fixed_through_refix_is_dropped_and_the_steps_match_the_restatement():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    orc = make_oracle(sc, ep, n)
    verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed[verts[0]] = 1
    fx = fixed.astype(bool)
    ts.setDotCoarseMode(2)
    ts.refix(fixed)
    orc.set_fixed(fixed)
    assert ts.dotCoarseInfo()[:3] == (24, 1, 1)
    st = DR.DotStepper(orc, fx, sc.cfg.dt, gravity(sc.cfg))
    dup = orc.dup()
    for k in range(2):
        scripted(sc, ts, orc)
        Z, A0, W, live = BR.parts(orc.state()[0], dup, verts, fx, orc.spmv)
        assert list(live) == [False, True, True, True]
        want = st.step(BR.balanced(orc.apply_precond, Z, A0, W))
        got = ts.step()
        err = np.abs(ts.getResult() - orc.state()[0]).max()
        print(f"subdomain 0 fixed, step {k}: {got.iters} / {want['iters']} iterations, positions {err:.2e}")
        assert (got.iters, got.ls_halvings, got.status) == (want["iters"], want["halvings"], want["status"]) and got.status == 0
        assert err < 1e-9
        assert ts.dotCoarseInfo()[1:3] == (1, 1)
    ts.close()
    orc.close()


# ---- 9. the iteration count -------------------------------------------------------------------------------------------------------------------
def test_balanced_form_takes_at_most_seven_tenths_of_mode_ones_iterations_on_32_subdomains():
    c1, _, _, _ = cached_run(BAR32, (1,))
    c2, _, _, _ = cached_run(BAR32, (2,))
    t1, t2 = sum(c[0] for c in c1), sum(c[0] for c in c2)
    print(f"{BAR32}: mode 1 {[c[0] for c in c1]} -> mode 2 {[c[0] for c in c2]} iterations: {t1} -> {t2}")
    assert all(c[2] == 0 for c in c1 + c2)
    assert t2 <= 0.7 * t1


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(dl.FLAG_FORCE_DIST, "single-rank"), (dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE, "single-rank"),
                                        (dl.FLAG_FORCE_DIST | dl.FLAG_DOT_COARSE, "single-rank"),
                                        (dl.FLAG_GSDD, "GSDD"), (dl.FLAG_NEWTON_PCG, "Newton-PCG"),
                                        (dl.FLAG_ASYNC_REFRESH, "DOTMI_FLAG_ASYNC_REFRESH")])
def test_mode_two_is_refused_with_these_flags(flags, word):
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=flags, alpha_min=1.0 if flags == dl.FLAG_NEWTON_PCG else 0.1)
    before = ts.dotCoarseMode()
    assert before == (1 if flags & dl.FLAG_DOT_COARSE else 0)    # DOTMI_FLAG_DOT_COARSE at create stays mode 1
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse_mode: .*" + word):
        ts.setDotCoarseMode(2)
    assert ts.dotCoarseMode() == before
    ts.close()


@pytest.mark.parametrize("flag,word", [(dl.FLAG_NEWTON, "Newton"), (dl.FLAG_LBFGS_PD, "LBFGS-PD"), (dl.FLAG_LBFGS_HI, "LBFGS-HI")])
def test_mode_two_is_refused_on_the_steppers_of_the_whole_mesh(flag, word):
    sc, ep, n = load_workload(BAR4)
    newton = flag == dl.FLAG_NEWTON
    ts = DOTTimeStepper(sc, np.zeros(sc.T.shape[0], dtype=np.int32) if newton else None, 1, flags=flag, alpha_min=1.0)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse_mode: .*" + word):
        ts.setDotCoarseMode(2)
    ts.close()


def test_mode_two_is_refused_on_a_vertex_partition_above_256_subdomains_and_other_values_stay_refused():
    sc, ep, n = load_workload(BAR4)
    vpart = np.full(sc.V_rest.shape[0], n, dtype=np.int32)      # a vertex goes to the lowest subdomain among its elements
    np.minimum.at(vpart, np.asarray(sc.T).ravel(), np.repeat(ep, 4))
    ts = DOTTimeStepper(sc, None, n, vpart=vpart)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse_mode: .*vpart"):
        ts.setDotCoarseMode(2)
    ts.close()
    ts = DOTTimeStepper(sc, ep, n)
    for mode in (3, -1, 256):
        with pytest.raises(DotmiError, match="dotmi_set_dot_coarse_mode: mode"):
            ts.setDotCoarseMode(mode)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse: mode"):   # the two-valued setter keeps refusing what it refused
        ts.setDotCoarse(2)
    assert ts.dotCoarseMode() == 0
    ts.close()
    sc, ep, n = load_workload("synbar:40x3x3:257")
    assert n == 257
    ts = DOTTimeStepper(sc, ep, n)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse_mode: at most 256 subdomains"):
        ts.setDotCoarseMode(2)
    ts.setDotCoarse(0)
    ts.close()


# ---- 11. the runner --------------------------------------------------------------------------------------------------------------------------
def test_headless_runner_takes_dot_coarse_balanced(tmp_path):
    """dot_hip --dot-coarse-balanced on the bunny script of tests/test_gpu_dot_coarse.py's runner test: exit 0, the coarse space
    reported as balanced, and in log.txt at most the iterations of the run with --dot-coarse"""
    from tests.test_host_logic import _write_msh
    from tests.workloads import MESH_DIR
    from dot_amd import scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    (tmp_path / "bunny.txt").write_text("energy FCR\ntimeStepper DOT 8\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\n"
                                        "stiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n")
    sc, ep, n = load_workload(BUNNY)
    ep.astype(np.int32).tofile(tmp_path / "epart.i32")
    totals = {}
    for tag, extra in (("additive", ["--dot-coarse"]), ("balanced", ["--dot-coarse-balanced"])):
        res = subprocess.run([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--epart", str(tmp_path / "epart.i32"),
                              "--frames", "3", "--out", str(tmp_path / tag)] + extra, capture_output=True, timeout=600)
        assert res.returncode == 0, res.stderr.decode()
        log = [l for l in (tmp_path / tag / "log.txt").read_text().splitlines() if "innerIterAmt" in l]
        assert len(log) == 3
        totals[tag] = int(log[-1].split("innerIterAmt = ")[1].split(",")[0])
        out = res.stdout.decode()
        assert "DOT coarse space: dimension 48, 0 dropped, active 1, 4 builds" in out
        assert (", balanced" in out) == (tag == "balanced")
    print(f"dot_hip, three frames of the bunny: --dot-coarse {totals['additive']} -> --dot-coarse-balanced {totals['balanced']} iterations")
    assert 0 < totals["balanced"] <= totals["additive"]
