"""The rigid-mode coarse term of DOT's block preconditioner on the device (dotmi_set_dot_coarse; dot_amd/csrc/k_coarse.hip,
k_loopvec.hip's COARSE merges, dotmi_coarse.hip, dotmi_devloop.hip): one application, the probe and whole steps against the numpy
restatement (tests/dot_coarse_reference.py on an OracleSim, Z and A0 from tests/coarse_reference.py); every form the merge and the
slot have; determinism; the iteration count; one build per refresh; off means untouched; a dropped subdomain; refusals; the runner.

Shapes: synbar:16x5x5:4 (nc = 24: one mostly padded tile), synbar:48x4x4:12 (nc = 72: a row block boundary inside A0),
synbar:96x4x4:32 (nc = 192: three full blocks), bunny5K_LTSS / 8 (fixed-corotational, element patches, dup <= 5).

The inactive fallback (a non-positive pivot of A0) is not provoked on the device: tests/test_dot_coarse_host.py covers it in the
restatement; on the device it is `active = h_info == 0` in coarse_finish, which dot_coarse() reads."""
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import dot_coarse_reference as DR
from tests import pcg_reference as R
from tests.test_dot_coarse_host import gravity, make_oracle, restated_run

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


def device_run(name, mode, flags=0, steps=STEPS, toggle=False):
    """`steps` scripted steps on a fresh handle -> (per step (iterations, halvings, status), positions after every step, the
    dotCoarseInfo after every step).  toggle: the mode is switched on and off again before the first step"""
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n, flags=flags)
    if toggle:
        ts.setDotCoarse(1)
        ts.setDotCoarse(0)
    if mode:
        ts.setDotCoarse(1)
    counts, xs, infos = [], [], []
    for _ in range(steps):
        scripted(sc, ts)
        st = ts.step()
        counts.append((st.iters, st.ls_halvings, st.status))
        xs.append(ts.getResult().copy())
        infos.append(ts.dotCoarseInfo())
    ts.close()
    return counts, xs, infos


def cached_run(name, mode):
    """the default form's run, once per (shape, mode)"""
    if (name, mode) not in _runs:
        _runs[(name, mode)] = device_run(name, mode)
    return _runs[(name, mode)]


# ---- 1. one application -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_application_is_the_plain_one_plus_the_restated_coarse_term_and_untouched_when_off(name):
    """dotmi_apply_precond with the mode on against (the same entry with the mode off) + Z A0^-1 Z^T r restated on the handle's own
    dotmi_spmv and positions: 1e-10 of the largest entry, the bound of tests/test_gpu_pcg_coarse.py.  Off again: the bits of a handle
    that never enabled the mode"""
    def two_steps_in():
        sc, ep, n = load_workload(name)
        ts = DOTTimeStepper(sc, ep, n)
        for _ in range(2):
            scripted(sc, ts)
            assert ts.step().status == 0
        scripted(sc, ts)
        ts.updatePrecondMtrAndFactorize()
        return sc, ep, n, ts
    sc, ep, n, ts = two_steps_in()
    _, _, _, never = two_steps_in()
    nV = sc.V_rest.shape[0]
    fixed = np.asarray(sc.fixed, dtype=bool)
    r = random_free(fixed, 11)
    off = ts.applyPrecond(r)
    assert np.array_equal(off, never.applyPrecond(r))
    apply, live = DR.coarse_term(ts.getResult(), R.dup_of(sc.T, ep, nV), part_verts(sc.T, ep, n), fixed, ts.multiply)
    assert live.all() and apply is not None
    builds0 = ts.dotCoarseInfo()[3]
    ts.setDotCoarse(1)
    dim, dropped, active, builds, ms = ts.dotCoarseInfo()
    assert (dim, dropped, active, builds) == (6 * n, 0, 1, builds0 + 1) and ms > 0.0
    on = ts.applyPrecond(r)
    want = off + apply(r)
    err = np.abs(on - want).max() / np.abs(want).max()
    print(f"{name}: nc {dim}, application against the restatement {err:.2e}; the coarse term is "
          f"{np.abs(on - off).max() / np.abs(on).max():.2e} of it; build {ms:.3f} ms")
    assert err <= 1e-10
    assert np.array_equal(ts.applyPrecond(r), on)
    assert np.array_equal(on[fixed], off[fixed])                 # w = 0 on fixed vertices: the coarse term adds nothing there
    assert ts.dotCoarseInfo()[3] == builds0 + 1                  # nothing refreshed: no build
    ts.setDotCoarse(0)
    assert ts.dotCoarseInfo()[:3] == (0, 0, 0)
    assert np.array_equal(ts.applyPrecond(r), never.applyPrecond(r))
    assert never.dotCoarseInfo()[:4] == (0, 0, 0, 0)
    ts.close()
    never.close()


# ---- 2. the probe ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR12, BUNNY])
def test_probe_direction_uses_the_coarse_term(name):
    """dotmi_probe_direction from the restatement's iterate and history in front of iterations 0 (m = 0) and 3 (m = 3) of the first
    step: p and alpha_0 within 1e-9 of the restatement's direction on the oracle's operators with M'"""
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
    M_run, act = DR.m_prime(run, dup, verts, fixed)
    r = st.step(M_run, keep=True)
    assert act and r["status"] == 0 and len(st.snapshots) > 3
    M_ops, _ = DR.m_prime(ops, dup, verts, fixed)
    ts.setDotCoarse(1)
    assert ts.dotCoarseInfo()[2] == 1
    for k in (0, 3):
        x, S, Y = st.snapshots[k]
        assert len(S) == k
        _, _, p, a0 = DR.direction(ops.gradient(x), S, Y, M_ops, ops.spmv)
        got = ts.probeDirection(x, S if k else None, Y if k else None)
        print(f"{name}, m = {k}: |p| {np.abs(p).max():.3e}, p {np.abs(got['p'] - p).max():.2e}, alpha_0 {got['alpha0']} / {a0}")
        assert np.abs(got["p"] - p).max() < 1e-9 and abs(got["alpha0"] - a0) < 1e-9
    ts.setDotCoarse(0)
    x, S, Y = st.snapshots[3]
    plain = ts.probeDirection(x, S, Y)
    assert np.abs(plain["p"] - got["p"]).max() > 1e-6             # (the term is not a rounding matter)
    ts.close()
    run.close()
    ops.close()


# ---- 3. steps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_four_steps_take_the_restatements_iterations_and_halvings(name):
    want, xr, active = restated_run(name, True)
    got, xs, infos = cached_run(name, 1)
    err = max(np.abs(a - b).max() for a, b in zip(xs, xr))
    print(f"{name}: device {got}, restatement {want}, positions {err:.2e}, builds {[i[3] for i in infos]}")
    assert active and all(i[2] == 1 and i[1] == 0 for i in infos)
    assert got == want
    assert err < 1e-9


# ---- 4. every form of the merge and the slot ------------------------------------------------------------------------------------------------
FORMS = [("default", {}, 0), ("element patches", {"DOTMI_VERTEX_PATCHES": "0"}, 0), ("q-based order", {"DOTMI_EARLY_BACKSOLVE": "0"}, 0),
         ("split merge", {"DOTMI_SPLIT_MERGE": "1"}, 0), ("two-level", {"DOTMI_TWO_LEVEL": "1"}, 0),
         ("paired trials", {"DOTMI_PAIR_TRIALS": "1"}, 0),
         ("split merge, q-based order", {"DOTMI_SPLIT_MERGE": "1", "DOTMI_EARLY_BACKSOLVE": "0"}, 0),
         ("split merge, host loop", {"DOTMI_SPLIT_MERGE": "1"}, dl.FLAG_HOST_LOOP)]


@pytest.mark.parametrize("form,env,flags", FORMS, ids=[f[0] for f in FORMS])
def test_every_form_takes_the_host_loops_steps(form, env, flags, monkeypatch):
    """synbar:96x4x4:32, four steps with the mode on: the list walk, the interleaved lists, the split form (psub) of the early merge;
    merge_tiles_kernel and merge_kernel in the q-based order and in the host loop; held, paired and two-level slots.  Same
    iterations and halvings as DOTMI_FLAG_HOST_LOOP, positions within 1e-9 of its"""
    if "host" not in _runs:
        _runs["host"] = device_run(BAR32, 1, flags=dl.FLAG_HOST_LOOP)
    want, xh, _ = _runs["host"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got, xs, infos = cached_run(BAR32, 1) if form == "default" else device_run(BAR32, 1, flags=flags)
    err = max(np.abs(a - b).max() for a, b in zip(xs, xh))
    print(f"{form}: {got}, host loop {want}, positions {err:.2e}")
    assert all(i[2] == 1 for i in infos)
    assert got == want
    assert err < 1e-9


# ---- 5. determinism, 6. the iteration count --------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    c0, x0, _ = cached_run(BAR32, 1)
    c1, x1, _ = device_run(BAR32, 1)
    assert c1 == c0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)


def test_coarse_term_cuts_the_iterations_on_32_subdomains():
    c0, _, _ = cached_run(BAR32, 0)
    c1, _, _ = cached_run(BAR32, 1)
    t0, t1 = sum(c[0] for c in c0), sum(c[0] for c in c1)
    print(f"{BAR32}: {[c[0] for c in c0]} -> {[c[0] for c in c1]} iterations: {t0} -> {t1}")
    assert all(c[2] == 0 for c in c0 + c1)
    assert t1 <= 0.8 * t0


# ---- 7. one build per refresh; off means untouched -------------------------------------------------------------------------------------------
def test_builds_advance_once_per_refresh():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    assert ts.dotCoarseInfo()[:4] == (0, 0, 0, 0)
    ts.setDotCoarse(1)                                           # the refresh of create built nothing: the setter does
    assert ts.dotCoarseInfo()[:4] == (24, 0, 1, 1)
    ts.setDotCoarse(1)
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
    ts.setDotCoarse(1)                                           # ... so switching it on again builds
    assert ts.dotCoarseInfo()[2:4] == (1, builds + 1)
    ts.close()


def test_a_handle_that_enabled_and_disabled_the_mode_steps_like_one_that_never_did():
    c0, x0, i0 = cached_run(BAR32, 0)
    c1, x1, i1 = device_run(BAR32, 0, toggle=True)
    assert c1 == c0
    for a, b in zip(x0, x1):
        assert np.array_equal(a, b)
    assert all(i[:4] == (0, 0, 0, 0) for i in i0) and all(i[:4] == (0, 0, 0, 1) for i in i1)


# ---- 8. a dropped subdomain ------------------------------------------------------------------------------------------------------------------
def test_subdomain_fixed_through_refix_is_dropped_and_the_steps_match_the_restatement():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    orc = make_oracle(sc, ep, n)
    verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed[verts[0]] = 1
    fx = fixed.astype(bool)
    ts.setDotCoarse(1)
    ts.refix(fixed)
    orc.set_fixed(fixed)
    assert ts.dotCoarseInfo()[:3] == (24, 1, 1)
    st = DR.DotStepper(orc, fx, sc.cfg.dt, gravity(sc.cfg))
    dup = orc.dup()
    for k in range(2):
        scripted(sc, ts, orc)
        apply, live = DR.coarse_term(orc.state()[0], dup, verts, fx, orc.spmv)
        assert list(live) == [False, True, True, True] and apply is not None
        want = st.step(CR.precond(orc.apply_precond, apply))
        got = ts.step()
        err = np.abs(ts.getResult() - orc.state()[0]).max()
        print(f"subdomain 0 fixed, step {k}: {got.iters} / {want['iters']} iterations, positions {err:.2e}")
        assert (got.iters, got.ls_halvings, got.status) == (want["iters"], want["halvings"], want["status"]) and got.status == 0
        assert err < 1e-9
        assert ts.dotCoarseInfo()[1:3] == (1, 1)
    ts.close()
    orc.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(dl.FLAG_FORCE_DIST, "single-rank"), (dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE, "single-rank"),
                                        (dl.FLAG_GSDD, "GSDD"), (dl.FLAG_NEWTON_PCG, "Newton-PCG"),
                                        (dl.FLAG_ASYNC_REFRESH, "DOTMI_FLAG_ASYNC_REFRESH")])
def test_mode_is_refused_with_these_flags(flags, word):
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=flags, alpha_min=1.0 if flags == dl.FLAG_NEWTON_PCG else 0.1)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse.*" + word):
        ts.setDotCoarse(1)
    assert ts.dotCoarseInfo()[:4] == (0, 0, 0, 0)
    ts.close()


@pytest.mark.parametrize("flag,word", [(dl.FLAG_NEWTON, "Newton"), (dl.FLAG_LBFGS_PD, "LBFGS-PD"), (dl.FLAG_LBFGS_HI, "LBFGS-HI")])
def test_mode_is_refused_on_the_steppers_of_the_whole_mesh(flag, word):
    sc, ep, n = load_workload(BAR4)
    newton = flag == dl.FLAG_NEWTON
    ts = DOTTimeStepper(sc, np.zeros(sc.T.shape[0], dtype=np.int32) if newton else None, 1, flags=flag, alpha_min=1.0)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse.*" + word):
        ts.setDotCoarse(1)
    ts.close()


def test_mode_is_refused_on_a_vertex_partition_above_256_subdomains_and_for_other_values():
    sc, ep, n = load_workload(BAR4)
    vpart = np.full(sc.V_rest.shape[0], n, dtype=np.int32)      # a vertex goes to the lowest subdomain among its elements
    np.minimum.at(vpart, np.asarray(sc.T).ravel(), np.repeat(ep, 4))
    ts = DOTTimeStepper(sc, None, n, vpart=vpart)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse.*vpart"):
        ts.setDotCoarse(1)
    ts.close()
    ts = DOTTimeStepper(sc, ep, n)
    for mode in (2, -1):
        with pytest.raises(DotmiError, match="dotmi_set_dot_coarse: mode"):
            ts.setDotCoarse(mode)
    ts.close()
    sc, ep, n = load_workload("synbar:40x3x3:257")
    assert n == 257
    ts = DOTTimeStepper(sc, ep, n)
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse: at most 256 subdomains"):
        ts.setDotCoarse(1)
    ts.setDotCoarse(0)
    ts.close()


# ---- 10. the runner --------------------------------------------------------------------------------------------------------------------------
def test_headless_runner_takes_dot_coarse(tmp_path):
    """dot_hip --dot-coarse on the bunny script of tests/test_gpu_parity.py's runner test: exit 0, the coarse space reported, and in
    log.txt at most the iterations of the run without the flag; together with --newton-pcg the flag is refused"""
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
    for tag, extra in (("off", []), ("on", ["--dot-coarse"])):
        res = subprocess.run([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--epart", str(tmp_path / "epart.i32"),
                              "--frames", "3", "--out", str(tmp_path / tag)] + extra, capture_output=True, timeout=600)
        assert res.returncode == 0, res.stderr.decode()
        log = [l for l in (tmp_path / tag / "log.txt").read_text().splitlines() if "innerIterAmt" in l]
        assert len(log) == 3
        totals[tag] = int(log[-1].split("innerIterAmt = ")[1].split(",")[0])
        if extra:
            assert "DOT coarse space: dimension 48, 0 dropped, active 1, 4 builds" in res.stdout.decode()
    print(f"dot_hip, three frames of the bunny: {totals['off']} -> {totals['on']} iterations")
    assert 0 < totals["on"] <= totals["off"]
    bad = subprocess.run([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--dot-coarse", "--newton-pcg", "4",
                          "--dump-scene", "0"], capture_output=True, timeout=600)
    assert bad.returncode == 1 and b"--dot-coarse" in bad.stderr
