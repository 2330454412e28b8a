"""The rigid-mode coarse space of Newton-PCG's preconditioner on the device (dotmi_set_pcg_coarse; dot_amd/csrc/k_coarse.hip,
dotmi_coarse.hip): the assembled A0 = Z^T H Z, one application and the solve against the numpy restatement (tests/coarse_reference.py)
driven by the same handle's operators; off means untouched; Newton-PCG steps against the oracle's exact Newton; staleness after
dotmi_refix and dotmi_set_time_step; a dropped subdomain; refusals; the runner flag.

Shapes: synbar:16x5x5:4 (nc = 24: most of the one 64 x 64 tile is identity padding), bunny5K_LTSS / 8 (nc = 48, dup up to 5),
synbar:96x4x4:32 (nc = 192: exactly three tiles, no padding).

The inactive fallback (a non-positive pivot of A0) is not provoked on the device: tests/test_coarse_host.py covers it in the
restatement, and on the device it is `active = h_info == 0` in coarse_refresh with the solve's `coarse` flag read from it."""
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import oracle_py as O
from tests import pcg_reference as R

pytestmark = pytest.mark.gpu

BAR4, BUNNY, BAR32 = "synbar:16x5x5:4", "bunny5K_LTSS", "synbar:96x4x4:32"
SHAPES = [BAR4, BUNNY, BAR32]
_cache = {}


def scripted(sc, ts, orc=None):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    if orc is not None:
        orc.move(idx, pos)


def part_verts(T, ep, n):
    T, ep = np.asarray(T), np.asarray(ep)
    return [np.unique(T[ep == s]) for s in range(n)]


def two_steps_in(name):
    """a DOT handle two steps into the script, the handles moved for the third, refactored there"""
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n)
    for _ in range(2):
        scripted(sc, ts)
        assert ts.step().status == 0
    scripted(sc, ts)
    ts.updatePrecondMtrAndFactorize()
    return sc, ep, n, ts


def restate(ts, dup, verts, fixed):
    """the restatement on the handle's own operators and positions: (A0, the coarse apply, live)"""
    Z, cen, live, w = CR.build_z(ts.getResult(), dup, verts, fixed)
    A0 = CR.coarse_matrix(Z, live, ts.multiply)
    return A0, CR.coarse_apply(Z, A0), live


def shared(name):
    """one handle per shape for the tests that leave it as they found it (mode off, default read-back interval), with the
    restatement at its state, computed once"""
    if name not in _cache:
        sc, ep, n, ts = two_steps_in(name)
        nV = sc.V_rest.shape[0]
        dup = R.dup_of(sc.T, ep, nV)
        verts = part_verts(sc.T, ep, n)
        fixed = np.asarray(sc.fixed, dtype=bool)
        A0, apply, live = restate(ts, dup, verts, fixed)
        assert live.all() and apply is not None
        b = -ts.computeGradient(ts.getResult())
        _cache[name] = dict(sc=sc, n=n, ts=ts, dup=dup, verts=verts, fixed=fixed, A0=A0, apply=apply, b=b,
                            Ms=R.m_sym(ts.applyPrecond, dup))
    return _cache[name]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_handles():
    yield
    for S in _cache.values():
        S["ts"].close()
    _cache.clear()


def random_free(fixed, seed):
    v = np.random.default_rng(seed).standard_normal((fixed.size, 3))
    v[fixed] = 0.0
    return v


# ---- 1. A0 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_coarse_matrix_is_zt_h_z_and_two_builds_are_bit_identical(name):
    S = shared(name)
    ts = S["ts"]
    try:
        ts.setPCGCoarse(1)
        builds0 = ts.pcgCoarseInfo()[3]
        ts.pcgApplyPrecond(random_free(S["fixed"], 0))         # the first use after switching on builds
        A0 = ts.pcgCoarseMatrix()
        dim, dropped, active, builds = ts.pcgCoarseInfo()
        assert (dim, dropped, active, builds) == (6 * S["n"], 0, 1, builds0 + 1) and A0.shape == (dim, dim)
        err = np.abs(A0 - S["A0"]).max() / np.abs(S["A0"]).max()
        print(f"{name}: nc {dim}, cond(A0) {np.linalg.cond(A0):.1e}, device against the restatement {err:.2e}")
        assert err <= 1e-12
        assert np.array_equal(A0, A0.T)
        ts.pcgApplyPrecond(random_free(S["fixed"], 0))         # nothing refreshed: no build
        assert ts.pcgCoarseInfo()[3] == builds0 + 1
        ts.updatePrecondMtrAndFactorize()                       # the same H once more: stale, rebuilt, the same bits
        ts.pcgApplyPrecond(random_free(S["fixed"], 0))
        assert ts.pcgCoarseInfo()[3] == builds0 + 2
        assert np.array_equal(ts.pcgCoarseMatrix(), A0)
    finally:
        ts.setPCGCoarse(0)


# ---- 2. one application -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_one_application_matches_the_restatement_and_is_m_sym_when_off(name):
    """1e-10 of the largest entry, the project's bound for an application.  With the mode off the entry gives M_sym: the same
    bits before the mode is switched on and after it has been switched off again; against the restated M_sym, which rounds
    differently (sqrt(dup) (.) the block solve of r / sqrt(dup)), to the application's bound"""
    S = shared(name)
    ts = S["ts"]
    r = random_free(S["fixed"], 11)
    off = ts.pcgApplyPrecond(r)
    want_off = S["Ms"](r)
    assert np.abs(off - want_off).max() <= 1e-10 * np.abs(want_off).max()
    try:
        ts.setPCGCoarse(1)
        on = ts.pcgApplyPrecond(r)
        want = want_off + S["apply"](r)
        err = np.abs(on - want).max() / np.abs(want).max()
        print(f"{name}: application against the restatement {err:.2e}; the coarse term is {np.abs(on - off).max() / np.abs(on).max():.2e} of it")
        assert err <= 1e-10
        assert np.array_equal(ts.pcgApplyPrecond(r), on)
        assert np.array_equal(on[S["fixed"]], off[S["fixed"]])   # w = 0 on fixed vertices: the coarse term adds nothing there
    finally:
        ts.setPCGCoarse(0)
    assert np.array_equal(ts.pcgApplyPrecond(r), off)


# ---- 3. the solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_solve_with_the_coarse_term(name):
    S = shared(name)
    ts, b = S["ts"], S["b"]
    u0, it0, res0 = ts.solveHessian(b, 1e-8, 500)               # the mode off
    try:
        ts.setPCGCoarse(1)
        u, it, res = ts.solveHessian(b, 1e-8, 500)
        assert ts.last_solve_status == 0 and ts.pcgCoarseInfo()[2] == 1
        true = np.linalg.norm(b - ts.multiply(u)) / np.linalg.norm(b)
        M = CR.precond(S["Ms"], S["apply"])
        _, it_ref, res_ref, state = R.pcg(ts.multiply, M, b, 1e-8, 500)
        print(f"{name}: {it0} -> {it} iterations (restatement {it_ref}), recursive {res:.3e}, true {true:.3e}")
        assert state == 1 and abs(it - it_ref) <= 1
        assert res <= 1e-8 and true <= 2e-8
        u2, it2, res2 = ts.solveHessian(b, 1e-8, 500)
        assert np.array_equal(u2, u) and (it2, res2) == (it, res)
        for every in (1, 4, 8):
            ts.setPCG(1e-3, 500, every)
            ue, ite, rese = ts.solveHessian(b, 1e-8, 500)
            assert np.array_equal(ue, u) and (ite, rese) == (it, res), every
        if name == BAR32:
            assert it <= 0.7 * it0
    finally:
        ts.setPCG(1e-3, 500, 8)
        ts.setPCGCoarse(0)
    u1, it1, res1 = ts.solveHessian(b, 1e-8, 500)
    assert np.array_equal(u1, u0) and (it1, res1) == (it0, res0)


# ---- 4. off means untouched ---------------------------------------------------------------------------------------------------------------
def test_a_handle_that_enabled_and_disabled_the_mode_solves_like_one_that_never_did():
    sc, ep, n, never = two_steps_in(BAR4)
    _, _, _, once = two_steps_in(BAR4)
    b = -never.computeGradient(never.getResult())
    once.setPCGCoarse(1)
    u_on, it_on, _ = once.solveHessian(b, 1e-8, 500)
    once.setPCGCoarse(0)
    assert once.pcgCoarseInfo()[:3] == (0, 0, 0)
    u1, it1, res1 = once.solveHessian(b, 1e-8, 500)
    u0, it0, res0 = never.solveHessian(b, 1e-8, 500)
    assert never.pcgCoarseInfo() == (0, 0, 0, 0)
    assert np.array_equal(u1, u0) and (it1, res1) == (it0, res0)
    assert not np.array_equal(u_on, u0)
    never.close()
    once.close()


# ---- 5. steps -----------------------------------------------------------------------------------------------------------------------------
def test_steps_on_four_subdomains_with_the_coarse_term_match_the_oracles_exact_newton():
    sc, ep, n = load_workload(BAR4)
    assert n == 4
    cfg = sc.cfg
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG)
    ts.setPCG(1e-10, 500, 4)
    ts.setPCGCoarse(1)
    one = np.zeros(sc.T.shape[0], dtype=np.int32)
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, one, 1, cfg.with_gravity)
    solves = total = builds = 0
    for k in range(3):
        scripted(sc, ts, orc)
        st, so = ts.step(), orc.step_newton()
        ns, ni, last, lres = ts.pcgInfo()
        dim, dropped, active, nb = ts.pcgCoarseInfo()
        print(f"step {k}: Newton iterations {st.iters} / {so.iters}, halvings {st.ls_halvings} / {so.ls_halvings}, "
              f"{ni - total} CG iterations in {ns - solves} solves, {nb - builds} coarse builds")
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
        assert ns - solves == st.iters and nb - builds == st.iters, k      # one solve and one build per Newton iteration
        assert st.backsolve_launches == ni - total, k
        assert (dim, dropped, active) == (24, 0, 1) and lres <= 1e-10
        solves, total, builds = ns, ni, nb
    ts.close()
    orc.close()


# ---- 6. staleness -------------------------------------------------------------------------------------------------------------------------
def test_refix_and_set_time_step_mark_the_coarse_matrix_stale():
    sc, ep, n, ts = two_steps_in(BAR4)
    nV = sc.V_rest.shape[0]
    dup, verts = R.dup_of(sc.T, ep, nV), part_verts(sc.T, ep, n)
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    ts.setPCGCoarse(1)

    def solve_and_compare(what, builds_want):
        fx = fixed.astype(bool)
        b = random_free(fx, 21)
        u, it, res = ts.solveHessian(b, 1e-8, 500)
        assert ts.last_solve_status == 0
        assert np.linalg.norm(b - ts.multiply(u)) <= 2e-8 * np.linalg.norm(b)
        dim, dropped, active, builds = ts.pcgCoarseInfo()
        assert (dropped, active, builds) == (0, 1, builds_want), what
        A0_ref, _, _ = restate(ts, dup, verts, fx)
        A0 = ts.pcgCoarseMatrix()
        err = np.abs(A0 - A0_ref).max() / np.abs(A0_ref).max()
        print(f"{what}: build {builds}, {it} iterations, A0 against the restatement {err:.2e}")
        assert err <= 1e-12, what
        return A0

    A_first = solve_and_compare("first solve", 1)
    solve_and_compare("second solve, nothing refreshed", 1)
    free = np.flatnonzero(fixed == 0)
    fixed[free[:5]] = 1                                          # five more fixed vertices: other weights, another H
    ts.refix(fixed)
    A_refix = solve_and_compare("after dotmi_refix", 2)
    assert not np.array_equal(A_refix, A_first)
    ts.setTime(sc.cfg.duration, 0.5 * sc.cfg.dt)
    A_dt = solve_and_compare("after dotmi_set_time_step", 3)
    assert not np.array_equal(A_dt, A_refix)
    ts.close()


# ---- 7. a dropped subdomain ---------------------------------------------------------------------------------------------------------------
def test_subdomain_without_free_vertices_is_dropped_and_the_solve_converges():
    sc, ep, n, ts = two_steps_in(BAR4)
    nV = sc.V_rest.shape[0]
    dup, verts = R.dup_of(sc.T, ep, nV), part_verts(sc.T, ep, n)
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed[verts[0]] = 1
    ts.refix(fixed)
    ts.setPCGCoarse(1)
    fx = fixed.astype(bool)
    b = random_free(fx, 31)
    u, it, res = ts.solveHessian(b, 1e-8, 500)
    true = np.linalg.norm(b - ts.multiply(u)) / np.linalg.norm(b)
    dim, dropped, active, builds = ts.pcgCoarseInfo()
    print(f"subdomain 0 fixed: {it} iterations, true residual {true:.3e}, dropped {dropped}, active {active}")
    assert ts.last_solve_status == 0 and true <= 2e-8
    assert (dim, dropped, active, builds) == (24, 1, 1, 1)
    A0 = ts.pcgCoarseMatrix()
    A0_ref, apply, live = restate(ts, dup, verts, fx)
    assert list(live) == [False, True, True, True] and apply is not None
    assert np.array_equal(A0[:6, :6], np.eye(6)) and not A0[:6, 6:].any() and not A0[6:, :6].any()
    assert np.abs(A0 - A0_ref).max() <= 1e-12 * np.abs(A0_ref).max()
    _, it_ref, _, state = R.pcg(ts.multiply, CR.precond(R.m_sym(ts.applyPrecond, dup), apply), b, 1e-8, 500)
    assert state == 1 and abs(it - it_ref) <= 1
    ts.close()


# ---- 8. refusals and the runner -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag,word", [(dl.FLAG_LBFGS_PD, "LBFGS-PD"), (dl.FLAG_LBFGS_HI, "LBFGS-HI"), (dl.FLAG_GSDD, "GSDD")])
def test_mode_is_refused_on_handles_without_the_global_solve(flag, word):
    sc, ep, n = load_workload(BAR4)
    whole = flag != dl.FLAG_GSDD
    ts = DOTTimeStepper(sc, None if whole else ep, 1 if whole else n, flags=flag, alpha_min=1.0 if whole else 0.1)
    with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse.*" + word):
        ts.setPCGCoarse(1)
    with pytest.raises(DotmiError, match="dotmi_pcg_apply_precond.*" + word):
        ts.pcgApplyPrecond(np.ones((sc.V_rest.shape[0], 3)))
    assert ts.pcgCoarseInfo() == (0, 0, 0, 0)
    ts.close()


def test_mode_is_refused_on_a_sharded_handle():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_FORCE_DIST)
    with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse.*single-rank"):
        ts.setPCGCoarse(1)
    ts.close()


def test_mode_is_refused_on_a_vertex_partition_for_other_values_and_bad_arguments():
    sc, ep, n = load_workload(BAR4)
    vpart = np.full(sc.V_rest.shape[0], n, dtype=np.int32)      # a vertex goes to the lowest subdomain among its elements
    np.minimum.at(vpart, np.asarray(sc.T).ravel(), np.repeat(ep, 4))
    ts = DOTTimeStepper(sc, None, n, vpart=vpart)
    with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse.*vpart"):
        ts.setPCGCoarse(1)
    ts.close()
    ts = DOTTimeStepper(sc, ep, n)
    for mode in (2, -1):
        with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse: mode"):
            ts.setPCGCoarse(mode)
    with pytest.raises(DotmiError, match="dotmi_pcg_coarse_matrix"):
        ts.pcgCoarseMatrix()                                     # nothing assembled yet
    L = dl.load()
    r = np.ones((sc.V_rest.shape[0], 3))
    assert L.dotmi_pcg_apply_precond(ts._h, None, dl.dp(r)) == -1 and L.dotmi_pcg_apply_precond(ts._h, dl.dp(r), None) == -1
    ts.setPCGCoarse(1)
    ts.pcgApplyPrecond(r)
    assert L.dotmi_pcg_coarse_matrix(ts._h, 24 * 24 - 1, dl.dp(np.zeros(24 * 24))) == -1
    ts.close()


def test_mode_is_refused_above_256_subdomains():
    """257 subdomains (nc would be 1542): refused with a message; switching off is always accepted"""
    sc, ep, n = load_workload("synbar:40x3x3:257")
    assert n == 257 and np.unique(ep).size == 257
    ts = DOTTimeStepper(sc, ep, n)
    with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse: at most 256 subdomains"):
        ts.setPCGCoarse(1)
    ts.setPCGCoarse(0)
    ts.close()


def test_headless_runner_takes_pcg_coarse(tmp_path):
    """dot_hip --newton-pcg 4 --pcg-coarse: per frame the iterations, halvings and energy of the Python-driven stepper with the mode
    on, on the same partition; the flag alone is refused"""
    from tests.test_host_logic import _write_msh
    from tests.workloads import MESH_DIR
    from dot_amd import scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    (tmp_path / "bunny.txt").write_text("energy FCR\ntimeStepper Newton\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\n"
                                        "stiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n")
    out = subprocess.check_output([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--frames", "2",
                                   "--newton-pcg", "4", "--pcg-coarse", "--no-files"], timeout=600).decode()
    frames = [l.split() for l in out.splitlines() if l.startswith("FRAME")]
    assert len(frames) == 2
    sc, _, _ = load_workload(BUNNY)
    ts = DOTTimeStepper(sc, None, 4, flags=dl.FLAG_NEWTON_PCG, alpha_min=1.0)
    ts.setPCGCoarse(1)
    for k in range(2):
        assert ts.solve(1) == 0
        assert int(frames[k][5]) == ts.last_stats.iters, k
        assert int(frames[k][7]) == ts.last_stats.ls_halvings, k
        assert abs(float(frames[k][9]) - ts.last_stats.E) <= 1e-12 * abs(ts.last_stats.E), k
    ns, ni, _, _ = ts.pcgInfo()
    dim, dropped, active, builds = ts.pcgCoarseInfo()
    assert f"PCG coarse space: dimension {dim}, {dropped} dropped, active {active}, {builds} builds, {ni} CG iterations in {ns} solves" in out
    assert (dim, active) == (24, 1) and builds == ns
    ts.close()
    bad = subprocess.run([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--pcg-coarse", "--dump-scene", "0"],
                         capture_output=True, timeout=600)
    assert bad.returncode == 1 and b"--pcg-coarse" in bad.stderr
