"""Newton-PCG (DOTMI_FLAG_NEWTON_PCG, dotmi_solve_hessian; dot_amd/csrc/k_pcg.hip, dotmi_pcg.hip): conjugate gradients on the global
projected Hessian, preconditioned with the symmetric scaling of the block solve.  The solve against the handle's own dotmi_spmv and
against the numpy restatement (tests/pcg_reference.py) driven by the same handle's operators; its edges; Newton steps on several
subdomains against the oracle's exact one-subdomain Newton and against the device's own; refusals; the runner."""
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import oracle_py as O
from tests import pcg_reference as R

pytestmark = pytest.mark.gpu

BAR, BUNNY = "synbar:16x5x5:4", "bunny5K_LTSS"


def scripted(sc, ts, orc=None):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    if orc is not None:
        orc.move(idx, pos)


def handle_two_steps_in(name, **kw):
    """a DOT handle two steps into the script, the handles moved for the third, refactored there: (sc, ts, dup, b = -g)"""
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n, **kw)
    for _ in range(2):
        scripted(sc, ts)
        assert ts.step().status == 0
    scripted(sc, ts)
    ts.updatePrecondMtrAndFactorize()
    b = -ts.computeGradient(ts.getResult())
    return sc, ts, R.dup_of(sc.T, ep, sc.V_rest.shape[0]), b


# ---- 1. the solve ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,two_level", [(BAR, False), (BUNNY, False), (BUNNY, True)])
def test_solve_reaches_the_tolerance_like_the_restatement_and_repeats_bit_for_bit(name, two_level, monkeypatch):
    if two_level:
        monkeypatch.setenv("DOTMI_TWO_LEVEL", "1")
    sc, ts, dup, b = handle_two_steps_in(name)
    assert ts.backsolveForm() == int(two_level)
    assert dup.max() == (2 if name == BAR else 5)
    u, it, res = ts.solveHessian(b, 1e-8, 500)
    assert ts.last_solve_status == 0
    true = np.linalg.norm(b - ts.multiply(u)) / np.linalg.norm(b)
    _, it_ref, res_ref, state = R.pcg(ts.multiply, R.m_sym(ts.applyPrecond, dup), b, 1e-8, 500)
    print(f"{name} two-level {two_level}: {it} iterations (restatement {it_ref}), recursive {res:.3e}, true {true:.3e}")
    assert state == 1 and abs(it - it_ref) <= 1
    assert res <= 1e-8 and true <= 2e-8
    u2, it2, res2 = ts.solveHessian(b, 1e-8, 500)
    assert np.array_equal(u2, u) and (it2, res2) == (it, res)
    # a batch boundary must not move u: the default read-back every 8 iterations above, here every 4 and after every iteration
    for every in (1, 4):
        ts.setPCG(1e-3, 500, every)
        ue, ite, rese = ts.solveHessian(b, 1e-8, 500)
        assert np.array_equal(ue, u) and (ite, rese) == (it, res), every
    assert ts.pcgInfo() == (4, 4 * it, it, res)
    ts.close()


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------
def test_solve_edges():
    sc, ts, dup, b = handle_two_steps_in(BAR)
    nV = sc.V_rest.shape[0]
    fixed = np.asarray(sc.fixed, dtype=bool)
    # b = 0
    u, it, res = ts.solveHessian(np.zeros((nV, 3)), 1e-8, 500)
    assert ts.last_solve_status == 0 and it == 0 and res == 0.0 and not u.any() and np.isfinite(u).all()
    # b on the fixed vertices only: H is the identity there and couples them to nothing
    bf = np.zeros((nV, 3))
    bf[fixed] = np.random.default_rng(0).standard_normal((int(fixed.sum()), 3))
    u, it, res = ts.solveHessian(bf, 1e-8, 500)
    assert ts.last_solve_status == 0 and it >= 1
    assert np.abs(u - bf).max() <= 1e-14
    # the cap: 2, three iterations, the restatement's third residual
    u, it, res = ts.solveHessian(b, 1e-8, 3)
    _, it_ref, res_ref, state = R.pcg(ts.multiply, R.m_sym(ts.applyPrecond, dup), b, 1e-8, 3)
    assert ts.last_solve_status == 2 and it == 3 == it_ref and state == 0
    print(f"third residual {res:.15e}, restatement {res_ref[3]:.15e}")
    assert abs(res - res_ref[3]) <= 1e-10 * res_ref[3]
    # bad arguments: refused with a message, the settings unchanged
    for tol, cap in ((0.0, 10), (-1.0, 10), (float("nan"), 10), (float("inf"), 10), (1e-8, 0)):
        with pytest.raises(DotmiError, match="dotmi_solve_hessian"):
            ts.solveHessian(b, tol, cap)
    for args in ((0.0, 500, 4), (float("nan"), 500, 4), (1e-3, 0, 4), (1e-3, 500, 0)):
        with pytest.raises(DotmiError, match="dotmi_set_pcg"):
            ts.setPCG(*args)
    L = dl.load()
    assert L.dotmi_solve_hessian(ts._h, None, dl.dp(u), 1e-8, 10, None, None) == -1
    assert L.dotmi_solve_hessian(ts._h, dl.dp(b), None, 1e-8, 10, None, None) == -1
    ts.close()


@pytest.mark.parametrize("name", [BAR, BUNNY])
def test_one_subdomain_is_the_exact_inverse(name):
    """M = H^-1 on one subdomain: one application solves (1e-10: the factors reach 1e-14 on these meshes), the PCG has converged
    after at most 2 iterations at 1e-10.  bunny5K as one subdomain has rows of 14 976 columns: four column chunks of the two-phase
    back-solve kernel (bs_tiles.hpp, BS_LONG_CHUNK)"""
    sc, _, _ = load_workload(name)
    ts = DOTTimeStepper(sc, np.zeros(sc.T.shape[0], dtype=np.int32), 1)
    assert ts.backsolveForm() == 0
    scripted(sc, ts)
    ts.updatePrecondMtrAndFactorize()
    r = np.random.default_rng(0).standard_normal((sc.V_rest.shape[0], 3))
    r[np.asarray(sc.fixed, dtype=bool)] = 0.0
    assert np.linalg.norm(ts.multiply(ts.applyPrecond(r)) - r) <= 1e-10 * np.linalg.norm(r)
    b = -ts.computeGradient(ts.getResult())
    u, it, res = ts.solveHessian(b, 1e-10, 500)
    assert ts.last_solve_status == 0 and 1 <= it <= 2 and res <= 1e-10
    assert np.linalg.norm(b - ts.multiply(u)) <= 2e-10 * np.linalg.norm(b)
    ts.close()


# ---- 3. steps against the oracle ---------------------------------------------------------------------------------------------------
def test_steps_on_four_subdomains_match_the_oracles_exact_newton():
    sc, ep, n = load_workload(BAR)
    assert n == 4
    cfg = sc.cfg
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG)
    ts.setPCG(1e-10, 500, 4)
    one = np.zeros(sc.T.shape[0], dtype=np.int32)
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, one, 1, cfg.with_gravity)
    solves = total = 0
    for k in range(3):
        scripted(sc, ts, orc)
        st, so = ts.step(), orc.step_newton()
        ns, ni, last, lres = ts.pcgInfo()
        print(f"step {k}: Newton iterations {st.iters} / {so.iters}, halvings {st.ls_halvings} / {so.ls_halvings}, "
              f"{ni - total} CG iterations in {ns - solves} solves")
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
        assert ns - solves == st.iters, k                       # one solve per Newton iteration
        assert st.backsolve_launches == ni - total, k            # one block-solve application per CG iteration
        assert lres <= 1e-10
        solves, total = ns, ni
    ts.close()
    orc.close()


# ---- 4. steps against the exact device path ------------------------------------------------------------------------------------------
def test_bunny_steps_match_the_one_subdomain_newton_handle():
    """bunny5K_LTSS / 8 under DOTMI_FLAG_NEWTON_PCG at eta = 1e-10 against a one-subdomain DOTMI_FLAG_NEWTON handle, two steps:
    iterations and halvings identical, positions to 1e-9.
    (The one-subdomain handle of this mesh is the case that showed the chunk count of the two-phase back-solve: bs_tiles.hpp.)"""
    sc, ep, n = load_workload(BUNNY)
    assert n == 8
    # (both handles stop after 50 Newton iterations: the exact method takes 3-4 here, and a handle that does not converge should
    # fail this test in a second, not after the default cap of 10000 iterations)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, iter_cap=50)
    ts.setPCG(1e-10, 500, 4)
    ex = DOTTimeStepper(sc, np.zeros(sc.T.shape[0], dtype=np.int32), 1, flags=dl.FLAG_NEWTON, iter_cap=50)
    for k in range(2):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        ex.setDirichlet(idx, pos)
        st, se = ts.step(), ex.step()
        print(f"step {k}: Newton iterations {st.iters} / {se.iters}, halvings {st.ls_halvings} / {se.ls_halvings}, "
              f"{st.backsolve_launches} block-solve applications")
        assert (st.status, st.iters, st.ls_halvings) == (se.status, se.iters, se.ls_halvings), k
        assert np.abs(ts.getResult() - ex.getResult()).max() < 1e-9, k
    ts.close()
    ex.close()


def test_bunny_steps_match_the_oracles_exact_newton_as_recorded():
    """the same two steps against the ORACLE's exact one-subdomain Newton (dor_step_newton; a minute of CPU per step, so recorded:
    tests/golden/newton_bunny5K.npz, tools/make_newton_golden.py): iterations and halvings identical, positions to 1e-9"""
    sc, ep, n = load_workload(BUNNY)
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_bunny5K.npz"))
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG)
    ts.setPCG(1e-10, 500, 4)
    for k in range(2):
        scripted(sc, ts)
        st = ts.step()
        dx = np.abs(ts.getResult() - rec["x"][k]).max()
        print(f"step {k}: {st.iters} Newton iterations, {st.ls_halvings} halvings, {st.backsolve_launches} applications, max |dx| {dx:.2e}")
        assert (st.status, st.iters, st.ls_halvings) == tuple(rec["stats"][k]), k
        assert dx < 1e-9, k
    ts.close()


def test_bunny_steps_converge_at_the_default_forcing_term():
    sc, ep, n = load_workload(BUNNY)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG)
    for k in range(3):
        scripted(sc, ts)
        st = ts.step()
        print(f"step {k}: {st.iters} Newton iterations, {st.backsolve_launches} block-solve applications, g2 {st.g2:.3e}")
        assert st.status == 0 and st.g2 <= ts.targetGRes, k
        assert st.backsolve_launches >= st.iters
    ts.close()


# ---- 5. refusals and the runner ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [dl.FLAG_FORCE_DIST, dl.FLAG_OWNER_EXCHANGE, dl.FLAG_GSDD, dl.FLAG_NEWTON, dl.FLAG_LBFGS_PD,
                                   dl.FLAG_LBFGS_HI, dl.FLAG_ASYNC_REFRESH])
def test_rejected_combinations(extra):
    sc, ep, n = load_workload(BAR)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG"):
        DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG | extra)


def test_rejects_a_vertex_partition_and_more_than_one_rank():
    sc, ep, n = load_workload(BAR)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG"):
        DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, vpart=np.zeros(sc.V_rest.shape[0], dtype=np.int32))
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG"):
        DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, world=2, rank=0, comm_id=bytes(128))


@pytest.mark.parametrize("flag,word", [(dl.FLAG_LBFGS_PD, "LBFGS-PD"), (dl.FLAG_LBFGS_HI, "LBFGS-HI"), (dl.FLAG_GSDD, "GSDD")])
def test_solve_is_refused_on_handles_without_the_global_solve(flag, word):
    sc, ep, n = load_workload(BAR)
    whole = flag != dl.FLAG_GSDD
    ts = DOTTimeStepper(sc, None if whole else ep, 1 if whole else n, flags=flag, alpha_min=1.0 if whole else 0.1)
    with pytest.raises(DotmiError, match=word):
        ts.solveHessian(np.ones((sc.V_rest.shape[0], 3)), 1e-8, 10)
    ts.close()


def test_headless_runner_takes_newton_pcg(tmp_path):
    """`timeStepper Newton` with --newton-pcg 4: dot_hip runs Newton-PCG on four subdomains of the built-in partitioner -- per frame
    the iterations, halvings and energy of the Python-driven stepper on the same partition -- and writes Newton's files"""
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
                                   "--newton-pcg", "4", "--out", str(tmp_path / "out")], timeout=600).decode()
    assert "4 subdomains" in out
    frames = [l.split() for l in out.splitlines() if l.startswith("FRAME")]
    assert len(frames) == 2
    sc, _, _ = load_workload(BUNNY)
    ts = DOTTimeStepper(sc, None, 4, flags=dl.FLAG_NEWTON_PCG, alpha_min=1.0)
    for k in range(2):
        assert ts.solve(1) == 0
        assert int(frames[k][5]) == ts.last_stats.iters, k
        assert int(frames[k][7]) == ts.last_stats.ls_halvings, k
        assert abs(float(frames[k][9]) - ts.last_stats.E) <= 1e-12 * abs(ts.last_stats.E), k
    ts.close()
    o = tmp_path / "out"
    for f in ("iterStats.txt", "log.txt", "info.txt", "status0", "status1", "0.obj", "1.obj", "label.obj", "wire.poly"):
        assert (o / f).exists(), f
    # the option belongs to Newton scripts
    (tmp_path / "dot.txt").write_text((tmp_path / "bunny.txt").read_text().replace("timeStepper Newton", "timeStepper DOT 4"))
    bad = subprocess.run([exe, "100", str(tmp_path / "dot.txt"), "--mesh-root", str(tmp_path), "--newton-pcg", "4", "--dump-scene", "0"],
                         capture_output=True, timeout=600)
    assert bad.returncode == 1 and b"--newton-pcg" in bad.stderr
