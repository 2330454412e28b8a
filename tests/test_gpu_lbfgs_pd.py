"""LBFGS-PD (DOTMI_FLAG_LBFGS_PD; `timeStepper LBFGS`, LBFGSTimeStepper with D0T_PD): L-BFGS whose initial inverse Hessian is the
constant projective-dynamics Laplacian L = M + sum_e dt^2 vol_e (2 mu_e + lambda_e) D_e^T D_e, fixed rows / columns replaced by the
identity (LBFGSTimeStepper.cpp:113-194), applied per coordinate, factored once per create / refix on the GPU."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.scene import lame
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import oracle_py as O

pytestmark = pytest.mark.gpu


def dense_L(ts, sc, fixed, mu=None, lam=None):
    """L from the handle's own features (restTriInv A, volumes, lumped mass) and the formula above, in numpy; mu / lam: optional
    per-element Lame parameters (nT,), else the scene's one material"""
    A, vol, mass = ts.features()
    A = A.reshape(-1, 3, 3)
    mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
    nT = sc.T.shape[0]
    mu = np.full(nT, mu0) if mu is None else np.asarray(mu, dtype=np.float64)
    lam = np.full(nT, lam0) if lam is None else np.asarray(lam, dtype=np.float64)
    nV = sc.V_rest.shape[0]
    L = np.diag(mass.astype(np.float64))
    Le = np.zeros((nV, nV))
    for e, t in enumerate(sc.T):
        D = np.zeros((3, 4))
        D[:, 1:] = A[e].T
        D[:, 0] = -A[e].sum(axis=0)
        Le[np.ix_(t, t)] += sc.cfg.dt ** 2 * vol[e] * (2 * mu[e] + lam[e]) * (D.T @ D)
    L = L + Le
    f = np.asarray(fixed, dtype=bool)
    L[f, :] = 0.0
    L[:, f] = 0.0
    L[f, f] = 1.0
    return L


def make_pd(sc, energy=None, flags=0, mu=None, lam=None):
    return DOTTimeStepper(sc, None, 1, energy=energy, alpha_min=1.0, flags=dl.FLAG_LBFGS_PD | flags, mu=mu, lam=lam)


def check_apply(ts, L, seed=0):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((L.shape[0], 3))
    z = ts.applyPrecond(r).reshape(-1, 3)
    ref = np.linalg.solve(L, r)
    for d in range(3):
        assert np.abs(z[:, d] - ref[:, d]).max() <= 1e-10 * np.abs(ref[:, d]).max(), d


@pytest.mark.parametrize("name", ["synbar:16x5x5:1", "bunny5K_LTSS"])
def test_apply_is_the_dense_solve_per_coordinate(name):
    sc, _, _ = load_workload(name)
    ts = make_pd(sc)
    L = dense_L(ts, sc, sc.fixed)
    check_apply(ts, L)
    ts.close()


class DenseSolver:
    """the oracle's external solver for its one subdomain: factor ignores the Hessian blocks, solve applies L^-1 per coordinate"""

    def __init__(self, L):
        self.Linv = np.linalg.inv(L)
        self.CREATE = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte))
        self.FACTOR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))
        self.SOLVE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double))
        self.DESTROY = C.CFUNCTYPE(None, C.c_void_p)
        n = L.shape[0]

        def create(nv, p, i, f):
            assert nv == n
            return 1

        def solve(hd, b):
            a = np.ctypeslib.as_array(b, shape=(3 * n,)).reshape(n, 3)
            a[:] = self.Linv @ a

        self.cbs = (self.CREATE(create), self.FACTOR(lambda hd, blocks: 0), self.SOLVE(solve), self.DESTROY(lambda hd: None))
        self.api = O.ExtSolverAPI(*(C.cast(c, C.c_void_p) for c in self.cbs))

    def bind(self, orc):
        L = O.lib()
        L.dor_use_ext_solver.argtypes = [C.c_void_p, C.c_void_p]
        L.dor_use_ext_solver.restype = C.c_int
        assert L.dor_use_ext_solver(orc.h, C.byref(self.api)) == 0


def oracle_for(sc, energy_id, mu=None, lam=None):
    ep = np.zeros(sc.T.shape[0], dtype=np.int32)
    cfg = sc.cfg
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, energy_id, cfg.dt, sc.fixed, sc.x0, ep, 1, cfg.with_gravity,
                      mu=mu, lam=lam)
    orc.set_alpha_min(1.0)
    return orc


@pytest.mark.parametrize("name,energy,nsteps", [("synbar:16x5x5:1", dl.ENERGY_FCR, 4), ("synbar:16x5x5:1", dl.ENERGY_SNH, 4),
                                                 ("bunny5K_LTSS", dl.ENERGY_FCR, 2)])
def test_steps_match_the_oracle_with_the_laplacian(name, energy, nsteps):
    sc, _, _ = load_workload(name)
    ts = make_pd(sc, energy=energy)
    sol = DenseSolver(dense_L(ts, sc, sc.fixed))
    orc = oracle_for(sc, energy)
    sol.bind(orc)
    for k in range(nsteps):
        x = ts.getResult()
        idx, pos = sc.scripter.step(x, sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        orc.move(idx, pos)
        st, so = ts.step(), orc.step()
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        # no refresh inside or at the end of a PD step
        assert st.ms_hessian == 0.0 and st.ms_factor == 0.0, k
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
    ts.close()
    orc.close()


def test_per_element_materials_weight_the_laplacian():
    """L's element weights dt^2 vol_e (2 mu_e + lambda_e) with a random Lame field per element (tests/materials.py): the apply
    is the dense solve of that L, and 2 steps take the oracle's iterations with a dense L^-1 of the same field"""
    from tests.materials import field
    sc, _, _ = load_workload("bunny5K_LTSS")
    mu, lam = field(sc, "random")
    ts = make_pd(sc, mu=mu, lam=lam)
    L = dense_L(ts, sc, sc.fixed, mu, lam)
    check_apply(ts, L)
    # (and the field matters: the one-material L is another matrix)
    assert np.abs(L - dense_L(ts, sc, sc.fixed)).max() > 1e-3 * np.abs(L).max()
    sol = DenseSolver(L)
    orc = oracle_for(sc, sc.cfg.energy_id, mu, lam)
    sol.bind(orc)
    for k in range(2):
        st, so = _scripted_step(sc, ts, orc)
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
    ts.close()
    orc.close()


def test_scalar_factor_is_at_most_a_sixth_of_the_lbfgs_h_factor():
    sc, _, _ = load_workload("bunny5K_LTSS")
    pd = make_pd(sc)
    h = DOTTimeStepper(sc, np.zeros(sc.T.shape[0], dtype=np.int32), 1, alpha_min=1.0)
    L = dl.load()
    b_pd, b_h = L.dotmi_factor_storage_bytes(pd._h), L.dotmi_factor_storage_bytes(h._h)
    assert 0 < b_pd <= b_h / 6, (b_pd, b_h)
    pd.close()
    h.close()


def _scripted_step(sc, ts, orc):
    x = ts.getResult()
    idx, pos = sc.scripter.step(x, sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    orc.move(idx, pos)
    return ts.step(), orc.step()


def test_refix_rebuilds_the_laplacian():
    """dotmi_refix (LBFGSTimeStepper::updatePrecondMtrAndFactorize, :266-270) rebuilds L for the new fixed set and refactors it:
    the apply is the dense solve of the NEW L, and the next step takes the oracle's iterations with a dense L^-1 of the new set"""
    sc, _, _ = load_workload("synbar:16x5x5:1")
    ts = make_pd(sc)
    sol = DenseSolver(dense_L(ts, sc, sc.fixed))
    orc = oracle_for(sc, sc.cfg.energy_id)
    sol.bind(orc)
    st, so = _scripted_step(sc, ts, orc)          # one step on the first factor
    assert (st.iters, st.ls_halvings) == (so.iters, so.ls_halvings)
    fixed = np.array(sc.fixed, dtype=np.uint8).copy()
    xs = np.unique(sc.V_rest[:, 0])
    fixed[sc.V_rest[:, 0] == xs[len(xs) // 2]] = 1   # pin the middle cross-section as well (the script holds both ends)
    assert (fixed != np.asarray(sc.fixed, dtype=np.uint8)).any()
    ts.refix(fixed)
    L2 = dense_L(ts, sc, fixed)
    check_apply(ts, L2, seed=1)
    sol.Linv = np.linalg.inv(L2)                  # the oracle's callback solves with the new set's L ...
    orc.set_fixed(fixed)                          # ... from here on (its refresh rebuilds the external solver)
    for k in range(2):
        st, so = _scripted_step(sc, ts, orc)
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.ms_hessian == 0.0 and st.ms_factor == 0.0
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
    ts.close()
    orc.close()


@pytest.mark.parametrize("extra", [dl.FLAG_GSDD, dl.FLAG_NEWTON, dl.FLAG_FORCE_DIST, dl.FLAG_ASYNC_REFRESH, dl.FLAG_OWNER_EXCHANGE])
def test_rejected_combinations(extra):
    sc, _, _ = load_workload("synbar:16x5x5:1")
    with pytest.raises(DotmiError):
        make_pd(sc, flags=extra)


def test_rejects_a_vertex_partition():
    sc, _, _ = load_workload("synbar:16x5x5:1")
    with pytest.raises(DotmiError):
        DOTTimeStepper(sc, None, 1, flags=dl.FLAG_LBFGS_PD, vpart=np.zeros(sc.V_rest.shape[0], dtype=np.int32))


def test_block_solve_entries_are_refused():
    sc, _, _ = load_workload("synbar:16x5x5:1")
    ts = make_pd(sc)
    L = dl.load()
    n = 3 * sc.V_rest.shape[0]
    buf = np.zeros(n)
    pp = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dotmi_refactor(ts._h, None) == -1      # DOTMI_E_INVALID
    assert L.dotmi_spmv(ts._h, pp, pp) == -1
    assert L.dotmi_part_size(ts._h, 0) == -1
    ts.close()


def test_headless_runner_takes_lbfgs_pd(tmp_path):
    """`timeStepper LBFGS` in a reference-format script: dot_hip runs LBFGS-PD on the whole mesh -- per frame the iterations and
    energy of the Python-driven PD stepper --, and writes the run's files but no partition files (label.obj / wire.poly come
    from the ADMMDD constructor only)"""
    import os
    import subprocess
    from tests.test_host_logic import _write_msh
    from tests.workloads import MESH_DIR
    from dot_amd import scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    (tmp_path / "bunny.txt").write_text("energy FCR\ntimeStepper LBFGS\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\n"
                                        "stiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n")
    out = subprocess.check_output([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--frames", "3",
                                   "--out", str(tmp_path / "out")], timeout=600).decode()
    frames = [l.split() for l in out.splitlines() if l.startswith("FRAME")]
    assert len(frames) == 3
    sc, _, _ = load_workload("bunny5K_LTSS")
    ts = make_pd(sc)
    for k in range(3):
        assert ts.solve(1) == 0
        assert int(frames[k][5]) == ts.last_stats.iters, k
        assert int(frames[k][7]) == ts.last_stats.ls_halvings, k
        assert abs(float(frames[k][9]) - ts.last_stats.E) <= 1e-12 * abs(ts.last_stats.E), k
    ts.close()
    o = tmp_path / "out"
    for f in ("iterStats.txt", "log.txt", "info.txt", "status0", "status2", "0.obj", "2.obj"):
        assert (o / f).exists(), f
    assert not (o / "label.obj").exists() and not (o / "wire.poly").exists()
