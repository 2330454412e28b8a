"""Newton-PCG, host only: the two facts the design rests on, checked on the oracle's operators (DOT's block solve is not symmetric, its
symmetric scaling is; the single-reduction recurrences of tests/pcg_reference.py reach the tolerance with a true residual to match),
and the new ABI entries' presence and argument checks (no device is touched)."""
import ctypes as C
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import oracle_py as O
from tests import pcg_reference as R

MESHES = ["synbar:16x5x5:4", "bunny5K_LTSS"]
_states = {}


def oracle_state(name):
    """the oracle two DOT steps into the script, the handles moved for the third, refactored there: (sc, orc, dup, free, b = -g)"""
    if name not in _states:
        sc, ep, n = load_workload(name)
        cfg = sc.cfg
        orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)
        for _ in range(2):
            idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
            orc.move(idx, pos)
            assert orc.step().status == 0
        idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
        orc.move(idx, pos)
        x = orc.state()[0]
        orc.refactor(x)
        dup = orc.dup()
        assert np.array_equal(dup, R.dup_of(sc.T, ep, sc.V_rest.shape[0]))
        free = ~np.asarray(sc.fixed, dtype=bool)
        _states[name] = (sc, orc, dup, free, -orc.gradient(x), n)
    return _states[name]


def random_free(free, seed):
    v = np.random.default_rng(seed).standard_normal((free.size, 3))
    v[~free] = 0.0
    return v


@pytest.mark.parametrize("name,maxdup", [("synbar:16x5x5:4", 2), ("bunny5K_LTSS", 5)])
def test_scaled_block_solve_is_the_sum_of_the_subdomain_solves_scaled_on_both_sides(name, maxdup):
    """sqrt(dup) (.) apply_precond(r / sqrt(dup)) against D^-1/2 (sum_s R_s^T H_s^-1 R_s) D^-1/2 r built from the oracle's dense
    subdomain matrices: 1e-10 of the largest entry"""
    sc, orc, dup, free, _, n = oracle_state(name)
    assert dup.min() == 1 and dup.max() == maxdup
    r = random_free(free, 0)
    got = R.m_sym(orc.apply_precond, dup)(r)
    isd = 1.0 / np.sqrt(dup)[:, None]
    q = r * isd
    S = np.zeros_like(r)
    for p in range(n):
        vs = orc.part_verts(p)
        S[vs] += np.linalg.solve(orc.part_dense(p), q[vs].ravel()).reshape(-1, 3)
    want = S * isd
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("name", MESHES)
def test_scaling_makes_the_block_solve_symmetric_and_dots_own_is_not(name):
    sc, orc, dup, free, _, _ = oracle_state(name)
    a, b = random_free(free, 1), random_free(free, 2)
    Ms = R.m_sym(orc.apply_precond, dup)
    ab, ba = np.vdot(a, Ms(b)), np.vdot(b, Ms(a))
    print(f"{name}: M_sym asymmetry {abs(ab - ba) / abs(ab):.2e}")
    assert abs(ab - ba) <= 1e-12 * abs(ab)
    ab, ba = np.vdot(a, orc.apply_precond(b)), np.vdot(b, orc.apply_precond(a))
    print(f"{name}: DOT's block solve, asymmetry {abs(ab - ba) / abs(ab):.2e}")
    assert abs(ab - ba) > 1e-3 * abs(ab)


@pytest.mark.parametrize("name", MESHES)
def test_restatement_reaches_the_tolerance_with_the_true_residual(name):
    """rel_tol 1e-8: converged, the recursive residual within the tolerance and the true one |b - H u| / |b| <= 2e-8"""
    sc, orc, dup, free, b, _ = oracle_state(name)
    u, it, res, state = R.pcg(orc.spmv, R.m_sym(orc.apply_precond, dup), b, 1e-8, 500)
    true = np.linalg.norm(b - orc.spmv(u)) / np.linalg.norm(b)
    print(f"{name}: {it} iterations, recursive {res[-1]:.3e}, true {true:.3e}")
    assert state == 1 and 0 < it < 200 and len(res) == it + 1
    assert res[-1] <= 1e-8 and true <= 2e-8
    assert np.abs(u[~free]).max() == 0.0          # b is zero on the fixed vertices and H is the identity there


def test_restatement_edges():
    A = np.diag([1.0, 2.0, 4.0])
    mul = lambda v: A @ v                                          # noqa: E731
    ident = lambda v: v                                            # noqa: E731
    u, it, res, state = R.pcg(mul, ident, np.zeros(3), 1e-8, 10)
    assert (it, state, res) == (0, 1, [0.0]) and not u.any()
    u, it, res, state = R.pcg(mul, ident, np.ones(3), 1e-12, 10)   # three distinct eigenvalues: three iterations
    assert (it, state) == (3, 1) and np.allclose(A @ u, 1.0, atol=1e-12)
    u, it, res, state = R.pcg(mul, ident, np.ones(3), 1e-12, 2)
    assert (it, state) == (2, 0) and len(res) == 3
    u, it, res, state = R.pcg(lambda v: -(A @ v), ident, np.ones(3), 1e-12, 10)   # negative curvature: breakdown, nothing divided
    assert (it, state) == (0, 2) and not u.any()


def test_new_entries_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    for name in ("dotmi_solve_hessian", "dotmi_set_pcg", "dotmi_pcg_info"):
        assert name in dl.EXPORTS and f"int {name}(" in header, name
        assert hasattr(dl.load(), name), name
    assert dl.FLAG_NEWTON_PCG == 2048 and "#define DOTMI_FLAG_NEWTON_PCG 2048" in header


def test_entries_reject_a_null_handle_without_a_device():
    L = dl.load()
    buf = np.zeros(3)
    it, res = C.c_int32(), C.c_double()
    assert L.dotmi_solve_hessian(None, dl.dp(buf), dl.dp(buf), 1e-8, 10, C.cast(C.byref(it), dl.c_ip),
                                 C.cast(C.byref(res), dl.c_dp)) == -1
    assert L.dotmi_set_pcg(None, 1e-3, 500, 4) == -1
    assert L.dotmi_pcg_info(None, None, None, None, None) == -1
