"""Per-element Lame parameters in the oracle (dor_set_lame): the reference reads u / lambda per element in every energy term
(Energy.cpp:411,730,764,990,1014,1042) and takes element 0's for the tolerance (Optimizer.cpp:622-623).  These pin the
oracle's per-element path against its scalar constructor and against its already-pinned element functions, so that the GPU
tests of tests/test_gpu_materials.py have a reference to compare with."""
import ctypes as C

import numpy as np
import pytest

from dot_amd.scene import lame
from tests import oracle_py as O
from tests.materials import KINDS, field
from tests.workloads import load_workload


def _oracle(sc, ep, n, mu=None, lam=None):
    cfg = sc.cfg
    return O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n,
                       cfg.with_gravity, mu=mu, lam=lam)


def _steps(sc, orc, nsteps):
    out = []
    for _ in range(nsteps):
        idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
        orc.move(idx, pos)
        st = orc.step()
        out.append((st.status, st.iters, st.ls_halvings, st.E, st.g2, st.E0, st.g2_0))
    return out


def test_constant_arrays_are_bit_identical_to_the_scalar_constructor():
    runs = []
    for arrays in (False, True):
        sc, ep, n = load_workload("bunny5K_LTSS")
        nT = sc.T.shape[0]
        mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
        orc = _oracle(sc, ep, n, *((np.full(nT, mu0), np.full(nT, lam0)) if arrays else (None, None)))
        tol = orc.target_gres
        rec = _steps(sc, orc, 3)
        x, v, xt = orc.state()
        E = orc.energy(x)
        runs.append((tol, rec, x, v, xt, E, orc.features()[3:]))
        orc.close()
    (t0, r0, x0, v0, xt0, E0, (mu0_, lam0_)), (t1, r1, x1, v1, xt1, E1, (mu1_, lam1_)) = runs
    assert t0 == t1 and r0 == r1 and E0 == E1
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1) and np.array_equal(xt0, xt1)
    assert np.array_equal(mu0_, mu1_) and np.array_equal(lam0_, lam1_)


@pytest.mark.parametrize("kind", KINDS)
def test_fields_are_reproducible_and_per_element(kind):
    sc, _, _ = load_workload("bunny5K_LTSS")
    mu, lam = field(sc, kind, 7)
    mu2, lam2 = field(sc, kind, 7)
    assert np.array_equal(mu, mu2) and np.array_equal(lam, lam2)
    assert mu.shape == lam.shape == (sc.T.shape[0],) and (mu > 0).all() and (lam > 0).all()
    mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
    if kind == "one-off":
        assert (mu[:-1] == mu0).all() and (lam[:-1] == lam0).all() and mu[-1] != mu0 and lam[-1] != lam0
    elif kind == "one-off-first":
        assert (mu[1:] == mu0).all() and (lam[1:] == lam0).all() and mu[0] != mu0 and lam[0] != lam0
    elif kind == "lam-only":
        assert (mu == mu0).all() and np.unique(lam).size > 1
    else:
        assert np.unique(mu).size > 1 and np.unique(lam).size > 1


def _elem_sums(sc, orc, x, mu, lam):
    """dor_eval_energy / _gradient restated from the per-element functions (dor_elem_energy_grad_x) with each element's mu_e,
    lam_e, plus the inertia term m (x - x~) of the free vertices"""
    L = O.lib()
    A, vol, mass, _, _ = orc.features()
    xt = orc.state()[2]
    w = sc.cfg.dt ** 2 * vol
    E = 0.0
    g = np.zeros_like(x)
    ge = np.zeros(12)
    psi = C.c_double()
    for e, t in enumerate(sc.T):
        x4 = np.ascontiguousarray(x[t].ravel())
        Ae = np.ascontiguousarray(A[e])
        L.dor_elem_energy_grad_x(sc.cfg.energy_id, O._dp(x4), O._dp(Ae), float(mu[e]), float(lam[e]), float(w[e]),
                                 C.cast(C.byref(psi), O.c_dp), O._dp(ge))
        E += psi.value
        g[t] += ge.reshape(4, 3)
    E += 0.5 * (mass[:, None] * (x - xt) ** 2).sum()
    g += mass[:, None] * (x - xt)
    g[sc.fixed.astype(bool)] = 0.0
    return E, g


@pytest.mark.parametrize("energy", ["FCR", "SNH"])
@pytest.mark.parametrize("amp", [1e-3, 0.05])
def test_energy_and_gradient_are_the_sums_of_the_element_functions(energy, amp):
    sc, ep, n = load_workload("bunny5K_LTSS")
    sc.cfg.energy = energy
    mu, lam = field(sc, "random", 1)
    orc = _oracle(sc, ep, n, mu, lam)
    x = sc.x0 + amp * np.random.default_rng(2).standard_normal(sc.x0.shape)
    E, g = orc.energy(x), orc.gradient(x)
    Es, gs = _elem_sums(sc, orc, x, mu, lam)
    assert abs(E - Es) <= 1e-12 * abs(Es)
    assert np.abs(g - gs).max() <= 1e-12 * np.abs(gs).max()
    # and the field matters: the scene's one material gives another energy
    mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
    Eu, _ = _elem_sums(sc, orc, x, np.full_like(mu, mu0), np.full_like(lam, lam0))
    assert abs(E - Eu) > 1e-3 * abs(E)
    orc.close()


def test_tolerance_follows_element_0_only():
    sc, ep, n = load_workload("bunny5K_LTSS")
    base = _oracle(sc, ep, n)
    first = _oracle(sc, ep, n, *field(sc, "one-off-first"))
    last = _oracle(sc, ep, n, *field(sc, "one-off"))
    assert last.target_gres == base.target_gres
    assert abs(first.target_gres - base.target_gres) > 1e-3 * base.target_gres
    # the random field's tolerance is that of its element 0's material everywhere
    mu, lam = field(sc, "random", 3)
    rnd = _oracle(sc, ep, n, mu, lam)
    const = _oracle(sc, ep, n, np.full_like(mu, mu[0]), np.full_like(lam, lam[0]))
    assert rnd.target_gres == const.target_gres
    for o in (base, first, last, rnd, const):
        o.close()


def test_set_lame_refreshes_the_factors_at_the_current_positions():
    """dor_set_lame after a step: the preconditioner is that of the new materials at the current x, as a fresh refactor gives"""
    sc, ep, n = load_workload("synbar:8x3x3:4")
    a, b = _oracle(sc, ep, n), _oracle(sc, ep, n)
    _steps(sc, a, 1)
    b.set_state(*a.state()[:2])
    mu, lam = field(sc, "random", 4)
    a.set_lame(mu, lam)
    b.set_lame(mu, lam)
    b.refactor(a.state()[0])
    r = np.random.default_rng(5).standard_normal(sc.x0.shape) * (1 - sc.fixed[:, None])
    assert np.array_equal(a.apply_precond(r), b.apply_precond(r))
    with pytest.raises(ValueError):
        a.set_lame(mu[:-1], lam)
    a.close(); b.close()
