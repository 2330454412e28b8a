"""The rigid-mode coarse term of DOT's block preconditioner (dotmi_set_dot_coarse), host only: the numpy restatement of DOT's step
(tests/dot_coarse_reference.py) against OracleSim.step() without the term, the iteration counts with it, a dropped subdomain and the
inactive fallback, and the new ABI entries' presence and argument checks (no device is touched)."""
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import dot_coarse_reference as DR
from tests import oracle_py as O

BAR4, BAR12, BAR32, BUNNY = "synbar:16x5x5:4", "synbar:48x4x4:12", "synbar:96x4x4:32", "bunny5K_LTSS"
STEPS = 4
_runs = {}


def make_oracle(sc, ep, n):
    cfg = sc.cfg
    return O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)


def gravity(cfg):
    return (0.0, -9.80665 if cfg.with_gravity else 0.0, 0.0)


def restated_run(name, coarse, steps=STEPS):
    """`steps` scripted steps of the restatement on an oracle of its own, without or with the coarse term:
    -> (per step (iterations, halvings, status), positions after every step, whether the term was active in every step); once per case"""
    key = (name, coarse, steps)
    if key not in _runs:
        sc, ep, n = load_workload(name)
        orc = make_oracle(sc, ep, n)
        fixed = np.asarray(sc.fixed, dtype=bool)
        st = DR.DotStepper(orc, fixed, sc.cfg.dt, gravity(sc.cfg))
        dup = orc.dup()
        verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
        counts, xs, active = [], [], True
        for _ in range(steps):
            idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
            orc.move(idx, pos)
            M = None
            if coarse:
                M, act = DR.m_prime(orc, dup, verts, fixed)
                active = active and act
            r = st.step(M)
            counts.append((r["iters"], r["halvings"], r["status"]))
            xs.append(orc.state()[0])
        orc.close()
        _runs[key] = (counts, xs, active)
    return _runs[key]


def oracle_run(name, steps=STEPS):
    key = (name, "oracle", steps)
    if key not in _runs:
        sc, ep, n = load_workload(name)
        orc = make_oracle(sc, ep, n)
        counts, xs = [], []
        for _ in range(steps):
            idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
            orc.move(idx, pos)
            s = orc.step()
            counts.append((s.iters, s.ls_halvings, s.status))
            xs.append(orc.state()[0])
        orc.close()
        _runs[key] = (counts, xs)
    return _runs[key]


# ---- 1. without a coarse term the restatement is the oracle's step --------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR4, BAR12, BAR32, BUNNY])
def test_restatement_without_the_term_takes_the_oracles_iterations_and_halvings(name):
    """four scripted steps: the same iterations and halvings per step, positions within 1e-9 (the project's standing bound; the
    two differ in the summation order of their dot products only)"""
    want, xo = oracle_run(name)
    got, xr, _ = restated_run(name, False)
    err = max(np.abs(a - b).max() for a, b in zip(xr, xo))
    print(f"{name}: oracle {want}, restatement {got}, positions {err:.2e}")
    assert got == want and all(c[2] == 0 for c in got)
    assert err < 1e-9


# ---- 2. with the term -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR32, BAR12])
def test_coarse_term_cuts_the_iterations_of_four_steps_by_a_fifth(name):
    """iteration total over four steps with M' = M + Z A0^-1 Z^T at most 0.8 x the total with M"""
    c0, _, _ = restated_run(name, False)
    c1, _, active = restated_run(name, True)
    t0, t1 = sum(c[0] for c in c0), sum(c[0] for c in c1)
    print(f"{name}: iterations (halvings) per step {[(c[0], c[1]) for c in c0]} -> {[(c[0], c[1]) for c in c1]}: {t0} -> {t1}")
    assert active and all(c[2] == 0 for c in c1)
    assert t1 <= 0.8 * t0


# ---- 3. a dropped subdomain and the inactive fallback ----------------------------------------------------------------------------------------
def test_restated_step_converges_with_a_dropped_subdomain():
    """synbar:16x5x5:4 with every vertex of subdomain 0 fixed: zero columns, an identity block; two steps converge to the step's
    own criterion |g|^2 <= targetGRes, as the plain step does from the same state"""
    sc, ep, n = load_workload(BAR4)
    for coarse in (True, False):
        orc = make_oracle(sc, ep, n)
        verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
        fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
        fixed[verts[0]] = 1
        orc.set_fixed(fixed)
        fx = fixed.astype(bool)
        st = DR.DotStepper(orc, fx, sc.cfg.dt, gravity(sc.cfg))
        dup = orc.dup()
        for k in range(2):
            M = None
            if coarse:
                apply, live = DR.coarse_term(orc.state()[0], dup, verts, fx, orc.spmv)
                assert list(live) == [False, True, True, True] and apply is not None
                M = CR.precond(orc.apply_precond, apply)
            r = st.step(M)
            print(f"subdomain 0 fixed, coarse {coarse}, step {k}: {r['iters']} iterations, {r['halvings']} halvings, |g|^2 {r['g2']:.3e}")
            assert r["status"] == 0 and r["g2"] <= orc.target_gres and 0 < r["iters"] < 100
        assert np.array_equal(orc.state()[0][fx], np.asarray(sc.x0)[fx])       # fixed vertices have not moved
        orc.close()


def test_rank_deficient_z_falls_back_to_the_plain_step():
    """the collinear case of tests/test_coarse_host.py switches the term off (apply is None); the step with that preconditioner is
    the plain step: the oracle's iterations and halvings"""
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    Z, cen, live, w = CR.build_z(x, np.ones(3, dtype=int), [np.arange(3)], np.zeros(3, dtype=bool))
    A0 = CR.coarse_matrix(Z, live, lambda v: 2.0 * v)
    with np.errstate(all="ignore"):
        apply = CR.coarse_apply(Z, A0 - 1e-12 * np.eye(6))
    assert apply is None
    sc, ep, n = load_workload(BAR4)
    orc = make_oracle(sc, ep, n)
    st = DR.DotStepper(orc, np.asarray(sc.fixed, dtype=bool), sc.cfg.dt, gravity(sc.cfg))
    idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
    orc.move(idx, pos)
    M = CR.precond(orc.apply_precond, apply)
    assert M == orc.apply_precond
    r = st.step(M)
    orc.close()
    want, _ = oracle_run(BAR4)
    assert (r["iters"], r["halvings"], r["status"]) == want[0]


def test_direction_of_the_restatement_is_the_oracles_probe():
    """the two-loop and the step estimate against dor_probe_direction on an iterate and a history of three pairs from a running step"""
    sc, ep, n = load_workload(BAR12)
    orc = make_oracle(sc, ep, n)
    idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
    orc.move(idx, pos)
    orc.step_begin()
    for _ in range(3):
        assert orc.step_iterate() == 0
    x, g, S, Y, _ = orc.lbfgs_state()
    assert len(S) == 3
    want = orc.probe_direction(x, S, Y)
    q, z, p, a0 = DR.direction(g, [s.reshape(-1, 3) for s in S], [y.reshape(-1, 3) for y in Y], orc.apply_precond, orc.spmv)
    orc.close()
    for got, key in ((q, "q"), (z, "z"), (p, "p")):
        assert np.abs(got - want[key]).max() <= 1e-10 * np.abs(want[key]).max(), key
    assert abs(a0 - want["alpha0"]) <= 1e-10


# ---- 4. the entries ----------------------------------------------------------------------------------------------------------------------------
NEW = ("dotmi_set_dot_coarse", "dotmi_dot_coarse_info")


def test_new_entries_are_exported_declared_and_reject_a_null_handle():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    L = dl.load()
    for name in NEW:
        assert name in dl.EXPORTS and f"int {name}(" in header, name
        assert hasattr(L, name), name
    assert L.dotmi_set_dot_coarse(None, 1) == -1
    assert L.dotmi_set_dot_coarse(None, 0) == -1
    assert L.dotmi_dot_coarse_info(None, None, None, None, None, None) == -1


def test_step_stats_have_not_grown():
    """dotmi_step_stats has no size field, so it keeps its 328 bytes: the mode reports through dotmi_dot_coarse_info"""
    import ctypes as C
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    body = header[:header.index("} dotmi_step_stats;")]
    body = body[body.rindex("typedef struct"):]
    assert "coarse" not in body
    assert C.sizeof(dl.StepStats) == 328
