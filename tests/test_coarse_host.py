"""The rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse), host only: the plan of the assembly
(dotmi_plan_coarse), the coarse matrix from the plan's lists against Z^T H Z, and the numpy restatement (tests/coarse_reference.py) on
the oracle's operators -- symmetry, iteration counts with and without the coarse term, the true residual, a dropped subdomain, the
inactive fallback -- and the new ABI entries' presence and argument checks (no device is touched)."""
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import pcg_reference as R
from tests.test_pcg_host import oracle_state, random_free

BAR4, BUNNY, BAR32 = "synbar:16x5x5:4", "bunny5K_LTSS", "synbar:96x4x4:32"
_coarse = {}


def coarse_state(name):
    """oracle_state plus the restatement's Z, A0 and apply at the oracle's positions, built once per mesh"""
    if name not in _coarse:
        sc, orc, dup, free, b, n = oracle_state(name)
        x = orc.state()[0]
        verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
        Z, cen, live, w = CR.build_z(x, dup, verts, ~free)
        A0 = CR.coarse_matrix(Z, live, orc.spmv)
        _coarse[name] = dict(x=x, verts=verts, Z=Z, cen=cen, live=live, w=w, A0=A0, apply=CR.coarse_apply(Z, A0))
    return _coarse[name]


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,maxdup", [(BAR4, 2), (BUNNY, 5)])
def test_plan_lists_every_block_once_per_pair_of_subdomains_in_ascending_order(name, maxdup):
    sc, ep, n = load_workload(name)
    nV = sc.V_rest.shape[0]
    P = CR.plan(sc.T, ep, n, nV)
    adj_ptr, adj_idx, blk_row = CR.block_csr(sc.T, nV)
    dup = R.dup_of(sc.T, ep, nV)
    assert dup.max() == maxdup
    # the vertex lists: the subdomains of a vertex / the vertices of a subdomain, both ascending
    inc = np.unique(np.stack([np.asarray(sc.T).ravel(), np.repeat(ep, 4)], axis=1), axis=0)     # (vertex, subdomain), sorted
    assert np.array_equal(np.diff(P["vsPtr"]), dup) and np.array_equal(P["vsIdx"], inc[:, 1])
    by_part = inc[np.lexsort((inc[:, 0], inc[:, 1]))]
    assert np.array_equal(P["svIdx"], by_part[:, 0]) and np.array_equal(np.diff(P["svPtr"]), np.bincount(inc[:, 1], minlength=n))
    # the pairs: s <= t, ordered, each once, every diagonal present
    pairs = np.stack([P["pairS"], P["pairT"]], axis=1)
    assert (pairs[:, 0] <= pairs[:, 1]).all()
    key = pairs[:, 0].astype(np.int64) * n + pairs[:, 1]
    assert (np.diff(key) > 0).all() and set(range(n)) <= set(pairs[pairs[:, 0] == pairs[:, 1], 0].tolist())
    # the entries: every (H block, s containing i, t containing j, s <= t) exactly once, ascending per pair
    subs = [P["vsIdx"][P["vsPtr"][v]:P["vsPtr"][v + 1]] for v in range(nV)]
    want = []
    for k in range(adj_idx.size):
        for s in subs[blk_row[k]]:
            for t in subs[adj_idx[k]]:
                if s <= t:
                    want.append((int(s) * n + int(t), k))
    got = []
    for p in range(pairs.shape[0]):
        blk = P["pairBlk"][P["pairPtr"][p]:P["pairPtr"][p + 1]]
        assert (np.diff(blk) > 0).all(), p
        got += [(int(key[p]), int(k)) for k in blk]
    assert len(got) == len(set(got)) == P["sizes"][1]
    assert sorted(got) == sorted(want)


def test_plan_rejects_bad_arguments():
    sc, ep, n = load_workload(BAR4)
    nV, nT = sc.V_rest.shape[0], sc.T.shape[0]
    L = dl.load()
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    ep = np.ascontiguousarray(ep, dtype=np.int32)
    sizes = np.zeros(3, dtype=np.int32)
    none = [None] * 8
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(ep), n, dl.ip(sizes), *none) == 0
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(ep), 257, dl.ip(sizes), *none) == -1      # more than 256 subdomains
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(ep), n - 1, dl.ip(sizes), *none) == -1    # epart out of range
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), None, n, dl.ip(sizes), *none) == -1
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(ep), n, None, *none) == -1


# ---- 2. A0 from the lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR4, BUNNY])
def test_coarse_matrix_from_the_plans_lists_is_zt_h_z(name):
    """the sums the assembly kernel forms, in numpy on the oracle's H blocks, against Z^T H Z column by column through the oracle's
    spmv: 1e-12 of the largest entry, the project's bound for assembled matrices"""
    sc, orc, dup, free, _, n = oracle_state(name)
    S = coarse_state(name)
    nV = sc.V_rest.shape[0]
    _, ep, _ = load_workload(name)
    P = CR.plan(sc.T, ep, n, nV)
    adj_ptr, adj_idx, blk_row = CR.block_csr(sc.T, nV)
    Hb = CR.h_blocks(orc.spmv, adj_ptr, adj_idx, blk_row, nV)
    # (the probed blocks are H: one product against the operator)
    v = random_free(free, 5)
    Hv = np.zeros_like(v)
    np.add.at(Hv, blk_row, np.einsum("kab,kb->ka", Hb, v[adj_idx]))
    assert np.abs(Hv - orc.spmv(v)).max() <= 1e-12 * np.abs(Hv).max()
    got = CR.a0_from_lists(P, Hb, adj_idx, blk_row, S["x"], S["w"], S["cen"], S["live"])
    err = np.abs(got - S["A0"]).max() / np.abs(S["A0"]).max()
    print(f"{name}: nc {got.shape[0]}, cond(A0) {np.linalg.cond(S['A0']):.1e}, lists against Z^T H Z {err:.2e}")
    assert S["live"].all() and err <= 1e-12


# ---- 3. the preconditioner ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR4, BUNNY, BAR32])
def test_preconditioner_with_the_coarse_term_is_symmetric(name):
    sc, orc, dup, free, _, _ = oracle_state(name)
    S = coarse_state(name)
    M = CR.precond(R.m_sym(orc.apply_precond, dup), S["apply"])
    a, b = random_free(free, 1), random_free(free, 2)
    ab, ba = np.vdot(a, M(b)), np.vdot(b, M(a))
    asym = np.abs(S["A0"] - S["A0"].T).max() / np.abs(S["A0"]).max()
    print(f"{name}: M asymmetry {abs(ab - ba) / abs(ab):.2e}, A0 asymmetry {asym:.2e}")
    assert S["apply"] is not None and abs(ab - ba) <= 1e-12 * abs(ab) and asym <= 1e-12


def test_coarse_term_cuts_the_iterations_on_32_subdomains_and_keeps_the_true_residual():
    """synbar:96x4x4:32: at 1e-3 and at 1e-8 at most 0.7 x the iterations of M_sym alone; true residual <= 2e-8 at 1e-8"""
    sc, orc, dup, free, b, n = oracle_state(BAR32)
    assert n == 32
    S = coarse_state(BAR32)
    Ms = R.m_sym(orc.apply_precond, dup)
    M = CR.precond(Ms, S["apply"])
    for tol in (1e-3, 1e-8):
        _, it0, _, st0 = R.pcg(orc.spmv, Ms, b, tol, 500)
        u, it1, res, st1 = R.pcg(orc.spmv, M, b, tol, 500)
        true = np.linalg.norm(b - orc.spmv(u)) / np.linalg.norm(b)
        print(f"{BAR32} at {tol:g}: {it0} -> {it1} iterations, recursive {res[-1]:.3e}, true {true:.3e}")
        assert st0 == 1 and st1 == 1 and it1 <= 0.7 * it0
        if tol == 1e-8:
            assert res[-1] <= 1e-8 and true <= 2e-8


@pytest.mark.parametrize("name", [BAR4, BUNNY])
def test_restatement_with_the_coarse_term_reaches_the_tolerance_with_the_true_residual(name):
    sc, orc, dup, free, b, _ = oracle_state(name)
    S = coarse_state(name)
    M = CR.precond(R.m_sym(orc.apply_precond, dup), S["apply"])
    u, it, res, state = R.pcg(orc.spmv, M, b, 1e-8, 500)
    true = np.linalg.norm(b - orc.spmv(u)) / np.linalg.norm(b)
    print(f"{name}: {it} iterations, recursive {res[-1]:.3e}, true {true:.3e}")
    assert state == 1 and 0 < it < 200 and res[-1] <= 1e-8 and true <= 2e-8
    assert np.abs(u[~free]).max() == 0.0


# ---- 4. a dropped subdomain and the inactive fallback ------------------------------------------------------------------------------------
def test_subdomain_without_free_vertices_is_dropped_and_the_solve_converges():
    """synbar:16x5x5:4 with every vertex of subdomain 0 fixed: zero columns, an identity block, A0 SPD, convergence at 1e-8"""
    sc, orc, dup, free, _, n = oracle_state(BAR4)
    x = orc.state()[0]
    verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
    fixed0 = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed = fixed0.copy()
    fixed[verts[0]] = 1
    try:
        orc.set_fixed(fixed)
        orc.refactor(x)
        b = -orc.gradient(x)
        b[fixed.astype(bool)] = 0.0
        Z, cen, live, w = CR.build_z(x, dup, verts, fixed)
        assert list(live) == [False, True, True, True] and not Z[:, :6].any() and not cen[0].any()
        A0 = CR.coarse_matrix(Z, live, orc.spmv)
        assert np.array_equal(A0[:6, :6], np.eye(6)) and not A0[:6, 6:].any() and not A0[6:, :6].any()
        assert np.linalg.eigvalsh(0.5 * (A0 + A0.T)).min() > 0.0
        apply = CR.coarse_apply(Z, A0)
        assert apply is not None
        M = CR.precond(R.m_sym(orc.apply_precond, dup), apply)
        u, it, res, state = R.pcg(orc.spmv, M, b, 1e-8, 500)
        true = np.linalg.norm(b - orc.spmv(u)) / np.linalg.norm(b)
        print(f"subdomain 0 fixed: {it} iterations, true residual {true:.3e}")
        assert state == 1 and true <= 2e-8
    finally:
        orc.set_fixed(fixed0)
        orc.refactor(x)


def test_rank_deficient_z_switches_the_term_off():
    """three collinear free vertices leave the rotation about their line without stiffness: A0 is singular, the restatement's
    apply is None and the preconditioner is M_sym itself -- the fallback the device takes on a non-positive pivot"""
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    Z, cen, live, w = CR.build_z(x, np.ones(3, dtype=int), [np.arange(3)], np.zeros(3, dtype=bool))
    assert live[0] and np.linalg.matrix_rank(Z) == 5
    A0 = CR.coarse_matrix(Z, live, lambda v: 2.0 * v)
    with np.errstate(all="ignore"):
        apply = CR.coarse_apply(Z, A0 - 1e-12 * np.eye(6))     # (rounding may leave the zero pivot on either side)
    assert apply is None
    ms = lambda r: 0.5 * r                                    # noqa: E731
    assert CR.precond(ms, apply) is ms


def test_weights_and_columns_are_the_specified_ones():
    x = np.random.default_rng(3).standard_normal((6, 3))
    dup = np.array([1, 2, 2, 1, 1, 3])
    fixed = np.array([0, 0, 0, 0, 1, 0], dtype=bool)
    verts = [np.array([0, 1, 2, 5]), np.array([1, 2, 3, 4, 5])]
    Z, cen, live, w = CR.build_z(x, dup, verts, fixed)
    assert np.allclose(w, [1, 0.5, 0.5, 1, 0, 1 / 3]) and live.all()
    for s, vs in enumerate(verts):
        c = (w[vs, None] * x[vs]).sum(0) / w[vs].sum()
        assert np.allclose(cen[s], c)
        for v in range(6):
            blk = Z[3 * v:3 * v + 3, 6 * s:6 * s + 6]
            if v not in vs:
                assert not blk.any()
                continue
            for a in range(3):
                e = np.eye(3)[a]
                assert np.allclose(blk[:, a], w[v] * e) and np.allclose(blk[:, 3 + a], w[v] * np.cross(e, x[v] - c))


# ---- 5. the entries ----------------------------------------------------------------------------------------------------------------------
NEW = ("dotmi_set_pcg_coarse", "dotmi_pcg_coarse_info", "dotmi_pcg_coarse_matrix", "dotmi_pcg_apply_precond", "dotmi_plan_coarse")


def test_new_entries_are_exported_declared_and_reject_a_null_handle():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    L = dl.load()
    for name in NEW:
        assert name in dl.EXPORTS and f"int {name}(" in header, name
        assert hasattr(L, name), name
    buf = np.zeros(3)
    assert L.dotmi_set_pcg_coarse(None, 1) == -1
    assert L.dotmi_pcg_coarse_info(None, None, None, None, None) == -1
    assert L.dotmi_pcg_coarse_matrix(None, 0, None) == -1
    assert L.dotmi_pcg_apply_precond(None, dl.dp(buf), dl.dp(buf)) == -1
