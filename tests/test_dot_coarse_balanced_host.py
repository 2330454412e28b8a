"""The balanced form of DOT's coarse term (dotmi_set_dot_coarse_mode, mode 2), host only: the plan of W = H Z (dotmi_plan_coarse_hz), W from
the plan's lists against H Z, and the numpy restatement (tests/dot_coarse_balanced_reference.py) on the oracle's operators --
exactness on the coarse space, the iteration counts against mode 1, a dropped subdomain, the inactive fallback -- and the new
entries' presence and argument checks (no device is touched)."""
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import dot_coarse_balanced_reference as BR
from tests import dot_coarse_reference as DR
from tests.test_dot_coarse_host import gravity, make_oracle, oracle_run, restated_run
from tests.test_pcg_host import oracle_state

BAR4, BAR12, BAR32, BUNNY = "synbar:16x5x5:4", "synbar:48x4x4:12", "synbar:96x4x4:32", "bunny5K_LTSS"
SHAPES = [BAR4, BAR12, BAR32, BUNNY]
STEPS = 4
_runs, _parts = {}, {}


def balanced_run(name, steps=STEPS):
    """`steps` scripted steps of the restatement with M'' on an oracle of its own -> (per step (iterations, halvings, status),
    positions after every step, whether the term was active in every step); once per case"""
    key = (name, steps)
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
            M, act = BR.m_second(orc, dup, verts, fixed)
            active = active and act
            r = st.step(M)
            counts.append((r["iters"], r["halvings"], r["status"]))
            xs.append(orc.state()[0])
        orc.close()
        _runs[key] = (counts, xs, active)
    return _runs[key]


def coarse_parts(name):
    """Z, A0, W, the centroids and weights at the positions of tests/test_pcg_host.oracle_state, once per mesh"""
    if name not in _parts:
        sc, orc, dup, free, _, n = oracle_state(name)
        x = orc.state()[0]
        verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
        Z, cen, live, w = CR.build_z(x, dup, verts, ~free)
        W = BR.hz(Z, live, orc.spmv)
        _parts[name] = dict(x=x, Z=Z, cen=cen, live=live, w=w, W=W, A0=CR.coarse_matrix(Z, live, orc.spmv))
    return _parts[name]


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_plan_lists_every_coupled_vertex_subdomain_pair_once_in_ascending_order(name):
    sc, ep, n = load_workload(name)
    nV = sc.V_rest.shape[0]
    P = BR.plan_hz(sc.T, ep, n, nV)
    C = CR.plan(sc.T, ep, n, nV)
    adj_ptr, adj_idx, blk_row = CR.block_csr(sc.T, nV)
    subs = [C["vsIdx"][C["vsPtr"][v]:C["vsPtr"][v + 1]] for v in range(nV)]
    # every (i, t, block (i, j) with j in t), as a sorted list: the entries and their block lists must be exactly this
    want = sorted((int(blk_row[k]), int(t), k) for k in range(adj_idx.size) for t in subs[adj_idx[k]])
    nE, nB = P["sizes"]
    assert nB == len(want) and P["hzPtr"][0] == 0 and P["hzPtr"][-1] == nE and P["hzBlkPtr"][0] == 0 and P["hzBlkPtr"][-1] == nB
    got = []
    for i in range(nV):
        e0, e1 = P["hzPtr"][i], P["hzPtr"][i + 1]
        assert (np.diff(P["hzSub"][e0:e1]) > 0).all(), i                         # the subdomains of a vertex ascend: each (i, t) once
        assert (P["hzVert"][e0:e1] == i).all()
        for e in range(e0, e1):
            blk = P["hzBlk"][P["hzBlkPtr"][e]:P["hzBlkPtr"][e + 1]]
            assert blk.size > 0 and (np.diff(blk) > 0).all(), e                    # the blocks of an entry ascend
            got += [(i, int(P["hzSub"][e]), int(k)) for k in blk]
    assert got == want
    entries = sorted(set((i, t) for i, t, _ in want))
    assert nE == len(entries) and entries == list(zip(P["hzVert"].tolist(), P["hzSub"].tolist()))
    # the transposed index: a permutation of the entries, per subdomain in ascending vertex
    assert sorted(P["hzTEnt"].tolist()) == list(range(nE))
    assert P["hzTPtr"][0] == 0 and P["hzTPtr"][-1] == nE
    for t in range(n):
        ent = P["hzTEnt"][P["hzTPtr"][t]:P["hzTPtr"][t + 1]]
        assert (P["hzSub"][ent] == t).all() and (np.diff(P["hzVert"][ent]) > 0).all(), t
    print(f"{name}: {nE} (vertex, subdomain) blocks for {nV} vertices (sum dup = {C['sizes'][2]}), {nB} H blocks")


def test_plan_rejects_bad_arguments():
    sc, ep, n = load_workload(BAR4)
    nV, nT = sc.V_rest.shape[0], sc.T.shape[0]
    L = dl.load()
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    ep = np.ascontiguousarray(ep, dtype=np.int32)
    sizes = np.zeros(2, dtype=np.int32)
    none = [None] * 7
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(ep), n, dl.ip(sizes), *none) == 0
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(ep), 257, dl.ip(sizes), *none) == -1      # more than 256 subdomains
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(ep), n - 1, dl.ip(sizes), *none) == -1    # epart out of range
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), None, n, dl.ip(sizes), *none) == -1
    assert L.dotmi_plan_coarse_hz(nV, nT, None, dl.ip(ep), n, dl.ip(sizes), *none) == -1
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(ep), n, None, *none) == -1
    assert L.dotmi_plan_coarse_hz(0, nT, dl.ip(T), dl.ip(ep), n, dl.ip(sizes), *none) == -1


# ---- 2. W from the lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR4, BUNNY])
def test_w_from_the_plans_lists_is_h_z(name):
    """the sums coarse_hz_kernel forms, in numpy on the oracle's H blocks, against spmv(Z[:, c]) column by column: 1e-12 of the largest
    entry of W, the bound tests/test_coarse_host.py uses for A0 from its lists"""
    sc, orc, dup, free, _, n = oracle_state(name)
    S = coarse_parts(name)
    nV = sc.V_rest.shape[0]
    _, ep, _ = load_workload(name)
    P = BR.plan_hz(sc.T, ep, n, nV)
    adj_ptr, adj_idx, blk_row = CR.block_csr(sc.T, nV)
    Hb = CR.h_blocks(orc.spmv, adj_ptr, adj_idx, blk_row, nV)
    got = BR.w_from_lists(P, Hb, adj_idx, S["x"], S["w"], S["cen"], S["live"])
    err = np.abs(got - S["W"]).max() / np.abs(S["W"]).max()
    print(f"{name}: {P['sizes'][0]} blocks, lists against H Z {err:.2e}; rows of fixed vertices {np.abs(got.reshape(nV, 3, -1)[~free]).max():.1e}")
    assert S["live"].all() and err <= 1e-12
    assert not got.reshape(nV, 3, -1)[~free].any()                                # identity rows of H on vertices of weight zero
    # outside the listed entries H Z is structurally zero
    mask = np.zeros((nV, n), dtype=bool)
    mask[P["hzVert"], P["hzSub"]] = True
    assert not S["W"].reshape(nV, 3, n, 6).transpose(0, 2, 1, 3)[~mask].any()


# ---- 3. exactness on the coarse space ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_balanced_preconditioner_solves_the_coarse_space_exactly(name):
    """M''(H Z y) = Z y for four random y, relative to max|Z y|: 1e-10 (2e-14 measured where rcond(A0) >= 6e-5; the margin is eps / rcond)"""
    sc, orc, dup, free, _, n = oracle_state(name)
    S = coarse_parts(name)
    M = BR.balanced(orc.apply_precond, S["Z"], S["A0"], S["W"])
    assert M != orc.apply_precond
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(4):
        y = rng.standard_normal(6 * n)
        zy = (S["Z"] @ y).reshape(-1, 3)
        got = M(orc.spmv(zy))
        worst = max(worst, np.abs(got - zy).max() / np.abs(zy).max())
    print(f"{name}: M'' H Z y against Z y {worst:.2e}, rcond(A0) {1.0 / np.linalg.cond(S['A0']):.1e}")
    assert worst <= 1e-10


# ---- 4. the iterations --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR32, BAR12])
def test_balanced_form_takes_at_most_seven_tenths_of_mode_ones_iterations(name):
    """four scripted steps, every one with status 0: the total with M'' at most 0.7 x the total with M' = M + C (21 / 40 and 17 / 32 when
    the mode was proposed)"""
    c1, _, a1 = restated_run(name, True)
    c2, _, a2 = balanced_run(name)
    t1, t2 = sum(c[0] for c in c1), sum(c[0] for c in c2)
    print(f"{name}: iterations (halvings) per step, mode 1 {[(c[0], c[1]) for c in c1]} -> mode 2 {[(c[0], c[1]) for c in c2]}: {t1} -> {t2}")
    assert a1 and a2 and all(c[2] == 0 for c in c1 + c2)
    assert t2 <= 0.7 * t1


# ---- 5. a dropped subdomain and the inactive fallback -----------------------------------------------------------------------------------
def test_restated_step_converges_with_a_dropped_subdomain():
    """synbar:16x5x5:4 with every vertex of subdomain 0 fixed: zero columns of Z and W, an identity block; two steps converge to the
    step's own criterion"""
    sc, ep, n = load_workload(BAR4)
    orc = make_oracle(sc, ep, n)
    verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
    fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
    fixed[verts[0]] = 1
    orc.set_fixed(fixed)
    fx = fixed.astype(bool)
    st = DR.DotStepper(orc, fx, sc.cfg.dt, gravity(sc.cfg))
    dup = orc.dup()
    for k in range(2):
        Z, A0, W, live = BR.parts(orc.state()[0], dup, verts, fx, orc.spmv)
        assert list(live) == [False, True, True, True] and not W[:, :6].any()
        M = BR.balanced(orc.apply_precond, Z, A0, W)
        assert M != orc.apply_precond
        r = st.step(M)
        print(f"subdomain 0 fixed, step {k}: {r['iters']} iterations, {r['halvings']} halvings, |g|^2 {r['g2']:.3e}")
        assert r["status"] == 0 and r["g2"] <= orc.target_gres and 0 < r["iters"] < 100
    assert np.array_equal(orc.state()[0][fx], np.asarray(sc.x0)[fx])
    orc.close()


def test_indefinite_a0_returns_the_plain_preconditioner():
    """an A0 made indefinite switches the term off: the callable is plain M itself, and a step with it is the oracle's"""
    sc, ep, n = load_workload(BAR4)
    orc = make_oracle(sc, ep, n)
    fixed = np.asarray(sc.fixed, dtype=bool)
    st = DR.DotStepper(orc, fixed, sc.cfg.dt, gravity(sc.cfg))
    idx, pos = sc.scripter.step(orc.state()[0], sc.cfg.dt)
    orc.move(idx, pos)
    verts = [np.asarray(orc.part_verts(p)) for p in range(n)]
    Z, A0, W, live = BR.parts(orc.state()[0], orc.dup(), verts, fixed, orc.spmv)
    assert BR.balanced(orc.apply_precond, Z, A0, W) != orc.apply_precond
    bad = A0 - 2.0 * np.linalg.eigvalsh(A0).max() * np.eye(A0.shape[0])
    M = BR.balanced(orc.apply_precond, Z, bad, W)
    assert M == orc.apply_precond
    r = st.step(M)
    orc.close()
    want, _ = oracle_run(BAR4)
    assert (r["iters"], r["halvings"], r["status"]) == want[0]


# ---- 6. the entries ------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_exported_declared_and_check_their_arguments():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    L = dl.load()
    for name, ret in (("dotmi_set_dot_coarse_mode", "int"), ("dotmi_dot_coarse_mode", "int32_t"), ("dotmi_plan_coarse_hz", "int")):
        assert name in dl.EXPORTS and f"{ret} {name}(" in header, name
        assert hasattr(L, name), name
    assert L.dotmi_dot_coarse_mode(None) == 0
    for mode in (0, 1, 2):
        assert L.dotmi_set_dot_coarse_mode(None, mode) == -1
    comment = header[:header.index("int dotmi_set_dot_coarse_mode(")]
    comment = comment[comment.rindex("/*"):]
    assert "mode 2" in comment and "the reference has no counterpart" in comment
