"""LBFGS-HI (DOTMI_FLAG_LBFGS_HI; `timeStepper LBFGSHI`, LBFGSTimeStepper with D0T_HI): L-BFGS whose initial inverse Hessian is a block
incomplete Cholesky factor of the projected Hessian in a multicolour ordering, rebuilt at the end of every step with a
diagonal-shift restart (dot_amd/csrc/k_ic.hip, dotmi_ic.hip).  The reference is the numpy restatement tests/ic_reference.py: fed
with the handle's own H it must give the device's factor and solve, and as the oracle's external solver it must give the device's
iterations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import ic_reference as R

pytestmark = pytest.mark.gpu

BAR, BUNNY = "synbar:16x5x5:1", "bunny5K_LTSS"
_plans = {}


def plan_of(name, sc):
    if name not in _plans:
        _plans[name] = R.plan_ic(sc.T, sc.V_rest.shape[0])
    return _plans[name]


def make_hi(sc, energy=None, flags=0, **kw):
    return DOTTimeStepper(sc, None, 1, energy=energy, alpha_min=1.0, flags=dl.FLAG_LBFGS_HI | flags, **kw)


def hval_blocks(ts, sc):
    """the handle's own assembled H, (nnzb, 3, 3) in CSR order, EXACTLY: H times sums of unit vectors over vertex sets in which no
    two vertices share a neighbour -- every entry of the product is then one entry of H plus exact zeros"""
    nV = sc.V_rest.shape[0]
    ptr, idx = R.adjacency(sc.T, nV)
    rows = np.repeat(np.arange(nV), np.diff(ptr))
    nb = [idx[ptr[v]:ptr[v + 1]] for v in range(nV)]
    group = np.full(nV, -1)
    for v in range(nV):
        two = np.unique(np.concatenate([nb[u] for u in nb[v]]))
        used = set(group[two].tolist())
        g = 0
        while g in used:
            g += 1
        group[v] = g
    blocks = np.zeros((len(idx), 3, 3))
    for g in range(group.max() + 1):
        k = np.nonzero(group[idx] == g)[0]            # the CSR entries whose column is in the set
        for d in range(3):
            p = np.zeros((nV, 3))
            p[group == g, d] = 1.0
            blocks[k, :, d] = ts.multiply(p)[rows[k]]
    return blocks


def block_errors(got, ref):
    """per 3 x 3 block: max |difference| relative to the block's largest entry (a zero block -- the couplings of a fixed vertex --
    must be zero exactly)"""
    scale = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    err = np.abs(got - ref).reshape(len(ref), -1).max(axis=1)
    return np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), np.where(err == 0.0, 0.0, np.inf))


def scripted_step(sc, ts, orc):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    orc.move(idx, pos)
    return ts.step(), orc.step()


def expected_shift(prev, attempts):
    """the shift a factorisation ends on: half the last successful one first, doubled (from 1e-3) per further attempt"""
    sigma = 0.0 if prev == 0.0 else 0.5 * prev
    for _ in range(attempts - 1):
        sigma = max(1e-3, 2.0 * sigma)
    return sigma


# ---- 1. the factor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy", [dl.ENERGY_FCR, dl.ENERGY_SNH])
def test_factor_is_the_restatement_on_the_handles_own_hessian(energy):
    """dotmi_ic_factor against the restatement fed with the handle's H (create-time refresh, and the refresh at the end of a step):
    1e-12 relative per block, the same colours, shift and attempts"""
    sc, _, _ = load_workload(BAR)
    P = plan_of(BAR, sc)
    ts = make_hi(sc, energy=energy)
    ref = R.ICReference(P)
    for k in range(2):
        if k:
            idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
            ts.setDirichlet(idx, pos)
            assert ts.step().status == 0
        assert ref.factor(hval_blocks(ts, sc))
        F = ts.icFactor()
        assert F.shape == ref.F.shape == (P["nL"] + P["nV"], 3, 3)
        err = block_errors(F, ref.F)
        print(f"energy {energy} refresh {k}: max relative block error {err.max():.3e}")
        assert err.max() <= 1e-12
        assert ts.icInfo() == (P["nColours"], ref.shift, ref.attempts) == (8, 0.0, 1)
    ts.close()


# ---- 2. the application ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BAR, BUNNY])
def test_apply_is_the_restatements_solve(name):
    """applyPrecond(r) against the restatement's solve with the factor of the handle's own H at the shift the device reports,
    1e-10 relative"""
    sc, _, _ = load_workload(name)
    P = plan_of(name, sc)
    ts = make_hi(sc)
    colours, shift, attempts = ts.icInfo()
    assert colours == P["nColours"] and attempts >= 1
    ref = R.ICReference(P)
    F, ok = ref.factor_attempt(hval_blocks(ts, sc), shift)
    assert ok
    print(f"{name}: shift {shift}, {attempts} attempts, max relative block error {block_errors(ts.icFactor(), F).max():.3e}")
    r = np.random.default_rng(0).standard_normal((P["nV"], 3))
    z = ts.applyPrecond(r)
    want = ref.solve(r, F)
    err = np.abs(z - want).max() / np.abs(want).max()
    print(f"{name}: apply relative error {err:.3e}")
    assert err <= 1e-10
    assert ts.step().precond_bytes == 72 * (P["nL"] + P["nV"]) * 2      # every stored block, forward and backward
    ts.close()


# ---- 3. steps against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("energy", [dl.ENERGY_FCR, dl.ENERGY_SNH])
def test_steps_match_the_oracle_with_the_restatement(energy):
    sc, _, _ = load_workload(BAR)
    ts = make_hi(sc, energy=energy)
    sol = R.ICSolver(R.ICReference(plan_of(BAR, sc)))
    orc = R.oracle_whole_mesh(sc, energy)
    sol.bind(orc)
    iters = []
    for k in range(4):
        st, so = scripted_step(sc, ts, orc)
        iters.append(st.iters)
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
        assert st.ms_factor > 0.0 and st.ms_hessian > 0.0, k     # HI refreshes at the end of every step, unlike PD
        assert ts.icInfo()[1:] == sol.log[-1] == (0.0, 1), k
    assert iters == [9, 12, 14, 14]
    ts.close()
    orc.close()


# ---- 4. the shift path -------------------------------------------------------------------------------------------------------------
def test_shift_restart_on_bunny_matches_the_restatement():
    """bunny5K / FCR needs the shift at every factorisation: create and two steps.  The device reports the restatement's shift
    exactly and its attempt count; after the first factorisation the attempts follow the half-then-double rule; the steps match
    the oracle."""
    sc, _, _ = load_workload(BUNNY)
    ts = make_hi(sc, energy=dl.ENERGY_FCR)
    sol = R.ICSolver(R.ICReference(plan_of(BUNNY, sc)))
    orc = R.oracle_whole_mesh(sc, dl.ENERGY_FCR)
    sol.bind(orc)
    colours, shift, attempts = ts.icInfo()
    assert colours == 12 and shift > 0.0
    assert (shift, attempts) == sol.log[-1] and shift == expected_shift(0.0, attempts)
    for k in range(2):
        prev = shift
        st, so = scripted_step(sc, ts, orc)
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
        assert st.ms_factor > 0.0, k
        _, shift, attempts = ts.icInfo()
        print(f"step {k}: {st.iters} iterations, shift {shift}, {attempts} attempts, ms_factor {st.ms_factor:.3f}")
        assert (shift, attempts) == sol.log[-1], k
        assert shift > 0.0 and shift == expected_shift(prev, attempts), k
    assert len(sol.log) == 3
    ts.close()
    orc.close()


# ---- 5. refix ----------------------------------------------------------------------------------------------------------------------
def test_refix_refactors_on_the_new_fixed_set():
    sc, _, _ = load_workload(BAR)
    P = plan_of(BAR, sc)
    ts = make_hi(sc)
    sol = R.ICSolver(R.ICReference(P))
    orc = R.oracle_whole_mesh(sc, sc.cfg.energy_id)
    sol.bind(orc)
    st, so = scripted_step(sc, ts, orc)          # one step on the first fixed set
    assert (st.iters, st.ls_halvings) == (so.iters, so.ls_halvings)
    before = ts.icFactor()
    fixed = np.array(sc.fixed, dtype=np.uint8).copy()
    xs = np.unique(sc.V_rest[:, 0])
    fixed[sc.V_rest[:, 0] == xs[len(xs) // 2]] = 1   # pin the middle cross-section as well (the script holds both ends)
    assert (fixed != np.asarray(sc.fixed, dtype=np.uint8)).any()
    ts.refix(fixed)
    orc.set_fixed(fixed)                          # (its refresh factors through the callback again)
    own = R.ICReference(P)
    assert own.factor(hval_blocks(ts, sc))
    F = ts.icFactor()
    assert block_errors(F, own.F).max() <= 1e-12 and np.abs(F - before).max() > 1e-3
    assert ts.icInfo() == (8, own.shift, own.attempts)
    for k in range(2):
        st, so = scripted_step(sc, ts, orc)
        assert (st.status, st.iters, st.ls_halvings) == (so.status, so.iters, so.ls_halvings), k
        assert st.status == 0 and st.ms_factor > 0.0
        assert np.abs(ts.getResult() - orc.state()[0]).max() < 1e-9, k
    ts.close()
    orc.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [dl.FLAG_GSDD, dl.FLAG_NEWTON, dl.FLAG_FORCE_DIST, dl.FLAG_ASYNC_REFRESH, dl.FLAG_OWNER_EXCHANGE,
                                   dl.FLAG_LBFGS_PD])
def test_rejected_combinations(extra):
    sc, _, _ = load_workload(BAR)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_LBFGS_HI"):
        make_hi(sc, flags=extra)


def test_rejects_a_vertex_partition_and_more_than_one_rank():
    sc, _, _ = load_workload(BAR)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_LBFGS_HI"):
        make_hi(sc, vpart=np.zeros(sc.V_rest.shape[0], dtype=np.int32))
    with pytest.raises(DotmiError, match="DOTMI_FLAG_LBFGS_HI"):
        make_hi(sc, world=2, rank=0, comm_id=bytes(128))


def test_block_solve_entries_are_refused():
    sc, _, _ = load_workload(BAR)
    ts = make_hi(sc)
    L = dl.load()
    n = 3 * sc.V_rest.shape[0]
    buf = np.zeros(n)
    pp = buf.ctypes.data_as(C.POINTER(C.c_double))
    ms, nb = C.c_double(), C.c_int64()
    msp = C.cast(C.byref(ms), dl.c_dp)

    def refused(rc):
        return rc == -1 and b"LBFGS-HI" in L.dotmi_last_error(ts._h)     # DOTMI_E_INVALID with a message

    assert refused(L.dotmi_part_matrix(ts._h, 0, 0, pp, None))
    assert refused(L.dotmi_probe_direction(ts._h, pp, 0, None, None, None, None, None, None, None, None))
    assert refused(L.dotmi_bench_precond(ts._h, 1, msp, C.byref(nb)))
    for kind in ("backsolve", "merge", "build_qpad", "spmv_zp", "merge_early", "elem_step", "gather_early", "dirstep", "elem_vertex"):
        assert refused(L.dotmi_bench_kernel(ts._h, dl.BENCH_KERNELS.index(kind), 1, msp, C.byref(nb))), kind
    assert L.dotmi_part_size(ts._h, 0) == -1
    # what does not need the block solve keeps working: H exists (dotmi_spmv), dotmi_refactor refreshes H and its factor
    assert L.dotmi_bench_kernel(ts._h, dl.BENCH_KERNELS.index("spmv_dots"), 1, msp, C.byref(nb)) == 0
    e0 = np.zeros((sc.V_rest.shape[0], 3))
    e0[1, 0] = 1.0
    assert np.abs(ts.multiply(e0)).max() > 0.0
    before = ts.icFactor()
    ts.updatePrecondMtrAndFactorize()
    assert np.array_equal(ts.icFactor(), before)      # the same positions: bit-identical, run to run
    ts.close()


# ---- 7. the runner -----------------------------------------------------------------------------------------------------------------
def test_headless_runner_takes_lbfgs_hi(tmp_path):
    """`timeStepper LBFGSHI` in a reference-format script: dot_hip runs LBFGS-HI on the whole mesh -- dotmi_ic_info's colour count on
    its report line, per frame the iterations and energy of the Python-driven HI stepper --, and writes the run's files but no
    partition files"""
    from tests.test_host_logic import _write_msh
    from tests.workloads import MESH_DIR
    from dot_amd import scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(root, "dot_amd", "host")])
    V, T = scene.load_mesh_npz(os.path.join(MESH_DIR, "bunny5K.npz"))
    _write_msh(tmp_path / "bunny5K.msh", V, T)
    (tmp_path / "bunny.txt").write_text("energy FCR\ntimeStepper LBFGSHI\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\n"
                                        "stiffness 100000 0.4\nscript twistnsns\nshape input bunny5K.msh\n")
    out = subprocess.check_output([exe, "100", str(tmp_path / "bunny.txt"), "--mesh-root", str(tmp_path), "--frames", "3",
                                   "--out", str(tmp_path / "out")], timeout=600).decode()
    info = [l.split() for l in out.splitlines() if l.startswith("LBFGS-HI:")]
    assert len(info) == 1 and int(info[0][1]) == 12 and float(info[0][4].rstrip(",")) > 0.0
    frames = [l.split() for l in out.splitlines() if l.startswith("FRAME")]
    assert len(frames) == 3
    sc, _, _ = load_workload(BUNNY)
    ts = make_hi(sc)
    assert ts.icInfo()[0] == 12
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
