"""DOTMI_FLAG_NEWTON_PCG_DIST and dotmi_solve_hessian on SHARDED handles (pcg_iteration / pcg_agree in dot_amd/csrc/dotmi_pcg.hip,
pcg_spmv_rows_kernel and pcg_update_kernel<true> in k_pcg.hip; DESIGN.md sections 6 and 9).

1. one rank under DOTMI_FLAG_FORCE_DIST, the three sharding modes: the solve at 1e-8 against a plain handle's dotmi_spmv and solve.
2. steps under NEWTON_PCG_DIST | FORCE_DIST against the oracle's exact one-subdomain Newton.
3. 2, 3 and 4 ranks on one GPU (processes, a gloo all-reduce hook that records every call's payload size, a time-limited join):
   ranks bit-identical, the single-GPU DOTMI_FLAG_NEWTON_PCG run's Newton iterations and halvings, the payload histogram.
4. the flag on one rank without FORCE_DIST is DOTMI_FLAG_NEWTON_PCG, bit for bit.
5. refusals.
6. dotmi_solve_hessian on a plain sharded DOT handle leaves its DOT steps alone.

Sharding modes (DOTMI_SHARD_ELEMS, DOTMI_SHARD_HESS): "replicated" 0 / - (replicated element pass and Hessian), "elems" 1 / 0 (sharded
element pass, replicated Hessian), "rows" 1 / 1 (sharded Hessian rows: the second collective of a CG iteration).
Shapes: synbar:16x5x5:4 (612 vertices: a row slice is a fraction of one trip of the row kernel's lane groups), synbar:48x4x4:12 (slices
of 3 and 4 ranks that are no multiple of anything), bunny5K_LTSS / 8 (dup <= 5: subdomains share vertices across ranks)."""
import collections
import os
import sys
import tempfile

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import oracle_py as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAR4, BAR12, BUNNY = "synbar:16x5x5:4", "synbar:48x4x4:12", "bunny5K_LTSS"
MODES = {"replicated": ("0", "0"), "elems": ("1", "0"), "rows": ("1", "1")}
DIST = dl.DOTMI_FLAG_NEWTON_PCG_DIST | dl.FLAG_FORCE_DIST
_cache = {}


def set_mode(monkeypatch, mode):
    monkeypatch.setenv("DOTMI_SHARD_ELEMS", MODES[mode][0])
    monkeypatch.setenv("DOTMI_SHARD_HESS", MODES[mode][1])


def scripted(sc, ts, orc=None):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    if orc is not None:
        orc.move(idx, pos)


def plain_two_steps_in(name):
    """a plain DOT handle two steps into the script, the handles moved for the third, refactored there, with its solve of H u = -g at
    1e-8: once per mesh, shared and left unchanged (call it before the sharding mode is set)"""
    if ("solve", name) not in _cache:
        sc, ep, n = load_workload(name)
        ts = DOTTimeStepper(sc, ep, n)
        for _ in range(2):
            scripted(sc, ts)
            assert ts.step().status == 0
        scripted(sc, ts)
        ts.updatePrecondMtrAndFactorize()
        x = ts.getResult()
        b = -ts.computeGradient(x)
        u, it, res = ts.solveHessian(b, 1e-8, 500)
        assert ts.last_solve_status == 0
        _cache["solve", name] = dict(ts=ts, x=x, b=b, u=u, it=it, res=res)
    return _cache["solve", name]


def newton_pcg_run(name, steps):
    """the single-GPU DOTMI_FLAG_NEWTON_PCG run at eta = 1e-10: [(status, iters, halvings)], positions per step; once per case"""
    if ("steps", name, steps) not in _cache:
        sc, ep, n = load_workload(name)
        ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, iter_cap=50)
        ts.setPCG(1e-10, 500, 4)
        counts, xs = [], []
        for _ in range(steps):
            scripted(sc, ts)
            st = ts.step()
            counts.append((st.status, st.iters, st.ls_halvings))
            xs.append(ts.getResult())
        ts.close()
        _cache["steps", name, steps] = (counts, xs)
    return _cache["steps", name, steps]


# ---- 1. one rank under FORCE_DIST: the solve ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", [BAR4, BUNNY])
def test_sharded_solve_reaches_the_tolerance_like_the_plain_handles_and_repeats_bit_for_bit(name, mode, monkeypatch):
    """FORCE_DIST handle refactored at the plain handle's positions two steps in, the same b = -g: true residual <= 2e-8 against the
    PLAIN handle's dotmi_spmv (the standing bound of tests/test_gpu_newton_pcg.py), iterations within 1 of the plain solve, u within
    1e-10 relative of it, repeated solves and every read-back interval bit-identical, b = 0 in 0 iterations"""
    ref = plain_two_steps_in(name)
    set_mode(monkeypatch, mode)
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_FORCE_DIST)
    ts.updatePrecondMtrAndFactorize(ref["x"])
    b = ref["b"]
    u, it, res = ts.solveHessian(b, 1e-8, 500)
    assert ts.last_solve_status == 0
    true = np.linalg.norm(b - ref["ts"].multiply(u)) / np.linalg.norm(b)
    du = np.linalg.norm(u - ref["u"]) / np.linalg.norm(ref["u"])
    print(f"{name}, {mode}: {it} iterations (plain {ref['it']}), recursive {res:.3e}, true {true:.3e}, u against the plain solve {du:.2e}")
    assert res <= 1e-8 and true <= 2e-8
    assert abs(it - ref["it"]) <= 1
    assert du <= 1e-10
    u2, it2, res2 = ts.solveHessian(b, 1e-8, 500)
    assert np.array_equal(u2, u) and (it2, res2) == (it, res)
    for every in (1, 4, 8):
        ts.setPCG(1e-3, 500, every)
        ue, ite, rese = ts.solveHessian(b, 1e-8, 500)
        assert np.array_equal(ue, u) and (ite, rese) == (it, res), every
    assert ts.pcgInfo() == (5, 5 * it, it, res)
    u0, it0, res0 = ts.solveHessian(np.zeros_like(b), 1e-8, 500)
    assert ts.last_solve_status == 0 and it0 == 0 and res0 == 0.0 and not u0.any()
    ts.close()


# ---- 2. steps against the oracle's exact Newton ------------------------------------------------------------------------------------------
def oracle_newton_run(steps):
    if "oracle" not in _cache:
        sc, ep, n = load_workload(BAR4)
        cfg = sc.cfg
        one = np.zeros(sc.T.shape[0], dtype=np.int32)
        orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, one, 1, cfg.with_gravity)
        out = []
        for _ in range(steps):
            idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
            orc.move(idx, pos)
            so = orc.step_newton()
            out.append(((so.status, so.iters, so.ls_halvings), orc.state()[0].copy()))
        orc.close()
        _cache["oracle"] = out
    return _cache["oracle"]


@pytest.mark.parametrize("mode", list(MODES))
def test_sharded_steps_on_four_subdomains_match_the_oracles_exact_newton(mode, monkeypatch):
    """three steps of the bar on 4 subdomains at eta = 1e-10: the oracle's Newton iterations and halvings, positions to 1e-9 (the bound
    of test_steps_on_four_subdomains_match_the_oracles_exact_newton)"""
    want = oracle_newton_run(3)
    set_mode(monkeypatch, mode)
    sc, ep, n = load_workload(BAR4)
    assert n == 4
    ts = DOTTimeStepper(sc, ep, n, flags=DIST, iter_cap=50)
    ts.setPCG(1e-10, 500, 4)
    solves = total = 0
    for k in range(3):
        scripted(sc, ts)
        st = ts.step()
        ns, ni, last, lres = ts.pcgInfo()
        dx = np.abs(ts.getResult() - want[k][1]).max()
        print(f"{mode}, step {k}: Newton iterations {st.iters}, halvings {st.ls_halvings} (oracle {want[k][0]}), {ni - total} CG iterations "
              f"in {ns - solves} solves, {st.collective_calls} collectives of {st.collective_bytes} bytes, positions {dx:.2e}")
        assert (st.status, st.iters, st.ls_halvings) == want[k][0], k
        assert st.status == 0 and st.g2 <= ts.targetGRes
        assert dx < 1e-9, k
        assert ns - solves == st.iters and st.backsolve_launches == ni - total, k
        assert lres <= 1e-10
        assert st.collective_calls >= (2 if mode == "rows" else 1) * (ni - total)
        solves, total = ns, ni
    ts.close()


# ---- 3. several ranks on one GPU through the hook ----------------------------------------------------------------------------------------
def _worker(rank, world, initfile, outdir, workload, mode, steps):
    sys.path.insert(0, ROOT)
    os.environ["DOTMI_SHARD_ELEMS"], os.environ["DOTMI_SHARD_HESS"] = MODES[mode]
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    sizes = []

    def allreduce(a):
        sizes.append(a.nbytes)
        dist.all_reduce(torch.from_numpy(a))

    sc, ep, n = load_workload(workload)
    ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world, allreduce=allreduce, flags=dl.DOTMI_FLAG_NEWTON_PCG_DIST, iter_cap=50)
    ts.setPCG(1e-10, 500, 1)            # a read-back after every iteration: the enqueued iterations are the iterations done
    counts, xs, stats, hists, infos = [], [], [], [], []
    for _ in range(steps):
        scripted(sc, ts)
        del sizes[:]
        st = ts.step()
        counts.append((st.status, st.iters, st.ls_halvings))
        stats.append((st.backsolve_launches, st.energy_evals, st.collective_calls, st.collective_bytes))
        hists.append(np.array(sorted(collections.Counter(sizes).items())).reshape(-1, 2))
        xs.append(ts.getResult())
        infos.append(ts.pcgInfo())
    # the linear solve by itself, every rank together with the same b, and the refused coarse space
    b = -ts.computeGradient(ts.getResult())
    ts.updatePrecondMtrAndFactorize()
    ts.setPCG(1e-3, 500, 5)
    del sizes[:]                        # batches of 5: the collectives of every ENQUEUED iteration, also behind the deciding one
    u, it, res = ts.solveHessian(b, 1e-8, 500)
    solve_hist = np.array(sorted(collections.Counter(sizes).items())).reshape(-1, 2)
    refused = 0
    try:
        ts.setPCGCoarse(1)
    except DotmiError as e:
        refused = int("single-rank" in str(e))
    out = dict(counts=np.array(counts), x=np.array(xs), v=ts.getState()[1], stats=np.array(stats), infos=np.array(infos), u=u,
               solve=np.array([it, res, ts.last_solve_status]), solve_hist=solve_hist, refused=refused, E=st.E)
    for k, h in enumerate(hists):
        out[f"hist{k}"] = h
    ts.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(workload, steps, mode, world):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        procs = [ctx.Process(target=_worker, args=(r, world, os.path.join(d, "init"), d, workload, mode, steps)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive, "a rank hung (ranks branched apart?)"
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(world)]


def check_histogram(hist, n3, mode, newton_its, cg_its, trials, calls, nbytes):
    """hist: {payload bytes: calls} of one step's collectives, seen by the hook.  Per CG iteration exactly one packet of 8 n bytes (the
    ranks' shares of zsum) and, with sharded Hessian rows, one of 8 (n + 2) ([s | gamma | delta]); per batch -- here per iteration
    -- the agreement packet of 9 doubles; the step's existing ones: per trial rank 0's control scalars (RED_K + 2 = 23 doubles) and,
    with the sharded element pass, [g ; E] (n + 1 doubles); per refresh (one per Newton iteration) the factorisations' joint verdict
    (2 doubles).  The multiset is derived from the step's counters and must add up to collective_calls / collective_bytes"""
    z, pkt, g, adopt, two, agree = 8 * n3, 8 * (n3 + 2), 8 * (n3 + 1), 8 * 23, 16, 72
    want = {z: cg_its, agree: cg_its, adopt: trials, two: newton_its}
    if mode == "rows":
        want[pkt] = cg_its
    if mode != "replicated":
        want[g] = trials
    assert hist == want, (hist, want)
    assert sum(hist.values()) == calls and sum(k * v for k, v in hist.items()) == nbytes


CASES = [(BAR4, 2), (BAR12, 3), (BAR12, 4), (BUNNY, 2)]


@pytest.mark.parametrize("mode", ["replicated", "rows"])
@pytest.mark.parametrize("workload,world", CASES)
def test_ranks_agree_and_reproduce_the_single_gpu_newton_pcg_run(workload, world, mode):
    steps = 2
    want_counts, want_xs = newton_pcg_run(workload, steps)
    Rk = run_ranks(workload, steps, mode, world)
    sc, ep, n = load_workload(workload)
    n3 = 3 * sc.V_rest.shape[0]
    for r in range(1, world):
        for k in Rk[0]:
            assert np.array_equal(Rk[0][k], Rk[r][k]), (r, k)
    counts = [tuple(c) for c in Rk[0]["counts"].tolist()]
    err = max(np.abs(a - b).max() for a, b in zip(Rk[0]["x"], want_xs))
    it, res, status = Rk[0]["solve"]
    print(f"{workload}, {mode}, world {world}: (status, Newton iterations, halvings) {counts} (single GPU {want_counts}), CG iterations "
          f"{Rk[0]['stats'][:, 0].tolist()}, positions {err:.2e}; the solve by itself {int(it)} iterations to {res:.2e}")
    assert counts == want_counts
    assert err < 1e-9
    assert status == 0 and res <= 1e-8 and Rk[0]["refused"] == 1
    # the solve by itself ran in batches of 5: every enqueued iteration issues its collectives, whatever the record says.  A solve of
    # j >= 1 iterations is decided in batch ceil(j / 5) -- by the device in iteration j + 1's prologue, or by the host when 5 divides j
    # --, so 5 ceil(j / 5) iterations were enqueued and ceil(j / 5) agreement packets sent (9 doubles; no trial, no refresh here).
    # (22 and 56 iterations on these meshes: 3 and 4 iterations are enqueued behind the deciding one)
    batches = -(-int(it) // 5)
    print(f"the solve by itself: {int(it)} iterations done, {5 * batches} enqueued in {batches} batches")
    want = {8 * n3: 5 * batches, 72: batches}
    if mode == "rows":
        want[8 * (n3 + 2)] = 5 * batches
    assert dict(Rk[0]["solve_hist"].tolist()) == want, (Rk[0]["solve_hist"].tolist(), want)
    total = 0
    for k in range(steps):
        cg, trials, calls, nbytes = (int(v) for v in Rk[0]["stats"][k])
        total += cg
        assert Rk[0]["infos"][k][1] == total and Rk[0]["infos"][k][3] <= 1e-10
        check_histogram(dict(Rk[0][f"hist{k}"].tolist()), n3, mode, counts[k][1], cg, trials, calls, nbytes)


# ---- 4. the flag on one rank without FORCE_DIST ------------------------------------------------------------------------------------------
def test_flag_on_a_single_rank_handle_is_newton_pcg_bit_for_bit():
    sc, ep, n = load_workload(BUNNY)
    assert n == 8
    a = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, iter_cap=50)
    b = DOTTimeStepper(sc, ep, n, flags=dl.DOTMI_FLAG_NEWTON_PCG_DIST, iter_cap=50)
    for k in range(2):
        idx, pos = sc.scripter.step(a.getResult(), sc.cfg.dt)
        a.setDirichlet(idx, pos)
        b.setDirichlet(idx, pos)
        sa, sb = a.step(), b.step()
        assert (sa.status, sa.iters, sa.ls_halvings, sa.backsolve_launches) == (sb.status, sb.iters, sb.ls_halvings, sb.backsolve_launches), k
        assert sb.collective_calls == 0
        assert np.array_equal(a.getResult(), b.getResult()), k
    assert a.pcgInfo() == b.pcgInfo()
    a.close()
    b.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE, "OWNER_EXCHANGE"), (dl.FLAG_GSDD, "GSDD"),
                                        (dl.FLAG_NEWTON, "NEWTON"), (dl.FLAG_LBFGS_PD, "LBFGS_PD"), (dl.FLAG_LBFGS_HI, "LBFGS_HI"),
                                        (dl.FLAG_ASYNC_REFRESH, "ASYNC_REFRESH"), (dl.FLAG_DOT_COARSE, "DOT_COARSE")])
def test_flag_is_refused_at_create_with_these_flags(flags, word):
    sc, ep, n = load_workload(BAR4)
    whole = flags in (dl.FLAG_LBFGS_PD, dl.FLAG_LBFGS_HI)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG_DIST: not with DOTMI_FLAG_" + word + " "):
        DOTTimeStepper(sc, None if whole else ep, 1 if whole else n, flags=flags | dl.DOTMI_FLAG_NEWTON_PCG_DIST, alpha_min=1.0 if whole else 0.1)


def test_flag_is_refused_on_a_vertex_partition_and_the_old_flags_checks_run_first():
    sc, ep, n = load_workload(BAR4)
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG_DIST: not with a vertex partition"):
        DOTTimeStepper(sc, ep, n, flags=dl.DOTMI_FLAG_NEWTON_PCG_DIST, vpart=np.zeros(sc.V_rest.shape[0], dtype=np.int32))
    with pytest.raises(DotmiError, match="DOTMI_FLAG_NEWTON_PCG: single GPU"):
        DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG | DIST)


@pytest.mark.parametrize("flag,word", [(dl.FLAG_LBFGS_PD, "LBFGS-PD"), (dl.FLAG_LBFGS_HI, "LBFGS-HI"), (dl.FLAG_GSDD, "GSDD")])
def test_solve_is_still_refused_on_handles_without_the_global_solve(flag, word):
    sc, ep, n = load_workload(BAR4)
    whole = flag != dl.FLAG_GSDD
    ts = DOTTimeStepper(sc, None if whole else ep, 1 if whole else n, flags=flag, alpha_min=1.0 if whole else 0.1)
    with pytest.raises(DotmiError, match="dotmi_solve_hessian.*" + word):
        ts.solveHessian(np.ones((sc.V_rest.shape[0], 3)))
    ts.close()


def test_solve_is_refused_on_an_owner_exchange_handle():
    """its vectors are valid on a rank's own vertices only and its refresh assembles no rows for the SpMV slice"""
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE)
    with pytest.raises(DotmiError, match="dotmi_solve_hessian.*DOTMI_FLAG_OWNER_EXCHANGE"):
        ts.solveHessian(np.ones((sc.V_rest.shape[0], 3)))
    ts.close()


def test_coarse_space_is_still_refused_on_a_sharded_handle_with_the_flag():
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=DIST)
    with pytest.raises(DotmiError, match="dotmi_set_pcg_coarse.*single-rank"):
        ts.setPCGCoarse(1)
    with pytest.raises(DotmiError, match="dotmi_pcg_apply_precond.*single-rank"):
        ts.pcgApplyPrecond(np.ones((sc.V_rest.shape[0], 3)))
    ts.close()


# ---- 6. the solve on a plain sharded DOT handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["replicated", "rows"])
def test_solve_on_a_sharded_dot_handle_leaves_its_steps_alone(mode, monkeypatch):
    sc, ep, n = load_workload(BAR4)
    plain = DOTTimeStepper(sc, ep, n)                          # (dotmi_spmv is refused where the Hessian rows are sharded)
    set_mode(monkeypatch, mode)
    a = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_FORCE_DIST)
    b = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_FORCE_DIST)
    rhs = -a.computeGradient(a.getResult() + 1e-3 * np.random.default_rng(5).standard_normal((sc.V_rest.shape[0], 3)))
    u, it, res = a.solveHessian(rhs, 1e-8, 500)
    assert a.last_solve_status == 0 and it >= 1 and res <= 1e-8
    assert np.linalg.norm(rhs - plain.multiply(u)) <= 2e-8 * np.linalg.norm(rhs)
    plain.close()
    for k in range(3):
        idx, pos = sc.scripter.step(a.getResult(), sc.cfg.dt)
        a.setDirichlet(idx, pos)
        b.setDirichlet(idx, pos)
        sa, sb = a.step(), b.step()
        assert (sa.status, sa.iters, sa.ls_halvings) == (sb.status, sb.iters, sb.ls_halvings), k
        assert np.array_equal(a.getResult(), b.getResult()), k
        if k == 0:
            a.solveHessian(rhs, 1e-8, 500)                     # ... and between two steps
    a.close()
    b.close()
