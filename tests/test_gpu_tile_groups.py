"""Subdomain groups of the tile factorisation's level launches (DOTMI_TILE_GROUPS; dot_amd/csrc/tile_factor.hpp, issue_factor in
dotmi_refresh.hip) on the GPU: every group's levels run on a stream of its own between one fork and one join.  The groups share no
tile and every tile is still written by one task at a time in the same product order, so factors, iteration counts and positions
are those of the single chain bit for bit -- replayed from the captured graph and issued directly.  bunny5K, 8 subdomains, with
DOTMI_TILE_FLOW=0 so that the level launches run (the dataflow launch is that layout's default)."""
import os
import sys

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD, NPARTS = "bunny5K_LTSS", 8


def _create(groups, graph=1, flags=0):
    env = {"DOTMI_TILE_FLOW": "0", "DOTMI_TILE_GROUPS": str(groups), "DOTMI_FACTOR_GRAPH": str(graph)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sc, ep, n = load_workload(WORKLOAD)
        ts = DOTTimeStepper(sc, ep, n, flags=flags)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert n == NPARTS and dl.load().dotmi_factor_kind(ts._h) == 1          # level launches
    return sc, ts


def _step(sc, ts):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    return ts.step()


def _factors(ts):
    return [ts.partMatrix(p, inverse=True)[0] for p in range(NPARTS)]


def _factors_after_a_step(groups, graph, refactors=0):
    """the inverse factors of every subdomain after one scripted step (its refresh factorises H at the new positions) and
    `refactors` further factorisations of the same positions"""
    sc, ts = _create(groups, graph)
    used = dl.load().dotmi_factor_groups(ts._h)
    st = _step(sc, ts)
    assert st.status == 0
    for _ in range(refactors):
        ts.updatePrecondMtrAndFactorize()
    X = _factors(ts)
    ts.close()
    return used, (st.iters, st.ls_halvings), X


@pytest.fixture(scope="module")
def single_chain():
    used, its, X = _factors_after_a_step(1, 1)
    assert used == 1
    return its, X


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("groups,expect", [(2, 2), (3, 3), (16, 4)])
def test_grouped_chains_give_the_single_chains_factors_bit_for_bit(single_chain, groups, expect, graph):
    """2 groups, 3 groups (3 / 3 / 2 subdomains) and 16 (clamped to the four streams a handle uses), as a replayed graph with
    independent branches and as direct launches on the groups' streams"""
    used, its, X = _factors_after_a_step(groups, graph)
    assert used == expect
    assert its == single_chain[0]
    for p, (A, B) in enumerate(zip(single_chain[1], X)):
        assert np.isfinite(B).all()
        assert np.array_equal(A, B), (p, np.abs(A - B).max())


@pytest.mark.parametrize("graph", [0, 1])
def test_a_second_factorisation_waits_for_every_group_of_the_first(single_chain, graph):
    """dotmi_refactor twice in a row on three groups: the second call's clear and fill are ordered behind the join, so they
    cannot overtake a group that is still factoring -- the factors are the single chain's"""
    used, _, X = _factors_after_a_step(3, graph, refactors=2)
    assert used == 3
    _, _, X1 = _factors_after_a_step(1, graph, refactors=2)
    for A, B, C_ in zip(single_chain[1], X, X1):
        assert np.array_equal(A, B) and np.array_equal(C_, B)


def test_steps_with_the_asynchronous_refresh_are_the_single_chains():
    runs = []
    for groups in (1, 2):
        sc, ts = _create(groups, flags=dl.FLAG_ASYNC_REFRESH)
        assert dl.load().dotmi_factor_groups(ts._h) == groups
        rows = []
        for _ in range(3):
            st = _step(sc, ts)
            rows.append((st.status, st.iters, st.ls_halvings))
        runs.append((rows, ts.getResult().copy()))
        ts.close()
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert all(r[0] == 0 for r in runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1])


def _refresh_failure_worker(q):
    """in a process of its own, on the build with the test hooks (tests/test_gpu_round4.py::_async_failure_worker): the refresh at
    the end of step 1 reports a bad pivot while two groups factorise"""
    sys.path.insert(0, ROOT)
    from dot_amd import lib as dl_
    from dot_amd.timestepper import DOTTimeStepper as TS
    from tests.workloads import load_workload as lw
    out = {}
    try:
        sc, ep, n = lw(WORKLOAD)
        ts = TS(sc, ep, n, flags=dl_.FLAG_ASYNC_REFRESH)
        out["groups"] = dl_.load().dotmi_factor_groups(ts._h)
        sc.scripter.track(sc.x0)
        for k in range(2):
            idx, pos = sc.scripter.step(None, sc.cfg.dt)
            ts.setDirichlet(idx, pos)
            out[f"status{k}"] = ts.step().status       # step 1 returns with its (failing) refresh still queued
        idx, pos = sc.scripter.step(None, sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        try:
            ts.step()
            out["step"] = "no error"
        except dl_.DotmiError as e:
            out["step"] = str(e)
        ts.updatePrecondMtrAndFactorize(ts.getResult())     # a good factorisation heals the handle
        out["healed"] = ts.step().status
        ts.close()
    except Exception as e:   # noqa: BLE001
        out["exception"] = repr(e)
    q.put(out)


def test_a_failed_refresh_on_two_groups_still_stops_the_next_step():
    """enter_with_factors: the verdict of the refresh a step left running is taken before anything is enqueued -- with the
    factorisation on two streams as with one: the next dotmi_step returns DOTMI_E_NOTSPD (-3)"""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_refresh_failure_worker, args=(q,))
    # 1 = the factorisation in dotmi_create, 2 = the refresh at the end of step 0, 3 = the one at the end of step 1
    hook = {"DOTMI_LIBRARY": os.path.join(ROOT, "dot_amd", "libdotmi_testhooks.so"), "DOTMI_TEST_FAIL_REFRESH": "3",
            "DOTMI_TILE_FLOW": "0", "DOTMI_TILE_GROUPS": "2"}
    os.environ.update(hook)
    try:
        p.start()
    finally:
        for k in hook:
            del os.environ[k]
    out = q.get(timeout=300)
    p.join(timeout=60)
    assert "exception" not in out, out
    assert out["groups"] == 2, out
    assert out["status0"] == 0 and out["status1"] == 0, out
    assert "-3" in out["step"], out
    assert out["healed"] == 0, out
