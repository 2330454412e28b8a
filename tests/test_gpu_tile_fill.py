"""H tiles built inside their first tile task (DOTMI_TILE_HFILL, the default; dot_amd/csrc/k_tilefactor.hip tile_fill_build, the
init == 2 tasks of tile_factor.hpp) on the GPU, held against DOTMI_TILE_HFILL=0 -- the work buffer cleared and filled with H in
front of every factorisation, the tile read back by its first task.  The products, their order and the stores are the same, so
every factor is the same bit for bit, in every launch form of the factorisation: one launch per level with one and two subdomain
groups (replayed from the graph and issued directly), the dataflow launch, the split levels with their half-tile kernel, and
the two-level form.  bunny5K / 8 subdomains and synbar:16x5x5:2, whose tiles hold identity padding."""
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu

LEVELS = {"DOTMI_TILE_FLOW": "0", "DOTMI_TILE_SPLIT": "0", "DOTMI_TWO_LEVEL": "0"}
FORMS = {
    "levels-1-graph": dict(LEVELS, DOTMI_TILE_GROUPS="1", DOTMI_FACTOR_GRAPH="1"),
    "levels-1-direct": dict(LEVELS, DOTMI_TILE_GROUPS="1", DOTMI_FACTOR_GRAPH="0"),
    "levels-2-graph": dict(LEVELS, DOTMI_TILE_GROUPS="2", DOTMI_FACTOR_GRAPH="1"),
    "levels-2-direct": dict(LEVELS, DOTMI_TILE_GROUPS="2", DOTMI_FACTOR_GRAPH="0"),
    "flow": {"DOTMI_TILE_FLOW": "1", "DOTMI_TWO_LEVEL": "0"},
    "split": {"DOTMI_TILE_FLOW": "0", "DOTMI_TILE_SPLIT": "1", "DOTMI_TWO_LEVEL": "0"},
    "two-level": {"DOTMI_TWO_LEVEL": "1"},
}
# factor kinds (dotmi_factor_kind): 1 = one launch per level, 2 = dataflow, 3 = split levels
KIND = {"flow": 2, "split": 3}


def _create(name, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        sc, ep, n = load_workload(name)
        ts = DOTTimeStepper(sc, ep, n)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return sc, n, ts


def _step(sc, ts):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)
    return ts.step()


def _run(name, form, hfill):
    """one handle through the scripted calls; what it leaves after each"""
    sc, n, ts = _create(name, dict(FORMS[form], DOTMI_TILE_HFILL=str(hfill)))
    two_level = form == "two-level"
    assert ts.backsolveForm() == (1 if two_level else 0)
    if form in KIND:
        assert dl.load().dotmi_factor_kind(ts._h) == KIND[form]
    elif form.startswith("levels"):
        assert dl.load().dotmi_factor_kind(ts._h) == 1
        assert dl.load().dotmi_factor_groups(ts._h) == int(form.split("-")[1])
    r = np.random.default_rng(20240819).standard_normal((sc.V_rest.shape[0], 3))
    r[np.asarray(sc.fixed).astype(bool)] = 0

    def factors():
        # (the two-level form keeps no explicit inverse of a subdomain: one application of the block solve instead)
        return [ts.applyPrecond(r)] if two_level else [ts.partMatrix(p, inverse=True)[0] for p in range(n)]

    out = {}
    rows = []
    for k in range(3):
        st = _step(sc, ts)
        rows.append((st.status, st.iters, st.ls_halvings))
        if k == 0:
            out["after one step"] = factors()
    out["three steps"] = (rows, ts.getResult().copy())
    ts.updatePrecondMtrAndFactorize()
    out["one further factorisation"] = factors()
    ts.updatePrecondMtrAndFactorize()
    out["two further factorisations"] = factors()
    fixed = np.asarray(sc.fixed).astype(np.uint8).copy()
    free = np.flatnonzero(fixed == 0)
    fixed[free[:: max(1, len(free) // 7)]] = 1          # a handful of further vertices held
    ts.refix(fixed)
    out["after refix"] = factors()
    ts.setLame(ts._mu * 1.25, ts._lam * 0.75)
    out["after setLame"] = factors()
    ts.close()
    return out


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", ["bunny5K_LTSS", "synbar:16x5x5:2"])
def test_tiles_built_from_their_lists_give_the_filled_buffers_factors_bit_for_bit(name, form):
    if name == "bunny5K_LTSS":
        assert load_workload(name)[2] == 8
    a, b = _run(name, form, 0), _run(name, form, 1)
    assert all(s == 0 for s, _, _ in a["three steps"][0]), a["three steps"][0]
    assert a["three steps"][0] == b["three steps"][0], (a["three steps"][0], b["three steps"][0])
    assert np.array_equal(a["three steps"][1], b["three steps"][1])
    for what in ("after one step", "one further factorisation", "two further factorisations", "after refix", "after setLame"):
        assert len(a[what]) == len(b[what]) > 0
        for p, (A, B) in enumerate(zip(a[what], b[what])):
            assert np.isfinite(B).all(), (what, p)
            assert np.array_equal(A, B), (what, p, float(np.abs(A - B).max()))
    # with no clear in front of them, further factorisations at the same positions must return the same factors again: a stale
    # tile of the work buffer would show here
    for A, B in zip(b["one further factorisation"], b["two further factorisations"]):
        assert np.array_equal(A, B)
    # (and the calls in between did move the factors at all)
    assert any(not np.array_equal(A, B) for A, B in zip(b["after one step"], b["two further factorisations"]))
    assert any(not np.array_equal(A, B) for A, B in zip(b["after refix"], b["two further factorisations"]))
