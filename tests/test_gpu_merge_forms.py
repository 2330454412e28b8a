"""The storage forms of the merge give the same bits (dot_amd/csrc/merge_sum.hpp): DOTMI_SPLIT_MERGE=0 -- the
walk over a dof's list of tile partials inside the merge kernel -- against DOTMI_SPLIT_MERGE=1 -- reduce_partial_p_kernel leaves the
subdomains' own sums and the merge kernel gathers them --, np.array_equal on one application of the preconditioner to a fixed
random vector, on the positions after each of two device-loop steps, with the steps' iterations and halvings, and on one more
application behind the steps.

Four handles each way: plain; DOTMI_FLAG_FORCE_DIST on one rank (the undivided merge, then the zsum branch of
merge_tiles_early_kernel; applyPrecond: zfinish_kernel); and both with the rigid-mode coarse term -- setDotCoarse(1) on the plain
handle, DOTMI_FLAG_DOT_COARSE on the sharded one, where setDotCoarse is refused and the flag is the only way to the term.

Shape: synbar:4x4x2:3, 192 tets and 75 vertices, the smallest synthetic bar (by tets, over nx <= 12, ny <= 6, nz <= 3 and 3, 4, 6
or 8 subdomains) whose partition puts a vertex into three subdomains and whose padded subdomain size exceeds 128 (nmax = 192: three
row tiles, so a column's partial sum comes from more than one tile).  The test asserts both.  merge_check (tests/test_merge_sum.py)
compares the forms on the CPU on designed lists; this is the same claim through the kernels and their launchers."""
import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.sharding import plan_layout
from dot_amd.timestepper import DOTTimeStepper
from dot_amd.workloads import load_workload

pytestmark = pytest.mark.gpu

BAR = "synbar:4x4x2:3"
STEPS = 2


def run(flags, set_mode):
    sc, ep, n = load_workload(BAR)
    fixed = np.asarray(sc.fixed, dtype=bool)
    r = np.random.default_rng(29).standard_normal((fixed.size, 3))
    r[fixed] = 0.0
    ts = DOTTimeStepper(sc, ep, n, flags=flags)
    if set_mode:
        ts.setDotCoarse(1)
    coarse = ts.dotCoarseInfo()[:3]
    out = dict(z0=ts.applyPrecond(r), counts=[], xs=[], coarse=coarse)
    for _ in range(STEPS):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        out["counts"].append((st.iters, st.ls_halvings, st.status))
        out["xs"].append(ts.getResult().copy())
    out["z1"] = ts.applyPrecond(r)
    ts.close()
    return out


def test_the_bar_has_a_vertex_in_three_subdomains_and_columns_in_more_than_one_tile():
    sc, ep, n = load_workload(BAR)
    T = np.asarray(sc.T)
    held = np.zeros(sc.V_rest.shape[0], dtype=int)
    for s in range(n):
        held[np.unique(T[np.asarray(ep) == s])] += 1
    nmax = plan_layout(sc.V_rest, sc.T, ep, n)[1]
    assert held.max() >= 3
    assert nmax > 128


CASES = [("plain", 0, False), ("plain, coarse term", 0, True), ("one rank sharded", dl.FLAG_FORCE_DIST, False),
         ("one rank sharded, coarse term", dl.FLAG_FORCE_DIST | dl.FLAG_DOT_COARSE, False)]


@pytest.mark.parametrize("case,flags,set_mode", CASES, ids=[c[0] for c in CASES])
def test_list_walk_and_split_merge_give_the_same_bits(case, flags, set_mode, monkeypatch):
    monkeypatch.setenv("DOTMI_SPLIT_MERGE", "0")
    walk = run(flags, set_mode)
    monkeypatch.setenv("DOTMI_SPLIT_MERGE", "1")
    split = run(flags, set_mode)
    print(f"{case}: {walk['counts']}, coarse (dimension, dropped, active) {walk['coarse']}")
    assert walk["coarse"] == split["coarse"] == ((18, 0, 1) if "coarse" in case else (0, 0, 0))
    assert all(c[2] == 0 and c[0] > 0 for c in walk["counts"])
    assert walk["counts"] == split["counts"]
    assert np.abs(walk["z0"]).max() > 0.0
    assert np.array_equal(walk["z0"], split["z0"])
    for a, b in zip(walk["xs"], split["xs"]):
        assert np.array_equal(a, b)
    assert np.array_equal(walk["z1"], split["z1"])
