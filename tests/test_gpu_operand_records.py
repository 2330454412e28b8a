"""DOTMI_OPERAND_RECORDS (round 9): elem_vertex_kernel reads its per-owned-vertex operands as records -- the static ones in patch
order, the stored L-BFGS pairs as (s, y) entries, p and x~ of the owned dofs through LDS -- instead of 8-byte gathers behind the
vertex id.  The same values enter the same operations, so the default and DOTMI_OPERAND_RECORDS=0 (the flat arrays) must agree bit
for bit: status, iterations, halvings, energy evaluations, the per-iteration log, positions and velocities.  Two handles in one
process (the switch is read by dotmi_create), through the C ABI on the GPU."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.scene import Config, build_scene, partition_rcb, synthetic_bar
from dot_amd.timestepper import DOTTimeStepper
from dot_amd.workloads import load_workload

pytestmark = pytest.mark.gpu


def _stiff_bar():
    """24 x 6 x 6 bar (1 225 vertices, 5 184 tets) in 8 parts, Stable Neo-Hookean, twist, dt 0.1, YM 1e6, PR 0.45: stiff enough for
    thirty-odd iterations and a halving in every step -- the history (five pairs) wraps many times and retry slots read it"""
    V, T = synthetic_bar(24, 6, 6)
    assert (V.shape[0], T.shape[0]) == (1225, 5184)
    cfg = Config(energy="SNH", size=1.0, duration=5.0, dt=0.1, rho=1000.0, YM=1e6, PR=0.45, script="twist")
    sc = build_scene(cfg, V, T)
    return sc, partition_rcb(sc.V_rest, sc.T, 8), 8


_cache = {}


def _run(make, steps, records, monkeypatch, env=None, refix_after=None):
    """(a run is a pure function of its arguments: tests that need the same one share it)"""
    key = (make.__name__, steps, records, tuple(sorted((env or {}).items())), refix_after)
    if key not in _cache:
        _cache[key] = _run_once(make, steps, records, monkeypatch, env, refix_after)
    return _cache[key]


def _run_once(make, steps, records, monkeypatch, env, refix_after):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if records is None:
        monkeypatch.delenv("DOTMI_OPERAND_RECORDS", raising=False)
    else:
        monkeypatch.setenv("DOTMI_OPERAND_RECORDS", records)
    sc, ep, n = make()
    ts = DOTTimeStepper(sc, ep, n)
    rec, logs = [], []
    try:
        for k in range(steps):
            if refix_after is not None and k == refix_after:
                # a changed fixed set on the live handle: every 11th free vertex is held where it is from now on
                fixed = np.ascontiguousarray(sc.fixed, dtype=np.uint8).copy()
                free = np.nonzero(fixed == 0)[0]
                fixed[free[::11]] = 1
                assert fixed.sum() > sc.fixed.astype(bool).sum()
                ts.refix(fixed)
            x = ts.getResult()
            idx, pos = sc.scripter.step(x, sc.cfg.dt)
            ts.setDirichlet(idx, pos)
            st = ts.step()
            rec.append((st.status, st.iters, st.ls_halvings, st.energy_evals, st.E, st.g2, st.E0, st.g2_0, st.paired_slots))
            logs.append(tuple(np.array(v).copy() for v in ts.iterLog()))
        x = ts.getResult().copy()
        v = ts.getState()[1].copy()
        # the handle runs its trials on vertex patches (the kernel under test): its launch is a bench kind only there
        ms, nb = C.c_double(), C.c_int64()
        assert dl.load().dotmi_bench_kernel(ts._h, dl.BENCH_KERNELS.index("elem_vertex"), 1, C.byref(ms), C.byref(nb)) == 0
        # ... and it does so on the loads the run is meant to compare: records by default, the flat arrays with the switch at 0
        assert dl.load().dotmi_operand_records(ts._h) == (0 if records == "0" else 1)
    finally:
        ts.close()
    return rec, logs, x, v


def _same(a, b):
    (rec0, log0, x0, v0), (rec1, log1, x1, v1) = a, b
    assert rec0 == rec1, (rec0, rec1)
    for (a0, e0, g0), (a1, e1, g1) in zip(log0, log1):
        assert np.array_equal(a0, a1) and np.array_equal(e0, e1) and np.array_equal(g0, g1)
    assert np.array_equal(x0, x1) and np.array_equal(v0, v1)


def _exercised(rec):
    """more iterations than the history holds pairs, and a retry slot, in every step"""
    for k, r in enumerate(rec):
        assert r[0] == 0 and r[1] > 7 and r[2] >= 1, (k, r)


def test_stiff_bar_records_and_flat_arrays_take_the_same_steps_bit_for_bit(monkeypatch):
    on = _run(_stiff_bar, 4, None, monkeypatch)
    off = _run(_stiff_bar, 4, "0", monkeypatch)
    print("stiff bar:", [(r[1], r[2]) for r in on[0]], "iterations, halvings")
    _exercised(on[0])
    _same(on, off)


def test_stiff_bar_paired_trials_on_vertex_patches_bit_for_bit(monkeypatch):
    """elem_vertex_kernel<MAT, PAIR = true, REC>: every step pairs its trials, on vertex patches (forced)"""
    env = {"DOTMI_PAIR_TRIALS": "1", "DOTMI_VERTEX_PATCHES": "1"}
    on = _run(_stiff_bar, 4, None, monkeypatch, env)
    off = _run(_stiff_bar, 4, "0", monkeypatch, env)
    print("stiff bar, paired:", [(r[1], r[2], r[8]) for r in on[0]], "iterations, halvings, paired slots")
    _exercised(on[0])
    _same(on, off)


def test_stiff_bar_refix_rewrites_the_patch_order_flags(monkeypatch):
    """dotmi_refix between steps 2 and 3: the patch-order copy of `fixed` follows in the same call"""
    on = _run(_stiff_bar, 4, None, monkeypatch, refix_after=2)
    off = _run(_stiff_bar, 4, "0", monkeypatch, refix_after=2)
    plain = _run(_stiff_bar, 4, None, monkeypatch)
    print("stiff bar, refix:", [(r[1], r[2]) for r in on[0]], "iterations, halvings")
    _exercised(on[0])
    _same(on, off)
    assert on[0][:2] == plain[0][:2] and on[0][2:] != plain[0][2:]       # (the new mask does change the last two steps)


def test_bunny_vertices_with_more_than_four_copies_bit_for_bit(monkeypatch):
    """bunny5K in 8 parts, vertex patches forced (fixed-corotational: elem_vertex_kernel<0, ., REC>): some vertices lie in five
    subdomains, so their -g goes to a fifth padded right-hand side through the flat lists behind the record's four positions"""
    env = {"DOTMI_PAIR_TRIALS": "0", "DOTMI_SPEC_STEP": "0", "DOTMI_VERTEX_PATCHES": "1"}

    def bunny():
        return load_workload("bunny5K_LTSS")
    sc, ep, n = bunny()
    copies = np.zeros(sc.V_rest.shape[0], dtype=np.int64)
    for p in range(n):
        copies[np.unique(np.asarray(sc.T)[np.asarray(ep) == p])] += 1
    assert n == 8 and copies.max() > 4
    on = _run(bunny, 3, None, monkeypatch, env)
    off = _run(bunny, 3, "0", monkeypatch, env)
    print("bunny5K:", [(r[1], r[2]) for r in on[0]], "iterations, halvings; most copies of a vertex", int(copies.max()))
    assert all(r[0] == 0 and r[1] >= 1 for r in on[0])
    _same(on, off)


def test_stiff_monkey_rejected_first_trials_bit_for_bit(monkeypatch):
    """one step of monkey18K_stiff with vertex patches forced (tests/test_gpu_round6.py): rejected first trials on a real mesh"""
    env = {"DOTMI_PAIR_TRIALS": "0", "DOTMI_SPEC_STEP": "0", "DOTMI_VERTEX_PATCHES": "1"}
    def make():
        return load_workload("monkey18K_stiff")
    on = _run(make, 1, None, monkeypatch, env)
    off = _run(make, 1, "0", monkeypatch, env)
    print("stiff monkey:", on[0][0][:4])
    assert on[0][0][0] == 0 and on[0][0][2] >= 1
    _same(on, off)
