"""The wide forms of three kernels of the L-BFGS iteration -- vertex_gather_kernel<true, 512, 2>, merge_tiles_early_kernel<512, .> and
spmv_zp_wide_kernel (1024 threads); dot_amd/csrc/k_loopvec.hip -- which a mesh selects by its size (dot_amd/csrc/loop_forms.hpp: beyond
524 288 dofs, 131 072 dofs and 24 576 rows) and which therefore no mesh small enough to step against the oracle ever ran.
DOTMI_WIDE_FORMS forces them (a bit mask: 1 gather, 2 early merge, 4 direction kernel; a clear bit forces the narrow form), so here

  (a) each wide form alone, and all three, against the oracle on bunny5K (14 010 dofs: 27 full 512-thread workgroups, a partial one and
      228 with nothing to do), horse7K (back-tracks) and a bar of 432 dofs (less than one workgroup);
  (b) all wide against all narrow on the same meshes;
  (c) the combinations big meshes run by default and small ones never do: the wide merge behind the split merge (psub), with the coarse
      term (the COARSE instantiation), and all three on two ranks, summed by all-reduce and by the owner exchange (vl, kind, gshare,
      zshare);
  (d) one bar just past the merge's and the direction kernel's thresholds, chosen by size: a full first trip and a short second one.

Every run first asserts that DOTTimeStepper.loopForms() -- computed from the handle's own counts by the functions the launchers call --
shows the forms it means to run: a switch that is silently ignored fails here.  Through the C ABI on the GPU; the switch is read by
dotmi_create, so it is set around the constructor and restored (tests/test_gpu_two_level.py).

Bounds.  Against the oracle: status, iterations and halvings of every step, positions to 1e-9
(tests/test_gpu_round3.py::test_tuning_switches_do_not_change_results).  Form against form: the same decisions, positions to 1e-9 after a
step without back-tracking and 1e-6 after one with it -- the bounds of tests/test_gpu_designed_states.py for forms that group their sums
differently; E0 of the first step bit for bit (the energy partials are per patch, no form under test touches them, and the first step
starts from the same bits; later steps start from positions that agree to rounding only); |g|^2 at the start of the first step within
2 n eps / (1 - n eps), n = 3 nV, relative: both forms add the same n non-negative terms g_k^2, every g_k the same sum in the same
order, so each computed sum is within gamma_{n-1} of the true one -- a dropped or doubled dof would move it by about 1 / n."""
import os

import numpy as np
import pytest

from dot_amd.timestepper import DOTTimeStepper
from dot_amd.workloads import load_workload
from tests import oracle_py as O

pytestmark = pytest.mark.gpu

GATHER, MERGE, SPMV, SPLIT = 1, 2, 4, 8
EPS = np.finfo(np.float64).eps
# (mesh, switches every run on it takes): the two FCR meshes run on element patches by themselves -- the gather is a kernel of its own
# there --, the Stable Neo-Hookean bars only with the vertex patches off
MESHES = {"bunny5K_LTSS": {}, "horse7K_stretch": {}, "synbar:8x3x3:4": {"DOTMI_VERTEX_PATCHES": "0"}}
BAR4 = "synbar:16x5x5:4"
STEPS = 3


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_runs = {}


def device_run(name, mask, env=None, steps=STEPS, coarse=False, want_extra=0):
    """`steps` scripted steps of a fresh handle created under DOTMI_WIDE_FORMS=mask (None: unset) and `env`; asserts what the handle says
    it launches; -> (per step (status, iterations, halvings), per step positions, per step (E0, g2_0), loopForms).  A run is a function
    of its arguments: tests that need the same one share it"""
    key = (name, mask, tuple(sorted((env or {}).items())), steps, coarse)
    if key in _runs:
        return _runs[key]
    sc, ep, n = load_workload(name)
    e = dict(env or {})
    if mask is not None:
        e["DOTMI_WIDE_FORMS"] = str(mask)
    assert mask is not None or "DOTMI_WIDE_FORMS" not in os.environ
    ts = _with_env(e, lambda: DOTTimeStepper(sc, ep, n))
    try:
        forms = ts.loopForms()
        if mask is not None:
            assert forms & 7 == mask, (name, mask, forms)
        assert forms & want_extra == want_extra, (name, forms, want_extra)
        if coarse:
            ts.setDotCoarse(1)
            assert ts.dotCoarseInfo()[2] == 1
        counts, xs, starts = [], [], []
        for _ in range(steps):
            idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
            ts.setDirichlet(idx, pos)
            st = ts.step()
            counts.append((st.status, st.iters, st.ls_halvings))
            xs.append(ts.getResult().copy())
            starts.append((st.E0, st.g2_0))
        if coarse:
            assert ts.dotCoarseInfo()[2] == 1
    finally:
        ts.close()
    _runs[key] = (counts, xs, starts, forms)
    return _runs[key]


_oracle = {}


def oracle_run(name, steps=STEPS):
    """the oracle's steps on the same script, once per mesh (the handles' positions are the scripted ones to the bit)"""
    if name not in _oracle:
        sc, ep, n = load_workload(name)
        cfg = sc.cfg
        orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)
        try:
            counts, xs = [], []
            for _ in range(steps):
                idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
                orc.move(idx, pos)
                so = orc.step()
                counts.append((so.status, so.iters, so.ls_halvings))
                xs.append(np.array(orc.state()[0]).copy())
        finally:
            orc.close()
        _oracle[name] = (counts, xs)
    return _oracle[name]


def assert_same_to_rounding(a, b, nV, tag):
    """(b) of the module's text: form a against form b on the same mesh"""
    (ca, xa, sa, _), (cb, xb, sb, _) = a, b
    for k, (u, w) in enumerate(zip(sa, sb)):
        print(f"{tag} step {k}: {ca[k]} / {cb[k]}  max|dx| {float(np.abs(xa[k] - xb[k]).max()):.3e}  E0 {u[0]!r} / {w[0]!r}  "
              f"g2_0 {u[1]!r} / {w[1]!r}")
    assert ca == cb, tag
    assert all(c[0] == 0 for c in ca), tag
    for k in range(len(ca)):
        assert np.abs(xa[k] - xb[k]).max() < (1e-9 if ca[k][2] == 0 else 1e-6), (tag, k)
    assert sa[0][0] == sb[0][0], tag
    n = 3 * nV
    assert abs(sa[0][1] - sb[0][1]) <= 2 * n * EPS / (1 - n * EPS) * max(sa[0][1], sb[0][1]), tag


# ---- (a) each wide form against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", [GATHER, MERGE, SPMV, GATHER | MERGE | SPMV])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_forced_wide_forms_take_the_oracles_steps(name, mask):
    counts, xs, _, _ = device_run(name, mask, MESHES[name])
    ocounts, oxs = oracle_run(name)
    for k in range(STEPS):
        print(f"{name} mask {mask} step {k}: {counts[k]} oracle {ocounts[k]}  max|dx| {float(np.abs(xs[k] - oxs[k]).max()):.3e}")
    assert counts == ocounts
    for k in range(STEPS):
        assert np.abs(xs[k] - oxs[k]).max() < 1e-9, k
    if name == "bunny5K_LTSS":
        assert counts[0][2] > 0      # (its first step back-tracks: retry slots run through the forms too)


# ---- (b) all wide against all narrow ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_all_wide_against_all_narrow(name):
    nV = load_workload(name)[0].V_rest.shape[0]
    assert_same_to_rounding(device_run(name, 7, MESHES[name]), device_run(name, 0, MESHES[name]), nV, name)


# ---- (c) what big meshes combine the wide forms with ------------------------------------------------------------------------------------------
def test_wide_merge_behind_the_split_merge():
    """merge_tiles_early_kernel<512, false> reading the per-subdomain sums psub (from 400 k dofs by default: always with the wide merge)"""
    env = {"DOTMI_SPLIT_MERGE": "1"}
    nV = load_workload(BAR4)[0].V_rest.shape[0]
    assert_same_to_rounding(device_run(BAR4, MERGE, env, want_extra=SPLIT), device_run(BAR4, 0, env, want_extra=SPLIT), nV, "split merge")
    assert device_run(BAR4, 0)[3] & SPLIT == 0                 # (not what this mesh does by itself)


def test_wide_merge_with_the_coarse_term():
    """merge_tiles_early_kernel<512, true>: dotmi_set_dot_coarse on, as tests/test_gpu_dot_coarse.py sets it up"""
    nV = load_workload(BAR4)[0].V_rest.shape[0]
    on = device_run(BAR4, MERGE, coarse=True)
    assert_same_to_rounding(on, device_run(BAR4, 0, coarse=True), nV, "coarse term")


@pytest.mark.parametrize("shard_elems", ["0", "owner"])
def test_all_wide_on_two_ranks_reproduces_the_narrow_single_gpu_run(shard_elems):
    """two ranks on one GPU (tests/test_gpu_two_ranks.py's harness and its assertions) with every wide form forced on the ranks only,
    summed by all-reduce and by the owner exchange -- against the single-GPU run on the narrow forms"""
    from tests.test_gpu_two_ranks import _ranks_reproduce_the_single_gpu_run as harness
    forms = _with_env({"DOTMI_WIDE_FORMS": "0"}, lambda: harness(BAR4, 2, shard_elems, 2, rank_env={"DOTMI_WIDE_FORMS": "7"}))
    assert len(forms) == 2 and all(f & 7 == 7 for f in forms), forms


# ---- (d) just past two thresholds, by size ----------------------------------------------------------------------------------------------------
def test_bar_just_past_the_merge_and_direction_thresholds_by_size():
    """synbar:180x15x15:64, 46 336 vertices: by default the 512-thread merge takes a full trip of 131 072 dofs and 7 936 more, the
    1024-thread direction kernel 32 768 rows and 13 568 more, the gather stays narrow.  One step against the narrow forms (no oracle:
    at this size it is the slow side, and the forced forms above are tied to it)"""
    name = "synbar:180x15x15:64"
    nV = load_workload(name)[0].V_rest.shape[0]
    assert nV == 46336
    wide = device_run(name, None, steps=1)
    assert wide[3] & 7 == MERGE | SPMV, wide[3]
    assert_same_to_rounding(wide, device_run(name, 0, steps=1), nV, name)
