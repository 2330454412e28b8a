"""The loop's no-pair path on the device: an accepted trial with y . s <= 0 stores no L-BFGS pair -- the controller sets
DevLoop::pairNew = 0 (dot_amd/csrc/k_loopctl.hpp, lbfgs_history.hpp), merge_tiles_early_kernel (k_loopvec.hip) then takes every
stored pair's cached M y_j, moves u_old on, leaves my_new alone and, in the owner exchange's `pre` branch, takes xi_new = 0; the
operand records keep their free slot; the cached H s_j and M y_j go on following order[] when later pairs drop the oldest.  No scripted
workload of the suite ever produces a non-positive y . s; the state of tests/buckled_bar.py does, six times in a row at iterations 30
to 35 of one step capped at 48 (tests/test_no_pair_reference.py pins that on the CPU).  Every case here is that one capped step on a
fresh handle created at the rest state that gets dotmi_set_state(x, 0, x) and no refactor.

  (a) every form of the loop against the oracle: status 2, iterations, halvings, the per-iteration log, the positions;
  (b) the device's own curvature: the iterates x_29 .. x_36 (steps capped there) and their gradients from dotmi_eval_gradient --
      y_k . s_k is negative exactly where the oracle's is, so the device met the condition itself;
  (c) the device loop against the host loop bit for bit in the q-based order, at history 1, 2, 4, 5, 6, and both against the numpy
      restatement with that history;
  (d) the COARSE instantiation: dotmi_set_dot_coarse against the restatement with M';
  (e) two ranks on one GPU, summed by all-reduce (replicated and sharded element pass) and by the owner exchange.

Every run first asserts, wherever the handle can say so, that the form it means to run is in effect: a switch that is silently
ignored fails here.  The switches are read by dotmi_create: set around the constructor and restored.

Bounds.  Positions within 1e-9 of the oracle's, the suite's bound for steps against it (tests/test_gpu_round3.py,
tests/test_gpu_wide_forms.py): the oracle amplifies a 1e-13 perturbation of the start state about 230 times over the 48 iterations
(linear: the same factor at 1e-14 and 1e-12) and the restatement, which differs from it in summation order only, ends 3.4e-13 away,
so the bound leaves three orders of magnitude over both.  The log: step lengths equal where the reference's is 1, the clamp 0.1 or
one of them halved, estimates within 1e-9 relative, E within 1e-9, |g|^2 within 1e-6 (tests/test_gpu_round2.py's teacher-forced
steps; tests/buckled_bar.compare_logs).  Every test prints its measured maxima."""
import os
import sys
import tempfile

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper
from tests import buckled_bar as B
from tests.test_no_pair_reference import EVENTS, EVENTS_AT, EVENTS_COARSE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDE, SPLIT = 7, 8
SWITCHES = ("DOTMI_OPERAND_RECORDS", "DOTMI_VERTEX_PATCHES", "DOTMI_EARLY_BACKSOLVE", "DOTMI_FUSE_DIR", "DOTMI_FUSE_STEP", "DOTMI_EARLY_HOLD",
            "DOTMI_PAIR_TRIALS", "DOTMI_SPEC_STEP", "DOTMI_WIDE_FORMS", "DOTMI_SPLIT_MERGE", "DOTMI_SHARD_ELEMS", "DOTMI_SHARD_HESS")

# form -> (switches, flags, what the handle must say: operand records (dotmi_operand_records: 1 records, 0 flat arrays, -1 no vertex
# patches on this handle), loopForms() & 15, the early order (backsolve_stopped == halvings + 1 + redone slots; 0 in the q-based order and
# in the host loop), and which of paired / speculating slots there must be).
# Paired trials keep the element patches unless the vertex patches are forced (choose_step_forms): the row "with vertex patches" forces them;
# both paired rows train the pairing rule first (train_pairing), so that a slot does pair and the handle can say so.
# The speculative unit step under choose_step_forms' preconditions: one rank, early order, both fused kernels, no pairing, no coarse term.
FORMS = {
    "default": ({}, 0, dict(orec=1, forms=0, early=True)),
    "flat operands": ({"DOTMI_OPERAND_RECORDS": "0"}, 0, dict(orec=0, forms=0, early=True)),
    "element patches": ({"DOTMI_VERTEX_PATCHES": "0"}, 0, dict(orec=-1, forms=0, early=True)),
    "q-based order": ({"DOTMI_EARLY_BACKSOLVE": "0"}, 0, dict(orec=-1, forms=0, early=False)),
    "unfused direction": ({"DOTMI_FUSE_DIR": "0"}, 0, dict(orec=-1, forms=0, early=True)),
    "unfused step": ({"DOTMI_FUSE_STEP": "0"}, 0, dict(orec=-1, forms=0, early=True)),
    "no holds": ({"DOTMI_EARLY_HOLD": "0"}, 0, dict(orec=1, forms=0, early=True, held=0)),
    "paired, vertex patches": ({"DOTMI_PAIR_TRIALS": "1", "DOTMI_VERTEX_PATCHES": "1"}, 0, dict(orec=1, forms=0, early=True, paired=True)),
    "paired, element patches": ({"DOTMI_PAIR_TRIALS": "1", "DOTMI_VERTEX_PATCHES": "0"}, 0, dict(orec=-1, forms=0, early=True, paired=True)),
    "speculative unit step": ({"DOTMI_SPEC_STEP": "1", "DOTMI_PAIR_TRIALS": "0"}, 0, dict(orec=1, forms=0, early=True, spec=True)),
    "all wide": ({"DOTMI_WIDE_FORMS": "7"}, 0, dict(orec=1, forms=WIDE, early=True)),
    "split merge": ({"DOTMI_SPLIT_MERGE": "1"}, 0, dict(orec=1, forms=SPLIT, early=True)),
    "wide and split": ({"DOTMI_WIDE_FORMS": "7", "DOTMI_SPLIT_MERGE": "1"}, 0, dict(orec=1, forms=WIDE | SPLIT, early=True)),
    "host loop": ({}, dl.FLAG_HOST_LOOP, dict(orec=-1, forms=0, early=False)),
    "one rank sharded": ({}, dl.FLAG_FORCE_DIST, dict(orec=-1, forms=0, early=True, dist=True)),
}


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def assert_form(form, want, ts, st, forms):
    """what the handle and the step's statistics say about the form that ran"""
    assert dl.load().dotmi_operand_records(ts._h) == want["orec"], (form, "operand records")
    assert forms & 15 == want["forms"], (form, "loopForms", forms)
    assert (st.paired_slots > 0) == bool(want.get("paired")), (form, "paired slots", st.paired_slots)
    assert (st.spec_slots > 0) == bool(want.get("spec")), (form, "speculating slots", st.spec_slots)
    if want["early"] and not want.get("paired"):    # (a paired step pairs only in the early order: its slots say it)
        assert st.backsolve_stopped == st.ls_halvings + 1 + st.spec_redone, (form, "early order", st.backsolve_stopped)
    elif not want["early"]:
        assert st.backsolve_stopped == 0 and st.backsolve_held == 0, (form, "q-based order", st.backsolve_stopped)
    if "held" in want:
        assert st.backsolve_held == want["held"], (form, "held launches", st.backsolve_held)
    assert (st.collective_calls > 0) == bool(want.get("dist")), (form, "collectives", st.collective_calls)


def train_pairing(ts, sc):
    """A paired step pairs a first trial only in a band of step estimates whose first trials have mostly been rejected
    (DevLoop::pairCtr, carried from step to step; k_loopctl.hpp), and this state's step rejects one first trial in 48: untrained, it would
    run the paired launches and controllers without a single paired slot and the handle could not say that it pairs.  Three steps of
    one iteration each (the tolerance raised out of reach) from the rest state with 0.05 x Gaussian noise, where the oracle's first trial
    at alpha_0 = 0.96 .. 0.98 is rejected, fill the counter of the band [0.9, 1); the capped step's first estimate, 0.932, lies in it.
    Afterwards the tolerance and the rest state's factors are put back."""
    tol, rel = ts.targetGRes, ts.rel_tol
    x0 = np.asarray(sc.x0, dtype=np.float64)
    free = ~np.asarray(sc.fixed, dtype=bool)
    ts.setRelGL2Tol(1e3)
    for seed in range(3):
        x = x0.copy()
        x[free] += 0.05 * np.random.default_rng(seed).standard_normal((int(free.sum()), 3))
        ts.setState(x, np.zeros_like(x), x)
        st = ts.step()
        assert (st.status, st.iters) == (0, 1) and st.ls_halvings >= 1, (seed, st.status, st.iters, st.ls_halvings)
    ts.setRelGL2Tol(rel)
    assert ts.targetGRes == tol
    ts.updatePrecondMtrAndFactorize(x0)


_runs = {}


def device_run(form="default", hist=5, iter_cap=B.ITER_CAP, coarse=False, grad=False):
    """the capped step from the fixture on a fresh handle in `form`; asserts what the handle says it runs.  A run is a function of its
    arguments: tests that need the same one share it.  -> dict(status, iters, halvings, evals, E, x, log; g: the device's gradient at
    x for the step's own x~ (grad))"""
    key = (form, hist, iter_cap, coarse, grad)
    if key in _runs:
        return _runs[key]
    env, flags, want = FORMS[form]
    preset = [k for k in SWITCHES if k in os.environ]
    assert not preset, preset
    sc, ep, n, x0 = B.load()
    ts = _with_env(env, lambda: DOTTimeStepper(sc, ep, n, history=hist, iter_cap=iter_cap, flags=flags))
    try:
        zero = np.zeros_like(x0)
        if want.get("paired"):
            train_pairing(ts, sc)
        ts.setState(x0, zero, x0)                    # (no refactor: the factors stay those of the rest state)
        assert np.array_equal(ts.getResult(), x0)    # the fixed vertices' positions included
        if coarse:
            ts.setDotCoarse(1)
            assert ts.dotCoarseInfo()[1:3] == (0, 1)
        st = ts.step()
        assert_form(form, want, ts, st, ts.loopForms())
        if coarse:
            assert ts.dotCoarseInfo()[2] == 1
        r = dict(status=st.status, iters=st.iters, halvings=st.ls_halvings, evals=st.energy_evals, E=st.E, x=ts.getResult().copy(),
                 log=tuple(np.array(v).copy() for v in ts.iterLog()), held=st.backsolve_held, paired=st.paired_slots,
                 spec=(st.spec_slots, st.spec_redone))
        if grad:
            ts.setState(x0, zero, x0)                # x~ of the step again (the step's end moved x_n and v)
            r["g"] = ts.computeGradient(r["x"])
    finally:
        ts.close()
    _runs[key] = r
    return r


def assert_same_step(r, counts, log, x, tag, status=2):
    """the bounds of the module's text against a reference run's (iterations, halvings), log and positions; -> the measured maxima"""
    dx = float(np.abs(r["x"] - x).max())
    print(f"{tag}: status {r['status']}, {r['iters']} iterations, {r['halvings']} halvings (reference {counts}); positions {dx:.2e}; "
          f"held {r['held']}, paired {r['paired']}, speculating / redone {r['spec']}")
    assert r["status"] == status, tag
    assert (r["iters"], r["halvings"]) == counts, tag
    d = B.compare_logs(r["log"], log, tag)
    assert dx < 1e-9, (tag, dx)
    return (dx,) + d


# ---- (a) every form against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_takes_the_oracles_capped_step(form):
    R = B.oracle_run()
    assert_same_step(device_run(form), (R["iters"], R["halvings"]), R["log"], R["x"], form)


# ---- (b) the device's own curvature ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "host loop"])
def test_the_device_itself_meets_negative_curvature_where_the_oracle_does(form):
    """x_k from steps capped at k = 29 .. 36, g_k = dotmi_eval_gradient(x_k) under the step's x~: every iterate within 1e-9 of the
    oracle's, and y_k . s_k < 0 with cosine <= -5e-3 exactly for k + 1 in 30 .. 35"""
    R = B.oracle_run()
    ks = list(range(29, 37))
    runs = {k: device_run(form, iter_cap=k, grad=True) for k in ks}
    worst = 0.0
    for k in ks:
        assert (runs[k]["status"], runs[k]["iters"]) == (2, k), k
        worst = max(worst, float(np.abs(runs[k]["x"] - R["xs"][k]).max()))
    cos = {}
    for k in ks[:-1]:
        s, y = runs[k + 1]["x"] - runs[k]["x"], runs[k + 1]["g"] - runs[k]["g"]
        cos[k + 1] = B.cosine(s, y)
    ocos = {k + 1: B.cosine(R["xs"][k + 1] - R["xs"][k], R["gs"][k + 1] - R["gs"][k]) for k in ks[:-1]}
    print(f"{form}: iterates 29 .. 36 within {worst:.2e} of the oracle's; cosines of (y, s) by iteration",
          {k: f"{c:.4f}" for k, c in cos.items()}, "oracle", {k: f"{c:.4f}" for k, c in ocos.items()})
    assert worst < 1e-9
    assert [k for k in cos if cos[k] < 0.0] == EVENTS
    assert all(cos[k] <= -5e-3 for k in EVENTS)
    assert all(cos[k] > 0.0 for k in cos if k not in EVENTS)


# ---- (c) device loop against host loop, bit for bit; both against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("hist", [1, 2, 4, 5, 6])
def test_device_and_host_loop_agree_bit_for_bit_at_every_history_length(hist):
    a, b = device_run("q-based order", hist=hist), device_run("host loop", hist=hist)
    r = B.restated_run(hist)
    assert r["no_pair"] == (EVENTS if hist == 5 else EVENTS_AT[hist])          # (the subject is there at this length)
    dx = float(np.abs(a["x"] - r["x"]).max())
    print(f"history {hist}: device {a['iters']} iterations, {a['halvings']} halvings, {a['evals']} energy evaluations, status {a['status']}; "
          f"restatement {r['iters']}, {r['halvings']}, no pair at {r['no_pair']}; positions against it {dx:.2e}")
    assert np.array_equal(a["x"], b["x"])
    assert (a["iters"], a["halvings"], a["evals"], a["status"]) == (b["iters"], b["halvings"], b["evals"], b["status"])
    assert (a["iters"], a["halvings"], a["status"]) == (r["iters"], r["halvings"], 2)
    assert dx < 1e-9


# ---- (d) the coarse term ---------------------------------------------------------------------------------------------------------------------
def test_coarse_term_takes_the_restatements_capped_step():
    """merge_tiles_early_kernel<., true>: dotmi_set_dot_coarse(1) after dotmi_set_state -- Z at the state's positions, A0 on the rest
    state's H, as the restatement's M' -- whose no-pair accepts are at iterations 27 to 30"""
    r = B.restated_run(5, coarse=True)
    assert r["active"] and r["no_pair"] == EVENTS_COARSE
    assert_same_step(device_run("default", coarse=True), (r["iters"], r["halvings"]), r["log"], r["x"], "coarse term")


# ---- (e) two ranks on one GPU ------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, initfile, outdir, shard_elems):
    """one rank of tests/test_gpu_two_ranks.py's kind: its own handle on device 0, the library's collectives through the host hook into
    a gloo all_reduce; the capped step from the fixture"""
    sys.path.insert(0, ROOT)
    owner = shard_elems == "owner"        # DOTMI_FLAG_OWNER_EXCHANGE: on the sharded element pass
    os.environ["DOTMI_SHARD_ELEMS"] = "1" if owner else shard_elems
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    calls = [0]

    def allreduce(a):
        calls[0] += 1
        dist.all_reduce(torch.from_numpy(a))

    sc, ep, n, x0 = B.load()
    ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world, allreduce=allreduce, iter_cap=B.ITER_CAP,
                        flags=dl.FLAG_OWNER_EXCHANGE if owner else 0)
    ts.setState(x0, np.zeros_like(x0), x0)
    calls[0] = 0
    st = ts.step()
    a, e, g2 = ts.iterLog()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), x=ts.getResult(), status=st.status, its=st.iters, halv=st.ls_halvings, E=st.E,
             alpha=a, Elog=e, g2log=g2, calls=calls[0], forms=ts.loopForms())
    ts.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("shard_elems", ["0", "1", "owner"])
def test_two_ranks_take_the_single_gpu_step(shard_elems):
    """the ranks bit-identical to each other in x, iterations, halvings and E; against the single-GPU default run the same iterations
    and halvings, positions within 1e-9.  The owner exchange runs the `pre` branch of the early merge (xi_new = pairNew ? . : 0) on
    the vertices both ranks hold"""
    import torch.multiprocessing as mp
    world = 2
    one = device_run("default")
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        initfile = os.path.join(d, "init")
        procs = [ctx.Process(target=_worker, args=(r, world, initfile, d, shard_elems)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive, "a rank hung (ranks branched apart?)"
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        R = [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(world)]
    for k in ("x", "status", "its", "halv", "E", "alpha", "Elog", "g2log", "calls"):
        assert np.array_equal(R[0][k], R[1][k]), k
    dx = float(np.abs(R[0]["x"] - one["x"]).max())
    print(f"two ranks, element pass {shard_elems}: status {int(R[0]['status'])}, {int(R[0]['its'])} iterations, {int(R[0]['halv'])} halvings, "
          f"{int(R[0]['calls'])} collectives; positions against one GPU {dx:.2e}")
    assert int(R[0]["calls"]) >= int(R[0]["its"])
    assert int(R[0]["status"]) == 2
    assert (int(R[0]["its"]), int(R[0]["halv"])) == (one["iters"], one["halvings"])
    assert dx < 1e-9
