"""The scenario of tests/test_gpu_no_pair.py, pinned on the CPU: from the state of tests/buckled_bar.py the oracle's step, capped at 48
iterations, accepts six trials in a row whose pair it does not store (y . s < 0, iterations 30 to 35, the window of five pairs
full), and the numpy restatement (tests/dot_coarse_reference.DotStepper, with hist= and iter_cap=) does the same at history 5 and
at the iterations listed below at other history lengths and with the rigid-mode coarse term.  If a change of the oracle, the mesh
generator or the partition moved these events, the GPU module would compare two sides that no longer meet the no-pair path: this
module fails first.

An event: an accepted trial after which the newest stored s is not x_{k+1} - x_k; iterations count from 1 (iteration k + 1 goes
from x_k to x_{k+1}).  No device is touched."""
import numpy as np
import pytest

from tests import buckled_bar as B

EVENTS = [30, 31, 32, 33, 34, 35]
# history length -> iterations that store no pair, still capped at 48
EVENTS_AT = {1: [34], 2: [29, 30, 31, 32, 33, 34], 4: [30, 31, 32, 33], 6: [30, 31, 32, 33]}
EVENTS_COARSE = [27, 28, 29, 30]


def test_state_function_reproduces_the_fixture():
    """start_state() against the committed positions: the fixed vertices and the compression bit for bit always, the noise too wherever
    numpy's default_rng(4) still starts with the deviate it started with when the fixture was written"""
    sc, ep, n, x = B.load()
    fixed = np.asarray(sc.fixed, dtype=bool)
    assert (x.shape[0], sc.T.shape[0], int(fixed.sum()), n) == (117, 288, 18, 4)
    assert np.bincount(ep).tolist() == [72, 72, 72, 72]
    got = B.start_state(sc.x0, sc.fixed)
    assert np.array_equal(got[fixed], x[fixed])
    ax = int(np.argmax(np.ptp(np.asarray(sc.x0), axis=0)))
    other = [d for d in range(3) if d != ax]
    assert np.ptp(x[fixed][:, ax]) <= B.SCALE * np.ptp(np.asarray(sc.x0)[:, ax])
    assert np.abs(x[:, other] - np.asarray(sc.x0)[:, other]).max() < 6 * B.NOISE          # (only noise across the axis)
    same_stream = float(np.random.default_rng(B.SEED).standard_normal()) == B.FIRST_DEVIATE
    print("generator stream as recorded:", same_stream, " max|start_state - fixture|", float(np.abs(got - x).max()))
    if same_stream:
        assert np.array_equal(got, x)


def test_oracle_accepts_six_trials_without_storing_their_pair():
    R = B.oracle_run()
    assert R["iters"] == B.ITER_CAP
    ys, cos = [], []
    for k in range(B.ITER_CAP):
        s, y = R["xs"][k + 1] - R["xs"][k], R["gs"][k + 1] - R["gs"][k]
        ys.append(float(np.vdot(s, y)))
        cos.append(B.cosine(s, y))
    events = [k + 1 for k in range(B.ITER_CAP) if not ys[k] > 0.0]
    print("oracle:", R["iters"], "iterations,", R["halvings"], "halvings; y.s <= 0 at", events, "cosines",
          [f"{cos[k - 1]:.4f}" for k in events], "pairs stored in front of the first:", R["m"][events[0] - 1] if events else None)
    assert events == EVENTS
    assert all(cos[k - 1] <= -5e-3 for k in EVENTS)
    assert [k + 1 for k in range(B.ITER_CAP) if not R["stored"][k]] == EVENTS     # (the definition: nothing stored there, a pair everywhere else)
    assert R["m"][EVENTS[0] - 1] == 5                                            # the window is full at the first of them
    assert all(R["m"][k] == 5 for k in range(EVENTS[0] - 1, B.ITER_CAP))          # ... and later pairs drop the oldest
    assert R["halvings"] == 3
    alpha = R["log"][0]
    assert np.count_nonzero(alpha < 1.0) > B.ITER_CAP // 2                        # most step estimates lie below 1


def test_restatement_at_history_5_is_the_oracles_step():
    R, r = B.oracle_run(), B.restated_run(5)
    err = float(np.abs(r["x"] - R["x"]).max())
    print(f"restatement: {r['iters']} iterations, {r['halvings']} halvings, status {r['status']}, no pair at {r['no_pair']}; "
          f"positions against the oracle {err:.2e}")
    assert (r["iters"], r["halvings"], r["status"]) == (R["iters"], R["halvings"], 2)
    assert r["no_pair"] == EVENTS
    assert err < 1e-10
    B.compare_logs(r["log"], R["log"], "restatement against the oracle")


@pytest.mark.parametrize("hist", sorted(EVENTS_AT))
def test_restatement_meets_the_path_at_other_history_lengths(hist):
    r = B.restated_run(hist)
    print(f"history {hist}: {r['iters']} iterations, {r['halvings']} halvings, no pair at {r['no_pair']}")
    assert (r["iters"], r["status"]) == (B.ITER_CAP, 2)
    assert r["no_pair"] == EVENTS_AT[hist]


def test_restatement_meets_the_path_with_the_coarse_term():
    r = B.restated_run(5, coarse=True)
    print(f"coarse term: {r['iters']} iterations, {r['halvings']} halvings, no pair at {r['no_pair']}")
    assert r["active"]
    assert (r["iters"], r["status"]) == (B.ITER_CAP, 2)
    assert r["no_pair"] == EVENTS_COARSE


def test_default_parameters_of_the_restatement_are_unchanged():
    """hist and iter_cap default to the module's constants: every earlier use of DotStepper.step is what it was"""
    import inspect
    from tests import dot_coarse_reference as DR
    p = inspect.signature(DR.DotStepper.step).parameters
    assert (p["hist"].default, p["iter_cap"].default) == (DR.HIST, DR.ITER_CAP) == (5, 10000)
