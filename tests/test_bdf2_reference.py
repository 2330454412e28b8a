"""BDF2 beside backward Euler on the CPU: the library's host-only rule (dotmi_plan_time_integration, dot_amd/csrc/time_integration.hpp),
its exports, and the restatement of BDF2 through the unchanged oracle (tests/bdf2_reference.py) on the bar of the accuracy study --
synthetic_bar(8, 2, 2), fixed at x = 0, gravity, Stable Neo-Hookean, YM 2e4, PR 0.4, rho 1, two subdomains, rel_tol 1e-9, T = 0.48.

The bounds of the accuracy tests are the issue's: the reference solution is BDF2 at 1536 steps; BDF2's error at 48, 96 and 192 steps is
at most a fifth of backward Euler's at the same dt; halving dt shrinks BDF2's error by at least 2.5 and backward Euler's by at most 2.2
(gravity switched on at t = 0 excites modes dt does not resolve, so BDF2's ratio is 3, not 4); the two variable-step runs land between
the uniform 96-step and 192-step errors."""
import ctypes as C
import subprocess
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from tests import bdf2_reference as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["dotmi_set_time_integration", "dotmi_time_integration", "dotmi_time_integration_info", "dotmi_get_history",
               "dotmi_set_history", "dotmi_plan_time_integration"]


def plan(kind, dt, dt_prev, levels):
    L = dl.load()
    out = [C.c_double() for _ in range(4)]
    rc = L.dotmi_plan_time_integration(kind, dt, dt_prev, levels, *[C.cast(C.byref(o), dl.c_dp) for o in out])
    return rc, tuple(o.value for o in out)


# ---- the host entry and the exports (both fail on a library from before BDF2) ------------------------------------------------------
@pytest.mark.parametrize("w", [1.0, 0.5, 3.0])
def test_plan_entry_gives_the_bdf2_coefficients(w):
    dt_prev = 0.0125
    dt = w * dt_prev
    rc, (c0, c1, gamma, dte) = plan(dl.TIT_BDF2, dt, dt_prev, 1)
    assert rc == 0
    e0, e1, eg = B.closed_form(w)
    # c0 in [1, 4): its own rounding and the quotient's; c1 = c0 - 1 inherits them as an absolute error
    assert abs(c0 - e0) <= 9e-16 and abs(c1 - e1) <= 9e-16 and abs(gamma - eg) <= 4e-16 * eg
    assert c0 - c1 == 1.0
    assert dte == gamma * dt
    # the restatement's coefficients are the header's, operation by operation
    assert (c0, c1, gamma, dte) == B.coefficients(dt, dt_prev, 1)
    if w == 1.0:
        assert np.allclose([gamma, c0, c1], [2 / 3, 4 / 3, 1 / 3], rtol=3e-16, atol=0)


def test_plan_entry_backward_euler_is_one_zero_one():
    for kind, levels in ((dl.TIT_BE, 0), (dl.TIT_BE, 1), (dl.TIT_BDF2, 0)):
        rc, out = plan(kind, 0.025, 0.01, levels)
        assert rc == 0 and out == (1.0, 0.0, 1.0, 0.025), (kind, levels, out)


def test_plan_entry_refuses_bad_arguments():
    L = dl.load()
    assert plan(2, 0.01, 0.01, 1)[0] == -1 and plan(-1, 0.01, 0.01, 0)[0] == -1
    assert plan(dl.TIT_BDF2, 0.0, 0.01, 1)[0] == -1 and plan(dl.TIT_BDF2, float("nan"), 0.01, 1)[0] == -1
    assert plan(dl.TIT_BDF2, 0.01, 0.0, 1)[0] == -1 and plan(dl.TIT_BDF2, 0.01, -1.0, 1)[0] == -1
    assert plan(dl.TIT_BDF2, 0.01, 0.01, 2)[0] == -1
    assert L.dotmi_plan_time_integration(dl.TIT_BDF2, 0.01, 0.01, 1, None, None, None, None) == 0   # (any output may be NULL)


def test_library_exports_the_time_integration_entries():
    out = subprocess.check_output(["nm", "-D", "--defined-only", dl.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW_EXPORTS:
        assert name in exported, name
        assert name in dl.EXPORTS
    header = open(os.path.join(ROOT, "include", "dotmi.h")).read()
    assert "DOTMI_TIT_BE = 0" in header and "DOTMI_TIT_BDF2 = 1" in header
    for cite in ("Optimizer.cpp:354-361", ":588-610", ":1188", ":1225"):
        assert cite in header, cite


def test_entries_refuse_a_null_handle():
    L = dl.load()
    assert L.dotmi_set_time_integration(None, dl.TIT_BDF2) == -1
    assert L.dotmi_time_integration(None) == -1
    assert L.dotmi_time_integration_info(None, None, None, None, None) == -1
    assert L.dotmi_get_history(None, None, None, None) == -1
    assert L.dotmi_set_history(None, None, None, 0.01) == -1


def test_tit_check_passes_under_the_host_sanitizers():
    """make tit_check: the header against its plain statement, c0 - c1 == 1, (1, 0, 1), quadratics exact -- a stand-alone program"""
    out = subprocess.check_output(["make", "-s", "-C", os.path.join(ROOT, "dot_amd", "csrc"), "tit_check"], stderr=subprocess.STDOUT)
    assert b"equal to the plain statement" in out, out


# ---- the restatement on the bar -----------------------------------------------------------------------------------------------------
def err(x, ref):
    return float(np.abs(x - ref).max())


@pytest.fixture(scope="module")
def fine():
    """BDF2 at 1536 steps: the reference solution of every accuracy test below (computed once, never written to)"""
    x = B.run_bar([B.BAR_T / B.FINE_STEPS] * B.FINE_STEPS)
    x.setflags(write=False)
    return x


def test_recorded_fine_solution_is_the_fresh_one(fine):
    """tests/golden/bdf2_bar_fine.npz (what tests/test_gpu_bdf2.py measures the device's errors against) against the run above: both are
    converged to rel_tol 1e-9 per step, far below the 2e-4 .. 2e-2 errors that are measured against them"""
    assert B.FINE_STEPS == 1536
    assert err(B.load_golden(), fine) <= 1e-8


@pytest.fixture(scope="module")
def uniform(fine):
    """errors of backward Euler and BDF2 at 48, 96 and 192 steps"""
    e = {}
    for n in (48, 96, 192):
        e["be", n] = err(B.run_bar([B.BAR_T / n] * n, bdf2=False), fine)
        e["bdf2", n] = err(B.run_bar([B.BAR_T / n] * n), fine)
        print(f"{n} steps: backward Euler {e['be', n]:.3e}  BDF2 {e['bdf2', n]:.3e}")
    return e


def test_velocity_formulas_agree():
    """(x+ - x^) / dt_e is the BDF2 difference (3 x+ - 4 x_n + x_{n-1}) / (2 dt) at constant dt"""
    n = 48
    dt = B.BAR_T / n
    V = B.bar()[0]
    states = [(V, np.zeros_like(V))] + B.run_bar([dt] * 12, keep=True)
    worst = 0.0
    for k in range(2, len(states)):   # (step 1 is the backward-Euler start step)
        classic = (3 * states[k][0] - 4 * states[k - 1][0] + states[k - 2][0]) / (2 * dt)
        worst = max(worst, err(states[k][1], classic))
    print(f"velocity formulas: max difference {worst:.2e}")
    assert worst <= 1e-11


def test_bdf2_is_more_accurate_than_backward_euler(uniform):
    for n in (48, 96, 192):
        assert uniform["bdf2", n] <= uniform["be", n] / 5, (n, uniform["bdf2", n], uniform["be", n])


def test_convergence_orders(uniform):
    for a, b in ((48, 96), (96, 192)):
        r2, r1 = uniform["bdf2", a] / uniform["bdf2", b], uniform["be", a] / uniform["be", b]
        print(f"{a} -> {b} steps: BDF2 error shrinks by {r2:.2f}, backward Euler's by {r1:.2f}")
        assert r2 >= 2.5, (a, b, r2)
        assert r1 <= 2.2, (a, b, r1)


def test_variable_step_runs_land_between_the_uniform_ones(uniform, fine):
    T = B.BAR_T
    runs = {"48 x T/96 then 96 x T/192": [T / 96] * 48 + [T / 192] * 96,
            "T/288 and T/96 alternating": [T / 288, T / 96] * 72}
    for name, dts in runs.items():
        assert abs(sum(dts) - T) < 1e-12
        e = err(B.run_bar(dts), fine)
        print(f"{name}: {e:.3e} (uniform 96: {uniform['bdf2', 96]:.3e}, 192: {uniform['bdf2', 192]:.3e})")
        assert uniform["bdf2", 192] <= e <= uniform["bdf2", 96], (name, e)
