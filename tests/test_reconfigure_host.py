"""Host side of the setters of a live handle (dotmi_set_rel_tol, dotmi_set_time_step, dotmi_set_lame): the rule that picks a time
step's tolerance from a script's `tol` list, and the C++ adapter's members that forward to them.  The device side is
tests/test_gpu_reconfigure.py."""
import os
import subprocess

from dot_amd.timestepper import tol_for_step
from tests.test_abi import _has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tolerance_of_step_k():
    """src/main.cpp:108-118: entry k of the list, its last entry beyond the end, the stepper's own value without a list"""
    assert tol_for_step([], 0, 1e-5) == 1e-5 and tol_for_step(None, 7, 2e-4) == 2e-4
    assert [tol_for_step([1e-3], k, 1e-5) for k in range(3)] == [1e-3, 1e-3, 1e-3]
    assert [tol_for_step([1e-4, 1e-5], k, 1.0) for k in range(4)] == [1e-4, 1e-5, 1e-5, 1e-5]
    long = [10.0 ** -k for k in range(1, 9)]
    assert [tol_for_step(long, k, 1.0) for k in range(8)] == long and tol_for_step(long, 100, 1.0) == long[-1]


def test_cpp_adapter_setters_build_link_and_fail_loudly_or_step(tmp_path):
    """dot_amd/host/adapter_reconfig_check.cpp (plain g++, -Wall -Werror, no HIP headers) against libdotmi.so: on a GPU box it
    changes tolerance, time step and materials between steps of the built stepper; without one precompute() reports the ABI's
    no-CPU-fallback error (exit 3) after setLameParam before precompute() has thrown its logic_error"""
    exe = tmp_path / "adapter_reconfig_check"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "dot_amd", "host", "adapter_reconfig_check.cpp"),
                           "-o", str(exe), "-L" + os.path.join(ROOT, "dot_amd"), "-ldotmi",
                           "-Wl,-rpath," + os.path.join(ROOT, "dot_amd")])
    rc = subprocess.call([str(exe)])
    assert rc == (0 if _has_gpu() else 3)
