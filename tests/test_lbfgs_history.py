"""The L-BFGS history update that the host loop and the device controller share (dot_amd/csrc/lbfgs_history.hpp), checked on the CPU.

`make -C dot_amd/csrc history_check` builds history_check.cpp with the host compiler under the address and UB sanitizers and runs
it: for every history length 1 .. HIST_MAX, 200 random sequences of 40 accepted trials (one in five with y.s <= 0), and after every
update m, order / ys / b / sy over [0, m), xi and the free slot equal, bit for bit, to the plain indexed statement the host loop
used to run.  A program that does not build fails the test like one that finds a difference.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_history_update_is_bit_identical_to_the_plain_statement():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dot_amd", "csrc"), "history_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "48000 updates" in r.stdout, r.stdout
