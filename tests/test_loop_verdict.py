"""The loop controller's decision on a slot (dot_amd/csrc/loop_verdict.hpp, run by thread 0 of k_loopctl.hpp's controller), checked on the CPU.

`make -C dot_amd/csrc loopctl_check` builds loopctl_check.cpp with the host compiler under the address and UB sanitizers and runs it:
418 seeded scripts of a time step's trials, each walked by a sequential statement of the reference's loop and driven slot by slot
through loop_verdict<CTL> in its five forms (the paired ones with cold and with saturated pairing counters).  After every accepted
trial the energy, |g|^2, the log and the L-BFGS scalars, and at the end the counters and the status, equal the sequential model's bit
for bit; every slot publishes one verdict, holdVerdict = 2 slots + stop; the stop verdicts number what fill_step_stats reports (one
less in a collapsed step); the iterate and gradient pointers swap once per accept; the controller's chunk sums add up to chunked_sum.
The program counts the classes of case its scripts are meant to hold (every band of alpha_0, one to four rejections, redone and
rejected paired slots, redone speculative slots, y.s <= 0, every history length, the cap inside a halving iteration, convergence at
the first iteration, a collapsed step) and fails if one stayed empty.  A program that does not build fails the test like one that
finds a difference.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_controller_decision_is_bit_identical_to_the_sequential_line_search():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dot_amd", "csrc"), "loopctl_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "418 scripts x 7 drives" in r.stdout, r.stdout
    assert "every drive equal to the sequential model" in r.stdout, r.stdout
