"""The sum behind every merge of the block solve (dot_amd/csrc/merge_sum.hpp), checked on the CPU.

`make -C dot_amd/csrc merge_check` builds merge_check.cpp with the host compiler under the address and UB sanitizers and runs it: on
20 sets of merge lists that build_merge_lists (block_plan.hpp) makes from synthetic subdomains -- a vertex in three and in four
subdomains, lists longer than a batch of MT_CH entries with a subdomain boundary on a batch's first entry, one-entry lists, waves of
unequal lists, 3 nV no multiple of 64; the program asserts that each is there -- the CSR walk, the wave-interleaved walk and the gather
from the subdomains' own sums (one and three components) equal, bit for bit, the plain two-stage statement: the tiles of a subdomain
in tile order from 0.0, then the subdomains in vp order.  A program that does not build fails the test like one that finds a difference.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_forms_are_bit_identical_to_the_plain_two_stage_sum():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "dot_amd", "csrc"), "merge_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "36000 sums over 20 sets of lists" in r.stdout, r.stdout
