"""Which form -- narrow (256 threads) or wide (512 / 512 / 1024) -- the vertex gather, the early merge and the direction kernel of the
L-BFGS iteration take (dot_amd/csrc/loop_forms.hpp, the one statement the launchers, dotmi_loop_forms and dotmi_plan_loop_forms share),
through the host-only entry dotmi_plan_loop_forms: the thresholds, the force mask DOTMI_WIDE_FORMS, and the forms the named workloads
get.  No GPU.  The forms themselves against the oracle and against each other: tests/test_gpu_wide_forms.py."""
import ctypes as C

import pytest

from dot_amd import lib as dl
from dot_amd.workloads import WORKLOADS, load_workload

GATHER, MERGE, SPMV = 1, 2, 4
# one trip of the 256 workgroups, in what the launch counts (scalar dofs, scalar dofs, block rows): the wide form beyond ...
GATHER_DOFS = 2 * 4 * 256 * 256      # ... two trips of 256 threads x 4 dofs
MERGE_DOFS = 2 * 256 * 256           # ... two trips of 256 threads x 1 dof
SPMV_ROWS = 256 * 32 * 3             # ... one trip of 32 lane groups x 3 rows


def plan(ndof_gather, ndof_merge, nrows_spmv, force=-1):
    out = C.c_int32(-1)
    assert dl.load().dotmi_plan_loop_forms(ndof_gather, ndof_merge, nrows_spmv, force, C.byref(out)) == 0
    return out.value


def forms_of_mesh(nV, force=-1):
    return plan(3 * nV, 3 * nV, nV, force)


def test_thresholds_are_the_documented_numbers():
    assert (GATHER_DOFS, MERGE_DOFS, SPMV_ROWS) == (524288, 131072, 24576)


@pytest.mark.parametrize("bit,at", [(GATHER, GATHER_DOFS), (MERGE, MERGE_DOFS), (SPMV, SPMV_ROWS)])
def test_each_rule_flips_exactly_between_n_and_n_plus_1(bit, at):
    def one(n):   # (the other two counts at zero: their bits stay clear)
        return plan(n if bit == GATHER else 0, n if bit == MERGE else 0, n if bit == SPMV else 0)
    assert one(at) == 0 and one(at + 1) == bit
    assert one(0) == 0 and one(1) == 0 and one(at - 1) == 0
    assert one(2 * at) == bit and one(2 ** 40) == bit      # (counts are 64-bit: no wrap far beyond 2^31)


def test_the_rules_are_independent_of_each_other():
    for g in (GATHER_DOFS, GATHER_DOFS + 1):
        for m in (MERGE_DOFS, MERGE_DOFS + 1):
            for s in (SPMV_ROWS, SPMV_ROWS + 1):
                want = (GATHER if g > GATHER_DOFS else 0) | (MERGE if m > MERGE_DOFS else 0) | (SPMV if s > SPMV_ROWS else 0)
                assert plan(g, m, s) == want


@pytest.mark.parametrize("mask", range(8))
def test_every_mask_overrides_the_size_in_both_directions(mask):
    tiny, huge = (1, 1, 1), (GATHER_DOFS * 8, MERGE_DOFS * 8, SPMV_ROWS * 8)
    assert plan(*tiny) == 0 and plan(*huge) == 7
    assert plan(*tiny, force=mask) == mask
    assert plan(*huge, force=mask) == mask
    assert plan(GATHER_DOFS, MERGE_DOFS, SPMV_ROWS, force=mask) == mask
    assert plan(GATHER_DOFS + 1, MERGE_DOFS + 1, SPMV_ROWS + 1, force=mask) == mask


def test_minus_one_is_the_size_rule():
    for nV in (1, 4670, 24576, 24577, 43690, 43691, 46336, 174762, 174763, 182736, 10 ** 7):
        assert forms_of_mesh(nV, -1) == forms_of_mesh(nV)
        want = (GATHER if 3 * nV > GATHER_DOFS else 0) | (MERGE if 3 * nV > MERGE_DOFS else 0) | (SPMV if nV > SPMV_ROWS else 0)
        assert forms_of_mesh(nV) == want


def test_smallest_meshes_that_select_each_wide_form():
    """the table of the thresholds in vertices: 174 763, 43 691 and 24 577"""
    assert forms_of_mesh(174763) & GATHER and not forms_of_mesh(174762) & GATHER
    assert forms_of_mesh(43691) & MERGE and not forms_of_mesh(43690) & MERGE
    assert forms_of_mesh(24577) & SPMV and not forms_of_mesh(24576) & SPMV


def test_invalid_arguments():
    L = dl.load()
    assert L.dotmi_plan_loop_forms(1, 1, 1, -1, None) == -1
    out = C.c_int32()
    assert L.dotmi_plan_loop_forms(-1, 1, 1, -1, C.byref(out)) == -1


@pytest.mark.parametrize("name", sorted(WORKLOADS))
def test_named_workloads_stay_on_the_narrow_forms(name):
    """every named workload is below all three thresholds (the largest, monkey18K: 18 388 vertices): what the kernel-by-kernel oracle
    tests step never reaches a wide form by size"""
    nV = load_workload(name)[0].V_rest.shape[0]
    assert nV <= 18388
    assert forms_of_mesh(nV) == 0


def test_refined_horse_takes_the_wide_merge_and_direction_kernel():
    sc = load_workload("horse7K_stretch@r1:64")[0]
    nV = sc.V_rest.shape[0]
    assert sc.T.shape[0] == 248736 and 43691 <= nV < 174763
    assert forms_of_mesh(nV) == MERGE | SPMV


def test_the_1M_tet_bar_takes_all_three_wide_forms():
    sc = load_workload("synbar:140x35x35:256")[0]
    nV = sc.V_rest.shape[0]
    assert nV == 141 * 36 * 36 and 3 * nV == 548208
    assert forms_of_mesh(nV) == GATHER | MERGE | SPMV


def test_the_bar_just_past_two_thresholds():
    """tests/test_gpu_wide_forms.py's mesh chosen by size: 139 008 dofs -- the 512-thread merge takes one full trip (131 072 dofs) and
    7 936 more, the 1024-thread direction kernel 32 768 rows and then 13 568"""
    nV = 181 * 16 * 16
    assert nV == 46336 and 3 * nV - 256 * 512 == 7936 and nV - 256 * 128 == 13568
    assert forms_of_mesh(nV) == MERGE | SPMV


def test_the_small_meshes_of_the_gpu_tests_have_the_edges_they_are_chosen_for():
    """tests/test_gpu_wide_forms.py forces the wide forms on bunny5K -- 27 full 512-thread workgroups, a partial one and 228 with nothing
    to do -- and on a bar of less than one workgroup"""
    assert 3 * load_workload("bunny5K_LTSS")[0].V_rest.shape[0] == 14010 and divmod(14010, 512) == (27, 186)
    assert 3 * load_workload("synbar:8x3x3:4")[0].V_rest.shape[0] == 432
