"""Subdomain groups of the tile factorisation's level launches (dot_amd/csrc/tile_factor.hpp, DOTMI_TILE_GROUPS), on the CPU:
the assignment of subdomains to groups (longest processing time first) through dotmi_plan_tile_groups, and the grouped level
table -- every group a level schedule of its own, the groups' arrays one behind the other -- through
dotmi_plan_grouped_tile_schedule, held against the same table with one group."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl

WEIGHTS = [5, 5, 4, 3, 3, 2, 1, 1]
u8, i32, i64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def plan_groups(weights, G):
    L = C.CDLL(dl.LIB_PATH)
    f = L.dotmi_plan_tile_groups
    f.argtypes = [C.c_int32, i64, C.c_int32, i32]
    w = np.ascontiguousarray(weights, dtype=np.int64)
    g = np.full(len(w), -1, dtype=np.int32)
    used = f(len(w), w.ctypes.data_as(i64), G, g.ctypes.data_as(i32))
    return used, g


@pytest.mark.parametrize("G", [1, 2, 3, 8, 16])
def test_longest_processing_time_assignment(G):
    """every subdomain in exactly one group, no group empty, the heaviest group within the bound of the rule (mean + the largest
    single weight), 16 groups clamped to the 8 subdomains, and the same answer from a second call"""
    used, g = plan_groups(WEIGHTS, G)
    assert used == min(G, len(WEIGHTS))
    assert ((g >= 0) & (g < used)).all()                       # one group each (group_of has one entry per subdomain)
    load = np.bincount(g, weights=WEIGHTS, minlength=used)
    assert (np.bincount(g, minlength=used) > 0).all()
    assert load.sum() == sum(WEIGHTS)
    assert load.max() <= sum(WEIGHTS) / used + max(WEIGHTS)
    used2, g2 = plan_groups(WEIGHTS, G)
    assert used2 == used and np.array_equal(g, g2)


def test_equal_and_zero_weights_leave_no_group_empty():
    used, g = plan_groups([0, 0, 0, 0, 0], 3)
    assert used == 3 and (np.bincount(g, minlength=3) > 0).all()
    used, g = plan_groups([7, 7, 7, 7], 4)
    assert sorted(g.tolist()) == [0, 1, 2, 3]


def toy_blocks(seed=20240607):
    """five blocks of 3-6 tile columns in a shared layout of 6, random upper tile patterns"""
    rng = np.random.default_rng(seed)
    nt, cols = 6, [3, 6, 4, 5, 6]
    live = np.zeros((len(cols), nt), dtype=np.uint8)
    pat = np.zeros((len(cols), nt, nt), dtype=np.uint8)
    for b, c in enumerate(cols):
        live[b, :c] = 1
        for i in range(c):
            pat[b, i, i] = 1
            for j in range(i + 1, c):
                pat[b, i, j] = rng.random() < 0.5
    # a list ordered by block, like the dense fill's entries: a few entries per pattern tile
    fill_sub = np.concatenate([np.full(3 * int(pat[b].sum()), b, dtype=np.int32) for b in range(len(cols))])
    return nt, live, pat, fill_sub


def plan_grouped(nt, live, pat, fill_sub, G, eager_min=2, eager_chunk=1):
    L = C.CDLL(dl.LIB_PATH)
    f = L.dotmi_plan_grouped_tile_schedule
    f.argtypes = [C.c_int32, C.c_int32, u8, u8, C.c_int32, C.c_int32, C.c_int32, i64, i64, i32, i32, i64, i64, C.c_int32, i32, i32,
                  i32]
    nb = live.shape[0]
    live = np.ascontiguousarray(live, dtype=np.uint8)
    pat = np.ascontiguousarray(pat, dtype=np.uint8)
    fill_sub = np.ascontiguousarray(fill_sub, dtype=np.int32)
    nT, nC = C.c_int64(), C.c_int64()
    head = (nb, nt, live.ctypes.data_as(u8), pat.ctypes.data_as(u8), eager_min, eager_chunk, G)
    used = f(*head, None, C.byref(nT), None, None, None, C.byref(nC), len(fill_sub), fill_sub.ctypes.data_as(i32), None, None)
    assert used == min(G, nb)
    tasks = np.zeros((nT.value, 6), dtype=np.int64)
    clear = np.zeros((nC.value, 2), dtype=np.int64)
    group_of = np.zeros(nb, dtype=np.int32)
    group_level = np.zeros(used + 1, dtype=np.int32)
    perm = np.zeros(len(fill_sub), dtype=np.int32)
    start = np.zeros(used + 1, dtype=np.int32)
    assert f(*head, tasks.ctypes.data_as(i64), C.byref(nT), group_of.ctypes.data_as(i32), group_level.ctypes.data_as(i32),
             clear.ctypes.data_as(i64), C.byref(nC), len(fill_sub), fill_sub.ctypes.data_as(i32), perm.ctypes.data_as(i32),
             start.ctypes.data_as(i32)) == used
    return dict(G=used, tasks=tasks, clear=clear, group_of=group_of, group_level=group_level, perm=perm, start=start)


@pytest.fixture(scope="module")
def toy():
    nt, live, pat, fill_sub = toy_blocks()
    return fill_sub, {G: plan_grouped(nt, live, pat, fill_sub, G) for G in (1, 2, 3, 5)}


@pytest.mark.parametrize("G", [2, 3, 5])
def test_grouped_level_table_holds_every_task_once_in_its_subdomains_group(toy, G):
    _, plans = toy
    one, grp = plans[1], plans[G]
    key = lambda t: tuple(int(v) for v in t[1:])            # (level, block, tile written, post, products)
    assert sorted(map(key, one["tasks"])) == sorted(map(key, grp["tasks"]))
    assert len(set(map(key, one["tasks"]))) == len(one["tasks"])       # (a tile is written by one task per level: the keys are unique)
    assert (grp["tasks"][:, 0] == grp["group_of"][grp["tasks"][:, 2]]).all()
    assert (np.bincount(grp["group_of"], minlength=G) > 0).all()
    # the groups lie one behind the other, and inside a group the levels ascend from 1 to the group's count
    assert (np.diff(grp["tasks"][:, 0]) >= 0).all()
    for g in range(G):
        lv = grp["tasks"][grp["tasks"][:, 0] == g, 1]
        assert (np.diff(lv) >= 0).all() and lv.min() >= 1
        assert lv.max() == grp["group_level"][g + 1] - grp["group_level"][g]


@pytest.mark.parametrize("G", [2, 3, 5])
def test_a_subdomains_tasks_keep_the_level_order_of_the_ungrouped_schedule(toy, G):
    _, plans = toy
    one, grp = plans[1], plans[G]
    for b in range(len(grp["group_of"])):
        a = one["tasks"][one["tasks"][:, 2] == b]
        c = grp["tasks"][grp["tasks"][:, 2] == b]
        assert (np.diff(a[:, 1]) >= 0).all() and (np.diff(c[:, 1]) >= 0).all()
        # level by level the same tasks (the order inside a level is the dealing to the XCD lanes, which a group does for itself)
        for l in np.unique(a[:, 1]):
            assert sorted(map(tuple, a[a[:, 1] == l][:, 1:].tolist())) == sorted(map(tuple, c[c[:, 1] == l][:, 1:].tolist()))
        assert len(a) == len(c)


@pytest.mark.parametrize("G", [2, 3, 5])
def test_clear_and_fill_partitions_are_disjoint_and_cover_the_ungrouped_lists(toy, G):
    fill_sub, plans = toy
    one, grp = plans[1], plans[G]
    assert len(set(grp["clear"][:, 1].tolist())) == len(grp["clear"])                    # disjoint
    assert sorted(grp["clear"][:, 1].tolist()) == sorted(one["clear"][:, 1].tolist())      # union = the ungrouped list
    assert (np.diff(grp["clear"][:, 0]) >= 0).all()
    # a cleared tile belongs to the group of the subdomain whose storage holds it: the same tile is written by that group's tasks
    written = {int(t[3]): int(t[0]) for t in grp["tasks"]}
    hits = 0
    for g, off in grp["clear"].tolist():
        if off in written:
            hits += 1
            assert written[off] == g
    assert hits > 0
    perm, start = grp["perm"], grp["start"]
    assert sorted(perm.tolist()) == list(range(len(fill_sub)))                              # disjoint, union = every entry
    assert start[0] == 0 and start[-1] == len(fill_sub) and (np.diff(start) >= 0).all()
    for g in range(G):
        part = perm[start[g]:start[g + 1]]
        assert (grp["group_of"][fill_sub[part]] == g).all()
        assert (np.diff(part) > 0).all()                                                    # each group's entries in their old order
    assert np.array_equal(one["perm"], np.arange(len(fill_sub)))
