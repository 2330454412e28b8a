"""The H tiles' entry lists of the tile factorisation (DOTMI_TILE_HFILL; build_tile_fill in dot_amd/csrc/block_plan.hpp, the init == 2
tasks of tile_factor.hpp), on the CPU through the host-only entries dotmi_plan_tile_fill (blocks of tiles with the caller's fill
lists: the toy blocks of tests/test_tile_groups.py) and dotmi_plan_tile_fill_mesh (dotmi_create's own planning stages on a mesh:
synbar:16x5x5:2, whose subdomain sizes are no multiples of 64, so its tiles hold identity padding; one-pass and two-level form).
The lists must write exactly what the dense fill (fill_dst / fill_src / pad_dst) writes into a zeroed work buffer, and exactly one
task per H tile -- its first writer -- must start from them."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl
from tests.test_tile_groups import toy_blocks
from tests.workloads import load_workload

u8, i32, i64, f64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
TP_DIAG = 1
LDS_LD = 65                 # the kernels' LDS tile: element (row k, column j) of the column-major global tile at k * 65 + j


def hval_idx(blk, e):
    """dotmi_internal.hpp: Hval keeps eight 3x3 blocks interleaved, entry-major"""
    return (blk >> 3) * 72 + 8 * e + (blk & 7)


def _unpack(counts, G, tasks, clear, pos, src, **more):
    return dict(G=G, n_buf=int(counts[6]), two_level=int(counts[7]), tasks=tasks, clear=clear, pos=pos, src=src, **more)


def toy_fill_lists(nt, live, pat, seed=7):
    """fill lists for the toy blocks in the layout of dotmi_plan_grouped_tile_schedule (row block j of a block: 64 rows of 64 (j + 1)
    columns, the blocks one behind the other): 3x3 blocks on a grid of three inside pattern tiles (rows and columns 0..62 of a
    tile), one scalar in five not stored (-1), the identity padding on position 63 of the diagonal tiles"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([64 * 64 * (j + 1) for j in range(nt)])])
    tot = int(off[-1])
    dst, srcs, pad = [], [], []
    for b in range(live.shape[0]):
        for i in range(nt):
            for j in range(i, nt):
                if not pat[b, i, j]:
                    continue
                corners = rng.choice(21 * 21, size=int(rng.integers(3, 40)), replace=False)
                for c in corners:
                    r0, c0 = 64 * j + 3 * (c // 21), 64 * i + 3 * (c % 21)      # memory row / column of the corner
                    for rc in range(9):
                        a = b * tot + off[r0 // 64] + ((r0 + rc // 3) % 64) * 64 * (j + 1) + c0 + rc % 3
                        dst.append(-1 if rng.random() < 0.2 else int(a))
                    srcs.append(int(rng.integers(0, 5000)))
        for j in range(nt):
            if live[b, j]:
                pad.append(b * tot + int(off[j]) + 63 * 64 * (j + 1) + 64 * j + 63)
    return np.array(dst, dtype=np.int64), np.array(srcs, dtype=np.int32), np.array(pad, dtype=np.int64)


def plan_toy(G):
    nt, live, pat, _ = toy_blocks()
    dst, srcs, pad = toy_fill_lists(nt, live, pat)
    L = C.CDLL(dl.LIB_PATH)
    f = L.dotmi_plan_tile_fill
    f.argtypes = [C.c_int32, C.c_int32, u8, u8, C.c_int32, C.c_int32, C.c_int32, C.c_int64, i64, i32, C.c_int64, i64, i64, i64, i64,
                  i32, i32]
    live = np.ascontiguousarray(live, dtype=np.uint8)
    pat = np.ascontiguousarray(pat, dtype=np.uint8)
    counts = np.zeros(8, dtype=np.int64)
    head = (live.shape[0], nt, live.ctypes.data_as(u8), pat.ctypes.data_as(u8), 2, 1, G, len(srcs), dst.ctypes.data_as(i64),
            srcs.ctypes.data_as(i32), len(pad), pad.ctypes.data_as(i64), counts.ctypes.data_as(i64))
    used = f(*head, None, None, None, None)
    assert used == min(G, live.shape[0]), used
    tasks = np.zeros((counts[0], 10), dtype=np.int64)
    clear = np.zeros((counts[1], 5), dtype=np.int64)
    pos = np.zeros(counts[2], dtype=np.int32)
    src = np.zeros(counts[2], dtype=np.int32)
    assert f(*head, tasks.ctypes.data_as(i64), clear.ctypes.data_as(i64), pos.ctypes.data_as(i32), src.ctypes.data_as(i32)) == used
    return _unpack(counts, used, tasks, clear, pos, src, fill_dst=dst, fill_src=srcs, pad_dst=pad)


def plan_mesh(name, G, two_level):
    sc, ep, n = load_workload(name)
    L = C.CDLL(dl.LIB_PATH)
    f = L.dotmi_plan_tile_fill_mesh
    f.argtypes = [C.c_int32, C.c_int32, i32, f64, i32, C.c_int32, C.c_int32, C.c_int32, i64, i64, i64, i32, i32, i64, i32, i64]
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    X = np.ascontiguousarray(sc.V_rest, dtype=np.float64)
    ep = np.ascontiguousarray(ep, dtype=np.int32)
    counts = np.zeros(8, dtype=np.int64)
    head = (X.shape[0], T.shape[0], T.ctypes.data_as(i32), X.ctypes.data_as(f64), ep.ctypes.data_as(i32), n, G, two_level,
            counts.ctypes.data_as(i64))
    used = f(*head, None, None, None, None, None, None, None)
    assert used == min(G, n), used
    tasks = np.zeros((counts[0], 10), dtype=np.int64)
    clear = np.zeros((counts[1], 5), dtype=np.int64)
    pos = np.zeros(counts[2], dtype=np.int32)
    src = np.zeros(counts[2], dtype=np.int32)
    dst = np.zeros(9 * counts[3], dtype=np.int64)
    srcs = np.zeros(counts[3], dtype=np.int32)
    pad = np.zeros(counts[4], dtype=np.int64)
    assert f(*head, tasks.ctypes.data_as(i64), clear.ctypes.data_as(i64), pos.ctypes.data_as(i32), src.ctypes.data_as(i32),
             dst.ctypes.data_as(i64), srcs.ctypes.data_as(i32), pad.ctypes.data_as(i64)) == used
    return _unpack(counts, used, tasks, clear, pos, src, fill_dst=dst, fill_src=srcs, pad_dst=pad)


MESH = "synbar:16x5x5:2"
CASES = {
    "toy-1": lambda: plan_toy(1), "toy-2": lambda: plan_toy(2),
    "synbar-1": lambda: plan_mesh(MESH, 1, 0), "synbar-2": lambda: plan_mesh(MESH, 2, 0),
    "synbar-two-level-1": lambda: plan_mesh(MESH, 1, 1), "synbar-two-level-2": lambda: plan_mesh(MESH, 2, 1),
}
_plans = {}


@pytest.fixture(params=sorted(CASES))
def plan(request):
    if request.param not in _plans:
        _plans[request.param] = CASES[request.param]()
    return _plans[request.param]


def dense_fill(P, value):
    """what dense_fill_kernel + pad_identity_kernel leave in a zeroed buffer; value(scalar index in Hval)"""
    W = np.zeros(P["n_buf"])
    e = np.arange(len(P["fill_dst"]))
    keep = P["fill_dst"] >= 0
    W[P["fill_dst"][keep]] = value(hval_idx(P["fill_src"][e[keep] // 9].astype(np.int64), e[keep] % 9))
    W[P["pad_dst"]] = 1.0
    return W


def entry_addresses(P):
    """the address in the work buffer every entry stands for: its tile's origin + column j of the LDS tile x the leading dimension
    + row k"""
    tile = np.repeat(np.arange(len(P["clear"])), P["clear"][:, 4])
    assert len(tile) == len(P["pos"])
    assert np.array_equal(P["clear"][:, 3], np.concatenate([[0], np.cumsum(P["clear"][:, 4])[:-1]]))   # contiguous, tile after tile
    k, j = P["pos"] // LDS_LD, P["pos"] % LDS_LD
    assert (k < 64).all() and (j < 64).all() and (P["pos"] >= 0).all()
    return tile, P["clear"][tile, 1] + j.astype(np.int64) * P["clear"][tile, 2] + k


def test_the_lists_write_what_the_dense_fill_writes(plan):
    P = plan
    if "two_level" in P and P is _plans.get("synbar-two-level-1"):
        assert P["two_level"] == 1                              # (the second row-block table is in play)
    value = lambda s: 0.5 + (s % 9973) / 9973.0                 # never 0, never 1: a dropped or misplaced scalar shows
    want = dense_fill(P, value)
    assert (want != 0).sum() > 0 and len(P["pad_dst"]) > 0
    _, addr = entry_addresses(P)
    got = np.zeros(P["n_buf"])
    got[addr] = np.where(P["src"] < 0, 1.0, value(P["src"].astype(np.int64)))
    assert np.array_equal(got, want)
    # no tile position twice (so the scatter above, and the kernel's, is free of races), every entry inside a clear tile
    assert len(np.unique(addr)) == len(addr)
    assert len(addr) == (P["fill_dst"] >= 0).sum() + len(P["pad_dst"])    # unstored mirror copies are dropped, nothing else


def _factorisation_tasks_by_tile(tasks):
    """tile of the work buffer -> the factorisation tasks (form 0: eager updates, row and diagonal tasks) that start from / add to it"""
    by = {}
    for t in tasks[tasks[:, 9] == 0]:
        by.setdefault(int(t[3]), []).append(t)
    return by


def test_one_task_per_h_tile_starts_from_the_list_and_it_is_the_first_writer(plan):
    P = plan
    tasks, clear = P["tasks"], P["clear"]
    by = _factorisation_tasks_by_tile(tasks)
    assert len(set(clear[:, 1].tolist())) == len(clear)
    for c in clear:
        ts = by.get(int(c[1]), [])
        assert ts, c                                            # every H tile has a diagonal or a row task
        assert all(t[0] == c[0] for t in ts)                    # in the tile's own group
        started = [t for t in ts if t[5] == 2]
        assert len(started) == 1, (c, ts)
        s = started[0]
        assert s[7] == c[3] and s[8] == c[4]                    # the tile's own range of entries
        assert s[1] == min(t[1] for t in ts)                    # the first of the tile's tasks in level order ...
        assert sum(t[1] == s[1] for t in ts) == 1               # ... alone in its level
        assert all(t[5] == 1 for t in ts if t is not s)         # the later ones read the tile back
    assert (tasks[:, 5] == 2).sum() == len(clear)


def test_tasks_on_fill_in_tiles_start_from_zero(plan):
    """a tile of the work buffer that is no H tile, and every tile of the inversion: the first task starts from zero (init == 0),
    the later ones from the tile (1), none from a list"""
    P = plan
    tasks = P["tasks"]
    h_tiles = set(P["clear"][:, 1].tolist())
    fill_in = {k: v for k, v in _factorisation_tasks_by_tile(tasks).items() if k not in h_tiles}
    if P["G"] == 1 and P is _plans.get("toy-1"):
        assert fill_in                                          # (the random toy patterns do have fill-in)
    for ts in fill_in.values():
        lv = [t[1] for t in ts]
        assert len(set(lv)) == len(lv)
        for t in ts:
            assert t[5] == (0 if t[1] == min(lv) else 1)
    inv = tasks[tasks[:, 9] == 1]
    assert len(inv) > 0 and not (inv[:, 5] == 2).any()
    assert not ((tasks[:, 5] != 2) & (tasks[:, 8] != 0)).any()   # no range without the mark


def test_two_calls_give_identical_lists():
    a, b = plan_mesh(MESH, 2, 0), plan_mesh(MESH, 2, 0)
    for k in ("tasks", "clear", "pos", "src", "fill_dst", "fill_src", "pad_dst"):
        assert np.array_equal(a[k], b[k]), k
    a, b = plan_toy(2), plan_toy(2)
    for k in ("tasks", "clear", "pos", "src"):
        assert np.array_equal(a[k], b[k]), k
