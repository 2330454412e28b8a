"""DOTMI_FLAG_DOT_COARSE on sharded handles, the host side (no GPU): who assembles which pair of the coarse matrix and what the ranks'
restrictions add up to, from the library's own plans -- dotmi_plan_coarse (the pairs and their H blocks), dotmi_plan_rank with
dotmi_plan_shards behind it (the subdomains [p0, p1) of every rank, the code dotmi_create runs).

With a sharded Hessian refresh a rank holds the block rows of its subdomains' vertices whole and assembles the pairs (s, t), s <= t,
whose s it owns; the blocks are summed over the ranks.  That is exact iff every pair has exactly one assembler and every H block its
list names lies in a row the assembler holds.  Per application the rank's c_s = Z_s^T r, zeros for the others' subdomains, ride in the
tail of the z packet: their sum over the ranks must be the whole Z^T r, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import pcg_reference as R

CASES = [("synbar:48x4x4:12", 3), ("bunny5K_LTSS", 2)]


def rank_parts(sc, ep, n, world):
    """[p0, p1) of every rank from dotmi_plan_rank"""
    L = dl.load()
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    ep = np.ascontiguousarray(ep, dtype=np.int32)
    out = []
    for rank in range(world):
        p0, p1, ne, v0, v1 = (C.c_int32() for _ in range(5))
        assert L.dotmi_plan_rank(sc.V_rest.shape[0], T.shape[0], dl.ip(T), dl.ip(ep), n, rank, world, C.byref(p0), C.byref(p1), None,
                                 C.byref(ne), C.byref(v0), C.byref(v1), None) == 0
        out.append((p0.value, p1.value))
    first = np.zeros(world + 1, dtype=np.int32)
    psz = np.array([3 * np.unique(T[ep == s]).size for s in range(n)], dtype=np.int32)
    assert L.dotmi_plan_shards(n, dl.ip(psz), world, dl.ip(first)) == 0
    assert out == [(int(first[r]), int(first[r + 1])) for r in range(world)]
    return out


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    name, world = request.param
    sc, ep, n = load_workload(name)
    nV = sc.V_rest.shape[0]
    own = rank_parts(sc, ep, n, world)
    assert own[0][0] == 0 and own[-1][1] == n and all(a[1] == b[0] for a, b in zip(own, own[1:]))
    assert sum(p1 > p0 for p0, p1 in own) >= 2                      # real partial ownership
    verts = [np.unique(np.asarray(sc.T)[np.asarray(ep) == s]) for s in range(n)]
    return sc, ep, n, nV, own, verts, CR.plan(sc.T, ep, n, nV)


def test_every_pair_is_assembled_by_exactly_one_rank_the_owner_of_s(case):
    sc, ep, n, nV, own, verts, P = case
    s, t = P["pairS"], P["pairT"]
    assert s.size > n and (s <= t).all()
    who = np.stack([(s >= p0) & (s < p1) for p0, p1 in own])        # (world, nPairs): the kernel's test on st.x
    assert (who.sum(axis=0) == 1).all()
    for r, (p0, p1) in enumerate(own):
        assert np.array_equal(np.flatnonzero(who[r]), np.flatnonzero((s >= p0) & (s < p1)))
    # and the ranks have work to exchange: some pair couples subdomains of two ranks
    owner_of = np.concatenate([np.full(p1 - p0, r) for r, (p0, p1) in enumerate(own)])
    assert (owner_of[s] != owner_of[t]).any()


def test_every_block_of_a_pair_lies_in_a_row_its_assembler_holds(case):
    """the rows a rank's sharded refresh assembles whole are those of its subdomains' vertices (and its slice of the SpMV, which is
    not needed here)"""
    sc, ep, n, nV, own, verts, P = case
    _, _, blk_row = CR.block_csr(sc.T, nV)
    for p0, p1 in own:
        held = np.zeros(nV, dtype=bool)
        for q in range(p0, p1):
            held[verts[q]] = True
        for p in np.flatnonzero((P["pairS"] >= p0) & (P["pairS"] < p1)):
            blk = P["pairBlk"][P["pairPtr"][p]:P["pairPtr"][p + 1]]
            assert blk.size > 0 and held[blk_row[blk]].all(), (p0, p1, p)


def test_ranks_restrictions_with_zeros_elsewhere_sum_to_the_whole(case):
    sc, ep, n, nV, own, verts, P = case
    fixed = np.asarray(sc.fixed, dtype=bool)
    x = np.asarray(sc.x0, dtype=np.float64) + 0.01 * np.random.default_rng(7).standard_normal((nV, 3))
    Z, cen, live, w = CR.build_z(x, R.dup_of(sc.T, ep, nV), verts, fixed)
    assert live.all()
    r = np.random.default_rng(8).standard_normal(3 * nV)

    def restrict(s):                                                # c_s = Z_s^T r
        return np.array([np.dot(Z[:, 6 * s + a], r) for a in range(6)])
    whole = np.concatenate([restrict(s) for s in range(n)])
    assert np.abs(whole - Z.T @ r).max() <= 1e-12 * np.abs(whole).max()
    total = np.zeros(6 * n)
    for p0, p1 in own:                                              # the all-reduce: the ranks' packets' tails, added rank by rank
        mine = np.zeros(6 * n)
        for s in range(p0, p1):
            mine[6 * s:6 * s + 6] = restrict(s)
        assert np.count_nonzero(mine[:6 * p0]) == 0 and np.count_nonzero(mine[6 * p1:]) == 0
        total += mine
    assert np.array_equal(total, whole)


def test_flag_is_the_next_free_bit_in_header_and_binding():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    assert dl.FLAG_DOT_COARSE == 4096 and "#define DOTMI_FLAG_DOT_COARSE 4096" in header
    others = [getattr(dl, k) for k in dir(dl) if k.startswith("FLAG_") and k != "FLAG_DOT_COARSE"]
    assert all(dl.FLAG_DOT_COARSE > f and dl.FLAG_DOT_COARSE & f == 0 for f in others)
