"""The rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse; dot_amd/csrc/k_coarse.hip, dotmi_coarse.hip,
coarse_plan.hpp): the numpy restatement.  M = M_sym + Z A0^-1 Z^T, A0 = Z^T H Z; subdomain s has six columns of Z, on a vertex v of s
the block w_v [I | -[x_v - c_s]x] with w_v = 1 / dup_v on free vertices and 0 on fixed ones and c_s the w-weighted centroid of s; a
subdomain with fewer than 3 free vertices gets zero columns and an identity block in A0; an A0 that is not positive definite switches
the term off.  Z, A0 and the apply are built from x, dup, the subdomains' vertex sets and `fixed`, with H as a callable, and are used
with tests/pcg_reference.pcg.  TEST INFRASTRUCTURE."""
import numpy as np

from dot_amd import lib as dl


def weights(dup, fixed):
    w = 1.0 / np.maximum(np.asarray(dup, dtype=np.float64), 1.0)
    w[np.asarray(fixed, dtype=bool)] = 0.0
    return w


def cross_matrix(d):
    """[d]x for rows of d: (m, 3) -> (m, 3, 3)"""
    d = np.asarray(d, dtype=np.float64)
    C = np.zeros(d.shape[:-1] + (3, 3))
    C[..., 0, 1], C[..., 0, 2] = -d[..., 2], d[..., 1]
    C[..., 1, 0], C[..., 1, 2] = d[..., 2], -d[..., 0]
    C[..., 2, 0], C[..., 2, 1] = -d[..., 1], d[..., 0]
    return C


def build_z(x, dup, part_verts, fixed):
    """-> (Z (3 nV, 6 nParts) dense, centroids (nParts, 3), live (nParts,) bool, w (nV,))"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    nV, nP = x.shape[0], len(part_verts)
    w = weights(dup, fixed)
    free = ~np.asarray(fixed, dtype=bool)
    Z = np.zeros((3 * nV, 6 * nP))
    cen = np.zeros((nP, 3))
    live = np.zeros(nP, dtype=bool)
    for s, vs in enumerate(part_verts):
        vs = np.asarray(vs)
        live[s] = int(free[vs].sum()) >= 3
        if not live[s]:
            continue
        cen[s] = (w[vs, None] * x[vs]).sum(axis=0) / w[vs].sum()
        blk = np.concatenate([np.broadcast_to(np.eye(3), (vs.size, 3, 3)), -cross_matrix(x[vs] - cen[s])], axis=2)   # (m, 3, 6)
        blk = w[vs, None, None] * blk
        rows = (3 * vs[:, None] + np.arange(3)[None, :]).ravel()
        Z[rows, 6 * s:6 * s + 6] = blk.reshape(-1, 6)
    return Z, cen, live, w


def coarse_matrix(Z, live, spmv):
    """A0 = Z^T H Z column by column through the operator; identity blocks on the dropped subdomains"""
    nc = Z.shape[1]
    HZ = np.zeros_like(Z)
    for c in range(nc):
        if live[c // 6]:
            HZ[:, c] = spmv(Z[:, c].reshape(-1, 3)).ravel()
    A0 = Z.T @ HZ
    for s in np.flatnonzero(~live):
        A0[6 * s:6 * s + 6, 6 * s:6 * s + 6] = np.eye(6)
    return A0


def coarse_apply(Z, A0):
    """r -> Z A0^-1 Z^T r through the Cholesky factor of A0, or None when A0 is not positive definite (the term is switched off)"""
    try:
        Lc = np.linalg.cholesky(A0)
    except np.linalg.LinAlgError:
        return None

    def apply(r):
        c = Z.T @ np.asarray(r, dtype=np.float64).ravel()
        y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, c))
        return (Z @ y).reshape(-1, 3)
    return apply


def precond(m_sym, coarse):
    """M = M_sym + the coarse term (M_sym alone when the term is off)"""
    if coarse is None:
        return m_sym
    return lambda r: m_sym(r) + coarse(r)


# ---- the plan (dotmi_plan_coarse) and the assembly from its lists ----------------------------------------------------------------------
def plan(T, epart, nParts, nV):
    """dotmi_plan_coarse (host only) -> dict of the plan's arrays"""
    L = dl.load()
    T = np.ascontiguousarray(T, dtype=np.int32)
    epart = np.ascontiguousarray(epart, dtype=np.int32)
    nT = T.shape[0]
    sizes = np.zeros(3, dtype=np.int32)
    none = [None] * 8
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(epart), nParts, dl.ip(sizes), *none) == 0
    nP, nE, nI = (int(v) for v in sizes)
    shapes = dict(pairS=nP, pairT=nP, pairPtr=nP + 1, pairBlk=nE, vsPtr=nV + 1, vsIdx=nI, svPtr=nParts + 1, svIdx=nI)
    P = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in shapes.items()}
    assert L.dotmi_plan_coarse(nV, nT, dl.ip(T), dl.ip(epart), nParts, dl.ip(sizes), *(dl.ip(P[k]) for k in shapes)) == 0
    P = {k: P[k][:n] for k, n in shapes.items()}
    P["sizes"] = (nP, nE, nI)
    return P


def block_csr(T, nV):
    """the global block-CSR: vertex adjacency incl. self, ascending -> (adj_ptr, adj_idx, row of every block)"""
    T = np.asarray(T)
    a = np.repeat(T, 4, axis=1).ravel()
    b = np.tile(T, (1, 4)).ravel()
    key = np.unique(a.astype(np.int64) * nV + b)
    row, col = (key // nV).astype(np.int32), (key % nV).astype(np.int32)
    ptr = np.zeros(nV + 1, dtype=np.int64)
    np.add.at(ptr, row + 1, 1)
    return np.cumsum(ptr), col, row


def h_blocks(spmv, adj_ptr, adj_idx, blk_row, nV):
    """the 3 x 3 blocks of H in block-CSR order from products with unit vectors: columns whose vertices are more than two edges apart
    share no row, so one product per (colour of a distance-2 colouring, coordinate) recovers them all"""
    nbr = [adj_idx[adj_ptr[v]:adj_ptr[v + 1]] for v in range(nV)]
    colour = np.full(nV, -1, dtype=np.int64)
    for v in range(nV):
        near = np.unique(np.concatenate([nbr[u] for u in nbr[v]]))
        used = set(colour[near].tolist())
        c = 0
        while c in used:
            c += 1
        colour[v] = c
    Hb = np.zeros((adj_idx.size, 3, 3))
    col_colour = colour[adj_idx]
    for c in range(int(colour.max()) + 1):
        sel = np.flatnonzero(col_colour == c)
        for a in range(3):
            e = np.zeros((nV, 3))
            e[colour == c, a] = 1.0
            Hb[sel, :, a] = spmv(e)[blk_row[sel]]
    return Hb


def a0_from_lists(P, Hb, adj_idx, blk_row, x, w, cen, live):
    """the sums the assembly kernel forms: per listed pair (s, t) the 6 x 6 block sum Z_si^T H_ij Z_tj over the pair's H blocks,
    mirrored below the diagonal; identity blocks on the dropped subdomains"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    nP = live.size
    A0 = np.zeros((6 * nP, 6 * nP))
    for p, (s, t) in enumerate(zip(P["pairS"], P["pairT"])):
        if not (live[s] and live[t]):
            continue
        blk = P["pairBlk"][P["pairPtr"][p]:P["pairPtr"][p + 1]]
        i, j = blk_row[blk], adj_idx[blk]
        Zi = w[i, None, None] * np.concatenate([np.broadcast_to(np.eye(3), (i.size, 3, 3)), -cross_matrix(x[i] - cen[s])], axis=2)
        Zj = w[j, None, None] * np.concatenate([np.broadcast_to(np.eye(3), (j.size, 3, 3)), -cross_matrix(x[j] - cen[t])], axis=2)
        B = np.einsum("kab,kbc,kcd->ad", Zi.transpose(0, 2, 1), Hb[blk], Zj)
        A0[6 * s:6 * s + 6, 6 * t:6 * t + 6] = B
        if s != t:
            A0[6 * t:6 * t + 6, 6 * s:6 * s + 6] = B.T
    for s in np.flatnonzero(~live):
        A0[6 * s:6 * s + 6, 6 * s:6 * s + 6] = np.eye(6)
    return A0
