"""The balanced form of DOT's rigid-mode coarse term (dotmi_set_dot_coarse_mode, mode 2; dot_amd/csrc/k_coarse.hip, dotmi_coarse.hip,
coarse_plan.hpp's CoarseHzPlan): the numpy restatement over tests/coarse_reference.py.  With Z, A0 = Z^T H Z, the dropped-subdomain
and the pivot rule of mode 1 and W = H Z,
    C = Z A0^-1 Z^T,    M'' = C + (I - C H) M (I - H C),
applied as  y1 = A0^-1 Z^T r,  r1 = r - W y1,  u = M r1,  y2 = A0^-1 W^T u,  M'' r = u + Z (y1 - y2).  M is the block preconditioner as
a callable; nothing relies on its symmetry.  M'' H Z y = Z y.  An A0 that is not positive definite leaves plain M.  TEST INFRASTRUCTURE."""
import numpy as np

from dot_amd import lib as dl
from tests import coarse_reference as CR


def hz(Z, live, spmv):
    """W = H Z column by column through the operator; zero columns on the dropped subdomains"""
    W = np.zeros_like(Z)
    for c in range(Z.shape[1]):
        if live[c // 6]:
            W[:, c] = spmv(Z[:, c].reshape(-1, 3)).ravel()
    return W


def balanced(m_plain, Z, A0, W):
    """r -> M'' r, or m_plain itself when A0 is not positive definite (the term is switched off)"""
    try:
        Lc = np.linalg.cholesky(A0)
    except np.linalg.LinAlgError:
        return m_plain

    def solve(c):
        return np.linalg.solve(Lc.T, np.linalg.solve(Lc, c))

    def apply(r):
        r = np.asarray(r, dtype=np.float64).ravel()
        y1 = solve(Z.T @ r)
        u = np.asarray(m_plain((r - W @ y1).reshape(-1, 3))).ravel()
        y2 = solve(W.T @ u)
        return (u + Z @ (y1 - y2)).reshape(-1, 3)
    return apply


def parts(x, dup, part_verts, fixed, spmv):
    """Z, A0, W and the live flags at the positions x on the operator spmv"""
    Z, cen, live, w = CR.build_z(x, dup, part_verts, fixed)
    W = hz(Z, live, spmv)
    A0 = Z.T @ W
    for s in np.flatnonzero(~live):
        A0[6 * s:6 * s + 6, 6 * s:6 * s + 6] = np.eye(6)
    return Z, A0, W, live


def m_balanced(m_plain, x, dup, part_verts, fixed, spmv):
    """M'' at the positions x from a plain application and a product with H (an oracle's, or a handle's own) -> (callable, active)"""
    Z, A0, W, _ = parts(x, dup, part_verts, fixed, spmv)
    M = balanced(m_plain, Z, A0, W)
    return M, M is not m_plain


def m_second(orc, dup, part_verts, fixed):
    """M'' at the oracle's current positions and factors (call it after the refresh, before the step), like dot_coarse_reference.m_prime"""
    return m_balanced(orc.apply_precond, orc.state()[0], dup, part_verts, fixed, orc.spmv)


# ---- the plan (dotmi_plan_coarse_hz) and W from its lists -----------------------------------------------------------------------------------
def plan_hz(T, epart, nParts, nV):
    """dotmi_plan_coarse_hz (host only) -> dict of the plan's arrays"""
    L = dl.load()
    T = np.ascontiguousarray(T, dtype=np.int32)
    epart = np.ascontiguousarray(epart, dtype=np.int32)
    nT = T.shape[0]
    sizes = np.zeros(2, dtype=np.int32)
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(epart), nParts, dl.ip(sizes), *([None] * 7)) == 0
    nE, nB = (int(v) for v in sizes)
    shapes = dict(hzPtr=nV + 1, hzSub=nE, hzVert=nE, hzBlkPtr=nE + 1, hzBlk=nB, hzTPtr=nParts + 1, hzTEnt=nE)
    P = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in shapes.items()}
    assert L.dotmi_plan_coarse_hz(nV, nT, dl.ip(T), dl.ip(epart), nParts, dl.ip(sizes), *(dl.ip(P[k]) for k in shapes)) == 0
    P = {k: P[k][:n] for k, n in shapes.items()}
    P["sizes"] = (nE, nB)
    return P


def w_from_lists(P, Hb, adj_idx, x, w, cen, live):
    """the sums coarse_hz_kernel forms: per entry (i, t) the 3 x 6 block sum over the entry's H blocks (i, j) of H_ij Z_tj, as a dense
    (3 nV, 6 nParts) matrix; zero blocks on the dropped subdomains"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    W = np.zeros((3 * x.shape[0], 6 * live.size))
    for e, (i, t) in enumerate(zip(P["hzVert"], P["hzSub"])):
        if not live[t]:
            continue
        blk = P["hzBlk"][P["hzBlkPtr"][e]:P["hzBlkPtr"][e + 1]]
        j = adj_idx[blk]
        Zj = w[j, None, None] * np.concatenate([np.broadcast_to(np.eye(3), (j.size, 3, 3)), -CR.cross_matrix(x[j] - cen[t])], axis=2)
        W[3 * i:3 * i + 3, 6 * t:6 * t + 6] = np.einsum("kab,kbc->ac", Hb[blk], Zj)
    return W
