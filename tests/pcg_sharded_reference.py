"""Newton-PCG on sharded handles (DOTMI_FLAG_NEWTON_PCG_DIST; pcg_iteration in dot_amd/csrc/dotmi_pcg.hip): the numpy restatement of
the sharded iteration with sharded Hessian rows -- tests/pcg_reference.pcg with w = M_sym r and s = H w, gamma, delta taken the way
the ranks take them: every rank's share of zsum = S q from the block solves of ITS subdomains, summed (the first collective); every
rank's rows [v0, v1) of H w with its parts of gamma = r.w and delta = w.s in the packet [s | gamma | delta], summed (the second).
The plan -- who owns which subdomains and which rows -- is the library's own (dotmi_plan_rank, the code dotmi_create runs).
TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

from dot_amd import lib as dl


def rank_plan(sc, ep, n, world):
    """[(p0, p1, v0, v1)] of every rank from dotmi_plan_rank: its subdomains [p0, p1) and its rows [v0, v1)"""
    L = dl.load()
    T = np.ascontiguousarray(sc.T, dtype=np.int32)
    ep = np.ascontiguousarray(ep, dtype=np.int32)
    out = []
    for rank in range(world):
        p0, p1, ne, v0, v1 = (C.c_int32() for _ in range(5))
        assert L.dotmi_plan_rank(sc.V_rest.shape[0], T.shape[0], dl.ip(T), dl.ip(ep), n, rank, world, C.byref(p0), C.byref(p1), None,
                                 C.byref(ne), C.byref(v0), C.byref(v1), None) == 0
        out.append((p0.value, p1.value, v0.value, v1.value))
    return out


def subdomain_solves(orc, n):
    """per subdomain (its vertices, q_s -> H_s^-1 q_s) from the oracle's dense subdomain matrices, factorised once"""
    out = []
    for p in range(n):
        Lc = np.linalg.cholesky(orc.part_dense(p))
        Li = np.linalg.inv(Lc)                                      # (triangular; applied twice: H_s^-1 = Li^T Li)
        out.append((orc.part_verts(p), lambda q, Li=Li: Li.T @ (Li @ q)))
    return out


def pcg_sharded(spmv, solves, plan, dup, b, rel_tol, max_iter):
    """H u = b from u = 0 as `world` ranks run it -> (u, iterations, residuals, state) like tests/pcg_reference.pcg, and the payloads
    [(doubles of the first collective, doubles of the second)] of every iteration"""
    b = np.asarray(b, dtype=np.float64)
    nV = b.shape[0]
    isd = 1.0 / np.sqrt(np.asarray(dup, dtype=np.float64))[:, None]
    u, r = np.zeros_like(b), b.copy()
    d, Hd = np.zeros_like(b), np.zeros_like(b)
    bb = float(np.vdot(b, b))
    rr, gamma_old, alpha_old = bb, 1.0, 1.0
    res = [1.0 if bb > 0.0 else 0.0]
    tol2 = rel_tol * rel_tol * bb
    k, payloads = 0, []
    while True:
        if rr <= tol2:
            return u, k, res, 1, payloads
        if k >= max_iter:
            return u, k, res, 0, payloads
        q = r * isd
        zsum = np.zeros_like(b)                                     # the first collective: the ranks' shares of S q
        for p0, p1, _, _ in plan:
            share = np.zeros_like(b)
            for vs, solve in solves[p0:p1]:
                share[vs] += solve(q[vs].ravel()).reshape(-1, 3)
            zsum += share
        w = zsum * isd                                              # pointwise from the summed zsum: whole on every rank
        packet = np.zeros(3 * nV + 2)                               # the second collective: [s | gamma | delta]
        Hw = spmv(w)
        for _, _, v0, v1 in plan:
            mine = np.zeros(3 * nV + 2)
            mine[3 * v0:3 * v1] = Hw[v0:v1].ravel()                 # the rank's rows of H w, zeros outside its slice
            mine[-2] = float(np.vdot(r[v0:v1], w[v0:v1]))
            mine[-1] = float(np.vdot(w[v0:v1], Hw[v0:v1]))
            packet += mine
        payloads.append((zsum.size, packet.size))
        s, gamma, delta = packet[:-2].reshape(nV, 3), float(packet[-2]), float(packet[-1])
        if not (gamma > 0.0 and np.isfinite(gamma)):
            return u, k, res, 2, payloads
        beta = 0.0 if k == 0 else gamma / gamma_old
        den = delta if k == 0 else delta - beta * gamma / alpha_old
        if not (den > 0.0 and np.isfinite(den)):
            return u, k, res, 2, payloads
        alpha = gamma / den
        d = w + beta * d
        Hd = s + beta * Hd
        u = u + alpha * d
        r = r - alpha * Hd
        rr = float(np.vdot(r, r))                                   # a redundant sum over the replicated r
        gamma_old, alpha_old = gamma, alpha
        k += 1
        res.append(np.sqrt(rr / bb))
