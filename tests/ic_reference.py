"""numpy restatement of LBFGS-HI's block incomplete Cholesky (dot_amd/csrc/k_ic.hip, dotmi_ic.hip): the 3 x 3 block IC(0) of the
projected Hessian on its own block pattern in the multicolour ordering of dotmi_plan_ic, the diagonal-shift restart, and the
solve (L L^T)^-1 b.  It takes the ordering and every list from the plan and follows the kernels operation for operation: plain
multiplies and adds in the plan's list order, (a0 b0 + a1 b1) + a2 b2 per 3-term product, divisions and square roots where the
kernels have them.  Vectorised colour by colour (a colour's vertices share no edge), slot by slot inside a colour; `loop=True` runs
the same arithmetic one vertex at a time (the cross-check of the vectorisation, tests/test_ic_host.py).

Factor storage as dotmi_ic_factor returns it: (nL + nV, 3, 3), the lower blocks in plan order, then the lower-triangular diagonal
blocks by order position."""
import ctypes as C

import numpy as np

from dot_amd import lib as dl

MAX_ATTEMPTS = 40
FIRST_SHIFT = 1e-3


def plan_ic(T, nV):
    """dotmi_plan_ic (host only) -> dict of the plan's arrays"""
    L = dl.load()
    T = np.ascontiguousarray(T, dtype=np.int32)
    nT = T.shape[0]
    sizes = np.zeros(3, dtype=np.int32)
    none = [None] * 9
    assert L.dotmi_plan_ic(nV, nT, dl.ip(T), dl.ip(sizes), *none) == 0
    nc, nL, nP = (int(v) for v in sizes)
    shapes = dict(colour=nV, pos=nV, lptr=nV + 1, lidx=nL, lsrc=nL, dsrc=nV, pptr=nL + 1, pa=nP, pb=nP)
    P = {k: np.zeros(max(n, 1), dtype=np.int32) for k, n in shapes.items()}
    assert L.dotmi_plan_ic(nV, nT, dl.ip(T), dl.ip(sizes), *(dl.ip(P[k]) for k in shapes)) == 0
    P = {k: P[k][:n] for k, n in shapes.items()}
    P.update(nV=nV, nL=nL, nP=nP, nColours=nc)
    return P


def adjacency(T, nV):
    """the block pattern of the global Hessian: vertex adjacency incl. self, ascending -> (adj_ptr, adj_idx)"""
    T = np.asarray(T)
    a = np.repeat(T, 4, axis=1).ravel()
    b = np.tile(T, (1, 4)).ravel()
    key = np.unique(a.astype(np.int64) * nV + b)
    rows, cols = key // nV, key % nV
    ptr = np.zeros(nV + 1, dtype=np.int64)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr), cols.astype(np.int64)


def _prod(A, B):
    """(A B^T)[r][c] = (A[r,0] B[c,0] + A[r,1] B[c,1]) + A[r,2] B[c,2], batched"""
    return (A[:, :, None, 0] * B[:, None, :, 0] + A[:, :, None, 1] * B[:, None, :, 1]) + A[:, :, None, 2] * B[:, None, :, 2]


def _matvec(A, v):
    """(A v)[r] = (A[r,0] v0 + A[r,1] v1) + A[r,2] v2, batched"""
    return (A[:, :, 0] * v[:, None, 0] + A[:, :, 1] * v[:, None, 1]) + A[:, :, 2] * v[:, None, 2]


def _right_solve(T, d):
    """X with X d^T = T, d lower triangular (row by row, as the kernel)"""
    X = np.empty_like(T)
    X[:, :, 0] = T[:, :, 0] / d[:, None, 0, 0]
    X[:, :, 1] = (T[:, :, 1] - X[:, :, 0] * d[:, None, 1, 0]) / d[:, None, 1, 1]
    X[:, :, 2] = ((T[:, :, 2] - X[:, :, 0] * d[:, None, 2, 0]) - X[:, :, 1] * d[:, None, 2, 1]) / d[:, None, 2, 2]
    return X


def _chol3(E):
    """lower Cholesky factor of the 3 x 3 blocks from their lower triangles; ok: every scalar pivot positive (else the identity)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d00, d10, d11, d20, d21, d22 = E[:, 0, 0], E[:, 1, 0], E[:, 1, 1], E[:, 2, 0], E[:, 2, 1], E[:, 2, 2]
        ok = d00 > 0.0
        l00 = np.sqrt(d00)
        l10, l20 = d10 / l00, d20 / l00
        p11 = d11 - l10 * l10
        ok &= p11 > 0.0
        l11 = np.sqrt(p11)
        l21 = (d21 - l20 * l10) / l11
        p22 = (d22 - l20 * l20) - l21 * l21
        ok &= p22 > 0.0
        l22 = np.sqrt(p22)
    Lo = np.zeros_like(E)
    Lo[:, 0, 0], Lo[:, 1, 0], Lo[:, 1, 1], Lo[:, 2, 0], Lo[:, 2, 1], Lo[:, 2, 2] = l00, l10, l11, l20, l21, l22
    Lo[~ok] = np.eye(3)
    return Lo, ok


class ICReference:
    def __init__(self, plan, loop=False):
        P = self.P = plan
        self.nV, self.nL = P["nV"], P["nL"]
        self.shift, self.attempts = 0.0, 0      # of the last successful factorisation (the state of the shift policy)
        self.F = None
        lptr, lidx = P["lptr"].astype(np.int64), P["lidx"].astype(np.int64)
        self.vert = np.empty(self.nV, dtype=np.int64)
        self.vert[P["pos"]] = np.arange(self.nV)
        # upper entries per position: the blocks of later rows in its column, ascending row (a stable sort of the CSR by column)
        rowOf = np.repeat(np.arange(self.nV), np.diff(lptr))
        self.ublk = np.argsort(lidx, kind="stable")
        self.urow = rowOf[self.ublk]
        self.uptr = np.concatenate([[0], np.cumsum(np.bincount(lidx, minlength=self.nV))])
        cnt = np.bincount(P["colour"], minlength=P["nColours"])
        cstart = np.concatenate([[0], np.cumsum(cnt)])
        # the groups the arithmetic runs on: whole colours, or one vertex at a time in the same order
        if loop:
            self.groups = [np.array([p]) for p in range(self.nV)]
        else:
            self.groups = [np.arange(cstart[c], cstart[c + 1]) for c in range(P["nColours"])]
        pptr = P["pptr"].astype(np.int64)
        self.fsched, self.lsched, self.usched = [], [], []
        for rows in self.groups:
            deg = lptr[rows + 1] - lptr[rows]
            slots = []
            for m in range(int(deg.max()) if rows.size else 0):
                sel = np.nonzero(deg > m)[0]
                s = lptr[rows[sel]] + m
                np_ = pptr[s + 1] - pptr[s]
                prods = []
                for t in range(int(np_.max()) if s.size else 0):
                    w = np.nonzero(np_ > t)[0]
                    q = pptr[s[w]] + t
                    prods.append((w, P["pa"][q].astype(np.int64), P["pb"][q].astype(np.int64)))
                slots.append((sel, s, lidx[s], prods))
            self.fsched.append(slots)
            udeg = self.uptr[rows + 1] - self.uptr[rows]
            us = []
            for m in range(int(udeg.max()) if rows.size else 0):
                sel = np.nonzero(udeg > m)[0]
                u = self.uptr[rows[sel]] + m
                us.append((sel, self.ublk[u], self.urow[u]))
            self.usched.append(us)

    # ---- factor --------------------------------------------------------------------------------------------------------
    def fill(self, blocks, sigma):
        """blocks: (nnzb, 3, 3) of the global block-CSR; the diagonal gets A_ii += sigma diag(A_ii)"""
        P = self.P
        blocks = np.asarray(blocks).reshape(-1, 3, 3)
        F = np.empty((self.nL + self.nV, 3, 3))
        F[:self.nL] = blocks[P["lsrc"]]
        D = blocks[P["dsrc"]].copy()
        for e in range(3):
            D[:, e, e] = D[:, e, e] + sigma * D[:, e, e]
        F[self.nL:] = D
        return F

    def factor_attempt(self, blocks, sigma):
        """one fill + factorisation -> (F, ok)"""
        F = self.fill(blocks, sigma)
        nL = self.nL
        allok = True
        for rows, slots in zip(self.groups, self.fsched):
            for sel, s, j, prods in slots:
                T = F[s]
                for w, a, b in prods:
                    T[w] = T[w] - _prod(F[a], F[b])
                F[s] = _right_solve(T, F[nL + j])
            E = F[nL + rows]
            for sel, s, j, prods in slots:
                A = F[s]
                E[sel] = E[sel] - _prod(A, A)
            Lo, ok = _chol3(E)
            F[nL + rows] = Lo
            allok = allok and bool(ok.all())
        return F, allok

    def factor(self, blocks):
        """the shift policy of dotmi_ic.hip: first attempt at half the last successful shift (0 stays 0); a breakdown doubles it
        from 1e-3; at most 40 attempts.  Returns True on success (self.F, self.shift, self.attempts are then the new ones)"""
        sigma = 0.0 if self.shift == 0.0 else 0.5 * self.shift
        for attempt in range(1, MAX_ATTEMPTS + 1):
            F, ok = self.factor_attempt(blocks, sigma)
            if ok:
                self.F, self.shift, self.attempts = F, sigma, attempt
                return True
            if attempt < MAX_ATTEMPTS:
                sigma = max(FIRST_SHIFT, 2.0 * sigma)
        self.attempts = MAX_ATTEMPTS
        return False

    # ---- solve ---------------------------------------------------------------------------------------------------------
    def solve(self, b, F=None):
        """(L L^T)^-1 b; b, result: (nV, 3) in vertex order"""
        F = self.F if F is None else F
        nL = self.nL
        b = np.asarray(b, dtype=np.float64).reshape(self.nV, 3)
        y = np.empty((self.nV, 3))       # order position
        for rows, slots in zip(self.groups, self.fsched):
            t = b[self.vert[rows]].copy()
            for sel, s, j, _ in slots:
                t[sel] = t[sel] - _matvec(F[s], y[j])
            d = F[nL + rows]
            y0 = t[:, 0] / d[:, 0, 0]
            y1 = (t[:, 1] - d[:, 1, 0] * y0) / d[:, 1, 1]
            y2 = ((t[:, 2] - d[:, 2, 0] * y0) - d[:, 2, 1] * y1) / d[:, 2, 2]
            y[rows] = np.stack([y0, y1, y2], axis=1)
        x = np.empty((self.nV, 3))       # order position too; permuted at the end
        for rows, us in zip(self.groups[::-1], self.usched[::-1]):
            t = y[rows].copy()
            for sel, s, k in us:
                t[sel] = t[sel] - _matvec(F[s].transpose(0, 2, 1), x[k])
            d = F[nL + rows]
            x2 = t[:, 2] / d[:, 2, 2]
            x1 = (t[:, 1] - d[:, 2, 1] * x2) / d[:, 1, 1]
            x0 = ((t[:, 0] - d[:, 1, 0] * x1) - d[:, 2, 0] * x2) / d[:, 0, 0]
            x[rows] = np.stack([x0, x1, x2], axis=1)
        out = np.empty((self.nV, 3))
        out[self.vert] = x
        return out

    def dense_product(self, F=None):
        """L L^T as a dense (3 nV, 3 nV) matrix in VERTEX order (small meshes: the defining property of IC(0))"""
        F = self.F if F is None else F
        n = self.nV
        Lm = np.zeros((3 * n, 3 * n))
        lptr, lidx = self.P["lptr"], self.P["lidx"]
        for p in range(n):
            i = self.vert[p]
            Lm[3 * i:3 * i + 3, 3 * i:3 * i + 3] = F[self.nL + p]
            for s in range(lptr[p], lptr[p + 1]):
                j = self.vert[lidx[s]]
                Lm[3 * i:3 * i + 3, 3 * j:3 * j + 3] = F[s]
        return Lm @ Lm.T


class ICSolver:
    """the oracle's external solver (dor_use_ext_solver) for its ONE subdomain, the whole mesh: factor(blocks) receives every 3 x 3
    block of the oracle's H in CSR order and runs the restatement's factorisation with its shift policy, solve applies it"""

    def __init__(self, ref):
        from tests import oracle_py as O
        self.ref = ref
        self.log = []            # (shift, attempts) of every factorisation
        self.nnzb = None
        n = ref.nV
        CREATE = C.CFUNCTYPE(C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ubyte))
        FACTOR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))
        SOLVE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_double))
        DESTROY = C.CFUNCTYPE(None, C.c_void_p)

        def create(nv, p, i, f):
            assert nv == n
            self.nnzb = p[nv]
            return 1

        def factor(hd, blocks):
            a = np.ctypeslib.as_array(blocks, shape=(9 * self.nnzb,)).reshape(-1, 3, 3)
            ok = self.ref.factor(a)
            self.log.append((self.ref.shift, self.ref.attempts))
            return 0 if ok else 1

        def solve(hd, b):
            a = np.ctypeslib.as_array(b, shape=(3 * n,)).reshape(n, 3)
            a[:] = self.ref.solve(a)

        self.cbs = (CREATE(create), FACTOR(factor), SOLVE(solve), DESTROY(lambda hd: None))
        self.api = O.ExtSolverAPI(*(C.cast(c, C.c_void_p) for c in self.cbs))

    def bind(self, orc):
        from tests import oracle_py as O
        L = O.lib()
        L.dor_use_ext_solver.argtypes = [C.c_void_p, C.c_void_p]
        L.dor_use_ext_solver.restype = C.c_int
        assert L.dor_use_ext_solver(orc.h, C.byref(self.api)) == 0


def oracle_whole_mesh(sc, energy_id):
    """the oracle as LBFGS-H on the whole mesh (one subdomain, unit first step): what an ICSolver is bound to"""
    from tests import oracle_py as O
    cfg = sc.cfg
    ep = np.zeros(sc.T.shape[0], dtype=np.int32)
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, energy_id, cfg.dt, sc.fixed, sc.x0, ep, 1, cfg.with_gravity)
    orc.set_alpha_min(1.0)
    return orc
