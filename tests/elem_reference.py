"""A 60-digit reference of the per-tet element functions (mpmath), independent of every spectral formula in the tree.

Everything is evaluated from the *stored doubles* (rest positions, positions, x~, mu, lambda, density, dt), which convert
to mpmath exactly:  Dm^-1, volume and lumped mass are re-derived here, F = Ds Dm^-1, and

  Fixed-Corotational   Psi = mu |F - R|^2 + lam/2 (J - 1)^2          P = 2 mu (F - R) + lam (J - 1) cof F
  Stable Neo-Hookean   Psi = (mu (|F|^2 - 3) + lam (J - a)^2) / 2    P = mu F + lam (J - a) cof F,   a = 1 + mu / lam

with R = U V^T the rotation-variant polar factor (U, V in SO(3): the sign of det F sits on the smallest singular value).
The element gradient is dt^2 vol P Dm^-T (corner 0: minus the sum of the others) plus the inertia term m (x - x~); the
12x12 *unprojected* element Hessian is the central difference of that gradient (h = 1e-20 at 60 digits: truncation and
cancellation both ~1e-40).

The scales are sums of the absolute values of the terms a double evaluation forms (det F cancels to eps sigma_0^3, which
a scale made from |P| alone would miss):
  S_P   = 2 mu (s0 + 1) + lam (|J| + 1 + mu/lam) s0^2
  S_Psi = mu (s0 + 1)^2 + lam (|J| + 1 + mu/lam)^2
  gradient scale = dt^2 |vol| S_P |Dm^-1|_inf + max_k m_k |x_k - x~_k|_inf
and kappa_R = 1 + s0 / |s1 + s2| (signed s2) is the condition number of the polar factor."""
import mpmath
import numpy as np

M = mpmath.mp.clone()
M.dps = 60
mpf = M.mpf
EPS = float(np.finfo(np.float64).eps)
FCR, SNH = 0, 1
FD_H = mpf(10) ** -20


def m3(a):
    """3x3 list of mpf from anything indexable [i][j] (doubles convert exactly)"""
    return [[mpf(float(a[i][j])) if not isinstance(a[i][j], mpf) else a[i][j] for j in range(3)] for i in range(3)]


def mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def tr(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def cof(F):
    return [[F[(r + 1) % 3][(c + 1) % 3] * F[(r + 2) % 3][(c + 2) % 3] - F[(r + 1) % 3][(c + 2) % 3] * F[(r + 2) % 3][(c + 1) % 3]
             for c in range(3)] for r in range(3)]


def det(F):
    c = cof(F)
    return F[0][0] * c[0][0] + F[0][1] * c[0][1] + F[0][2] * c[0][2]


def inv(F):
    c, d = cof(F), det(F)
    return [[c[j][i] / d for j in range(3)] for i in range(3)]


def fro2(F):
    return sum(F[i][j] * F[i][j] for i in range(3) for j in range(3))


def to_np(A):
    return np.array([[float(v) for v in row] for row in A])


def svd_rot(F):
    """F = U diag(s) V^T with U, V in SO(3), s0 >= s1 >= |s2|, sign(s2) = sign(det F).  Returns U, s (signed), V, R = U V^T.
    (R is undefined where s1 + s2 = 0; what comes back there is one of the limits.)"""
    U, S, Vh = M.svd_r(M.matrix(F))
    U = [[U[i, j] for j in range(3)] for i in range(3)]
    V = [[Vh[j, i] for j in range(3)] for i in range(3)]
    s = [S[0], S[1], S[2]]
    if det(U) < 0:
        for i in range(3):
            U[i][2] = -U[i][2]
        s[2] = -s[2]
    if det(V) < 0:
        for i in range(3):
            V[i][2] = -V[i][2]
        s[2] = -s[2]
    return U, s, V, mul(U, tr(V))


def energy_density(mat, F, mu, lam):
    """Psi(F), P(F) and the signed singular values (FCR; SNH returns s = None: its closed form has no SVD)"""
    J, C = det(F), cof(F)
    if mat == FCR:
        _, s, _, R = svd_rot(F)
        D = [[F[i][j] - R[i][j] for j in range(3)] for i in range(3)]
        psi = mu * fro2(D) + lam / 2 * (J - 1) ** 2
        P = [[2 * mu * D[i][j] + lam * (J - 1) * C[i][j] for j in range(3)] for i in range(3)]
        return psi, P, s
    a = 1 + mu / lam
    psi = (mu * (fro2(F) - 3) + lam * (J - a) ** 2) / 2
    P = [[mu * F[i][j] + lam * (J - a) * C[i][j] for j in range(3)] for i in range(3)]
    return psi, P, None


def dPdF_fd(mat, F, mu, lam):
    """9x9 dP/dF (row 3i+j, column 3k+l) by central differences, as a float64 array (for the eigenvalue screen)"""
    out = np.empty((9, 9))
    for k in range(3):
        for l in range(3):
            Fp = [row[:] for row in F]
            Fm = [row[:] for row in F]
            Fp[k][l] += FD_H
            Fm[k][l] -= FD_H
            Pp, Pm = energy_density(mat, Fp, mu, lam)[1], energy_density(mat, Fm, mu, lam)[1]
            for i in range(3):
                for j in range(3):
                    out[3 * i + j, 3 * k + l] = float((Pp[i][j] - Pm[i][j]) / (2 * FD_H))
    return (out + out.T) / 2


class Tet:
    """One element: rest shape (4,3) doubles, mu, lam, rho, dt doubles."""

    def __init__(self, X4, mu, lam, rho, dt):
        X = [[mpf(float(X4[k][i])) for i in range(3)] for k in range(4)]
        self.Dm = [[X[k + 1][i] - X[0][i] for k in range(3)] for i in range(3)]
        self.DmInv = inv(self.Dm)
        self.vol = det(self.Dm) / 6                 # signed, as the reference's computeFeatures
        self.mass = mpf(float(rho)) * abs(self.vol) / 4   # lumped mass this tet gives each of its corners
        self.mu, self.lam, self.dt = mpf(float(mu)), mpf(float(lam)), mpf(float(dt))
        self.w = self.dt * self.dt * self.vol
        self._kDm = None
        self.DmInv_inf = float(max(sum(abs(v) for v in row) for row in self.DmInv))

    @property
    def kDm(self):
        """kappa_2(Dm)"""
        if self._kDm is None:
            sv = M.svd_r(M.matrix(self.Dm), compute_uv=False)
            self._kDm = float(sv[0] / sv[2])
        return self._kDm

    def F(self, x4):
        Ds = [[x4[k + 1][i] - x4[0][i] for k in range(3)] for i in range(3)]
        return mul(Ds, self.DmInv)

    def elastic(self, mat, x4):
        """dt^2 vol Psi, the 12 elastic gradient entries [3k + c], F, signed sigma"""
        F = self.F(x4)
        psi, P, s = energy_density(mat, F, self.mu, self.lam)
        g = [None] * 12
        for a in range(3):
            for c in range(3):
                g[3 + 3 * a + c] = self.w * sum(self.DmInv[a][j] * P[c][j] for j in range(3))
        for c in range(3):
            g[c] = -g[3 + c] - g[6 + c] - g[9 + c]
        return self.w * psi, g, F, s

    def hessian_fd(self, mat, x4):
        """12x12 unprojected elastic Hessian, central differences of the gradient, float64 array"""
        H = np.empty((12, 12))
        for k in range(4):
            for c in range(3):
                xp = [row[:] for row in x4]
                xm = [row[:] for row in x4]
                xp[k][c] += FD_H
                xm[k][c] -= FD_H
                gp, gm = self.elastic(mat, xp)[1], self.elastic(mat, xm)[1]
                for r in range(12):
                    H[r, 3 * k + c] = float((gp[r] - gm[r]) / (2 * FD_H))
        return H

    def scales(self, F, s=None):
        """signed sigma, kappa_R, S_P, S_Psi of the state F (all float64)"""
        if s is None:
            s = svd_rot(F)[1]
        s0, J = s[0], abs(s[0] * s[1] * s[2])
        den = abs(s[1] + s[2])
        kR = float(1 + s0 / den) if den != 0 else float("inf")
        t = J + 1 + self.mu / self.lam
        SP = 2 * self.mu * (s0 + 1) + self.lam * t * s0 * s0
        SPsi = self.mu * (s0 + 1) ** 2 + self.lam * t * t
        return [float(v) for v in s], kR, float(SP), float(SPsi)


class MeshRef:
    """The incremental potential of a tet mesh at 60 digits: E(x) = sum_e dt^2 vol_e Psi_e + sum_v m_v |x_v - x~_v|^2 / 2."""

    def __init__(self, V_rest, T, mu, lam, rho, dt, mat):
        self.T = np.asarray(T)
        nT = len(self.T)
        mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (nT,))
        lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (nT,))
        self.mat = mat
        self.tets = [Tet(V_rest[self.T[e]], mu[e], lam[e], rho, dt) for e in range(nT)]
        self.mass = [mpf(0)] * len(V_rest)
        for e, t in enumerate(self.tets):
            for v in self.T[e]:
                self.mass[v] = self.mass[v] + t.mass

    @staticmethod
    def _mp(x):
        return [[mpf(float(v)) for v in row] for row in np.asarray(x, dtype=np.float64)]

    def evaluate(self, x, xt, hessians=False):
        """-> dict with E (mpf), g (nV x 3 mpf, no fixed-vertex zeroing), and per element float64 arrays:
        sigma (nT,3), kR, kDm, S_P, S_Psi, gscale, escale, F (nT,3,3 F rounded to double), Fmp (list of mpf F);
        with hessians=True also H (nT,12,12), the finite-difference elastic Hessians."""
        X, Xt = self._mp(x), self._mp(xt)
        nV, nT = len(X), len(self.tets)
        g = [[mpf(0)] * 3 for _ in range(nV)]
        E = mpf(0)
        out = dict(sigma=np.empty((nT, 3)), kR=np.empty(nT), kDm=np.empty(nT), S_P=np.empty(nT), S_Psi=np.empty(nT),
                   gscale=np.empty(nT), escale=np.empty(nT), F=np.empty((nT, 3, 3)), Fmp=[], psi_w=[])
        if hessians:
            out["H"] = np.empty((nT, 12, 12))
        inert = [max(abs(float(self.mass[v] * (X[v][c] - Xt[v][c]))) for c in range(3)) for v in range(nV)]
        for e, t in enumerate(self.tets):
            x4 = [X[v] for v in self.T[e]]
            pw, ge, F, s = t.elastic(self.mat, x4)
            E += pw
            for k, v in enumerate(self.T[e]):
                for c in range(3):
                    g[v][c] = g[v][c] + ge[3 * k + c]
            sig, kR, SP, SPsi = t.scales(F, s)
            out["sigma"][e], out["kR"][e], out["kDm"][e], out["S_P"][e], out["S_Psi"][e] = sig, kR, t.kDm, SP, SPsi
            out["gscale"][e] = abs(float(t.w)) * SP * t.DmInv_inf + max(inert[v] for v in self.T[e])
            out["escale"][e] = abs(float(t.w)) * SPsi + sum(
                float(t.mass * sum((X[v][c] - Xt[v][c]) ** 2 for c in range(3)) / 2) for v in self.T[e])
            out["F"][e] = to_np(F)
            out["Fmp"].append(F)
            out["psi_w"].append(pw)
            if hessians:
                out["H"][e] = t.hessian_fd(self.mat, x4)
        for v in range(nV):
            d2 = sum((X[v][c] - Xt[v][c]) ** 2 for c in range(3))
            E += self.mass[v] * d2 / 2
            for c in range(3):
                g[v][c] = g[v][c] + self.mass[v] * (X[v][c] - Xt[v][c])
        out["E"], out["g"] = E, g
        return out


def g_to_np(g):
    return np.array([[float(v) for v in row] for row in g])


def g_err(g_double, g_ref):
    """|g_double - g_ref| per entry, formed in mpmath (no cancellation in the comparison), float64 array"""
    gd = np.asarray(g_double, dtype=np.float64)
    return np.array([[float(abs(mpf(float(gd[v][c])) - g_ref[v][c])) for c in range(3)] for v in range(len(g_ref))])


# ---- Fixed-Corotational gradient of a whole mesh, for several material fields on one state --------------------------------------
_FCR_GEOMETRY = {}


def _fcr_geometry(V_rest, T, x):
    """per tet (Dm^-1, vol, F - R, cof F, det F, sigma) at 60 digits; cached per (V_rest, T, x): the polar factor, which is what
    costs, does not depend on the material"""
    import hashlib
    V_rest, T, x = np.ascontiguousarray(V_rest, dtype=np.float64), np.ascontiguousarray(T), np.ascontiguousarray(x, dtype=np.float64)
    key = hashlib.sha1(V_rest.tobytes() + T.tobytes() + x.tobytes()).hexdigest()
    if key not in _FCR_GEOMETRY:
        X = MeshRef._mp(x)
        geo = []
        for t in T:
            tet = Tet(V_rest[t], 1.0, 1.0, 1.0, 1.0)
            F = tet.F([X[v] for v in t])
            _, s, _, Rot = svd_rot(F)
            geo.append((tet.DmInv, tet.vol, [[F[i][j] - Rot[i][j] for j in range(3)] for i in range(3)], cof(F), det(F),
                        [float(v) for v in s]))
        _FCR_GEOMETRY.clear()          # one state at a time: a bunny is 19 379 tets
        _FCR_GEOMETRY[key] = geo
    return _FCR_GEOMETRY[key]


def fcr_mesh_gradient(V_rest, T, x, xt, mu, lam, rho, dt, fixed):
    """Gradient of the incremental potential, Fixed-Corotational, per-element mu / lam (nT,), evaluated at 60 digits and rounded
    to double; zero on fixed vertices.  -> g (nV,3), sigma (nT,3) signed singular values"""
    geo = _fcr_geometry(V_rest, T, x)
    X, Xt = MeshRef._mp(x), MeshRef._mp(xt)
    nV = len(X)
    g = [[mpf(0)] * 3 for _ in range(nV)]
    mass = [mpf(0)] * nV
    dt2, rho = mpf(float(dt)) ** 2, mpf(float(rho))
    for e, (t, (DmInv, vol, D, C, J, _)) in enumerate(zip(np.asarray(T), geo)):
        m, l = mpf(float(mu[e])), mpf(float(lam[e]))
        P = [[2 * m * D[i][j] + l * (J - 1) * C[i][j] for j in range(3)] for i in range(3)]
        w = dt2 * vol
        for a in range(3):
            for c in range(3):
                v = w * (DmInv[a][0] * P[c][0] + DmInv[a][1] * P[c][1] + DmInv[a][2] * P[c][2])
                g[t[a + 1]][c] = g[t[a + 1]][c] + v
                g[t[0]][c] = g[t[0]][c] - v
        for v in t:
            mass[v] = mass[v] + rho * abs(vol) / 4
    out = np.array([[float(g[v][c] + mass[v] * (X[v][c] - Xt[v][c])) for c in range(3)] for v in range(nV)])
    out[np.asarray(fixed).astype(bool)] = 0
    return out, np.array([q[5] for q in geo])
