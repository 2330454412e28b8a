"""The log-regularised Stable Neo-Hookean material (DOTMI_ENERGY_SNH_LOG = 2; StableNHEnergy.cpp, the SNH_WITHLOG branches) at
60 digits, on the primitives of tests/elem_reference.py, and on the designed states of tests/designed_states.py.

  Psi = (mu (|F|^2 - 3 - log(|F|^2 + 1)) + lam (J - a)^2) / 2,   a = 1 + 3 mu / (4 lam)        (:84-89)
  P   = tau F + lam (J - a) cof F,   tau = mu (1 - 1 / (|F|^2 + 1))                             (:237-243)

Neither of the two modules knows this material (their `mat` is 0 or 1, and anything else would fall through to plain Stable
Neo-Hookean), so what branches on the material there is restated here for id 2 only: the density, Tet.elastic / Tet.scales
(subclassed), and the mesh-level helpers of designed_states (reference, pd_mask, normalised_errors, the float64 / LAPACK
evaluation that defines the constants).  Everything else -- meshes, families, rest shapes, error norms -- is theirs.

The scales are, as there, sums of the absolute values of the terms a double evaluation forms; the regulariser adds
mu log(|sigma|^2 + 1) to the energy's and nothing to the stress's (tau <= mu):
  S_P   = 2 mu (s0 + 1) + lam (|J| + 1 + 3 mu / (4 lam)) s0^2
  S_Psi = mu ((s0 + 1)^2 + log(|sigma|^2 + 1)) + lam (|J| + 1 + 3 mu / (4 lam))^2

The three constants of the bounds (designed_states.py:21-23) for this material are derived like today's: 4 x the largest
normalised error of a plain float64 numpy evaluation of the closed form (the Hessian: of the spectral coefficients on LAPACK's
SVD) against the 60-digit reference, over all asserted families (`lapack_constants`, recomputed and compared by
tests/test_snhlog_reference.py).  They are never measured on the kernels."""
import functools

import numpy as np

from tests import designed_states as D
from tests import elem_reference as R

SNH_LOG = 2
mpf = R.mpf

K_PSI = 4 * 6.826     # wide_10
K_P = 4 * 5.509       # scale_1e3
K_H = 4 * 17.43       # pd_c

MU, LAM, EPS = D.MU, D.LAM, D.EPS


def alpha(mu, lam):
    """1 + 3 mu / (4 lam), in the reference's order of operations (what a float64 restatement has to round like)"""
    return 1 + 3 * mu / 4 / lam


def energy_density(F, mu, lam):
    """Psi(F), P(F) at 60 digits (mu, lam mpf; the log is the 60-digit context's)"""
    J, C, S = R.det(F), R.cof(F), R.fro2(F)
    a = alpha(mu, lam)
    psi = (mu * (S - 3 - R.M.log(S + 1)) + lam * (J - a) ** 2) / 2
    tau = mu * (1 - 1 / (S + 1))
    P = [[tau * F[i][j] + lam * (J - a) * C[i][j] for j in range(3)] for i in range(3)]
    return psi, P


def dPdF_fd(F, mu, lam):
    """9x9 dP/dF (row 3i+j, column 3k+l) by central differences at 60 digits, symmetrised, as a float64 array"""
    out = np.empty((9, 9))
    for k in range(3):
        for l in range(3):
            Fp = [row[:] for row in F]
            Fm = [row[:] for row in F]
            Fp[k][l] += R.FD_H
            Fm[k][l] -= R.FD_H
            Pp, Pm = energy_density(Fp, mu, lam)[1], energy_density(Fm, mu, lam)[1]
            for i in range(3):
                for j in range(3):
                    out[3 * i + j, 3 * k + l] = float((Pp[i][j] - Pm[i][j]) / (2 * R.FD_H))
    return (out + out.T) / 2


class Tet(R.Tet):
    def elastic(self, mat, x4):
        assert mat == SNH_LOG
        F = self.F(x4)
        psi, P = energy_density(F, self.mu, self.lam)
        g = [None] * 12
        for a in range(3):
            for c in range(3):
                g[3 + 3 * a + c] = self.w * sum(self.DmInv[a][j] * P[c][j] for j in range(3))
        for c in range(3):
            g[c] = -g[3 + c] - g[6 + c] - g[9 + c]
        return self.w * psi, g, F, None

    def scales(self, F, s=None):
        if s is None:
            s = R.svd_rot(F)[1]
        s0, J = s[0], abs(s[0] * s[1] * s[2])
        den = abs(s[1] + s[2])
        kR = float(1 + s0 / den) if den != 0 else float("inf")
        t = J + alpha(self.mu, self.lam)
        SP = 2 * self.mu * (s0 + 1) + self.lam * t * s0 * s0
        SPsi = self.mu * ((s0 + 1) ** 2 + R.M.log(s[0] ** 2 + s[1] ** 2 + s[2] ** 2 + 1)) + self.lam * t * t
        return [float(v) for v in s], kR, float(SP), float(SPsi)


class MeshRef(R.MeshRef):
    """elem_reference.MeshRef with the tets of this material"""

    def __init__(self, V_rest, T, mu, lam, rho, dt):
        super().__init__(V_rest, T, mu, lam, rho, dt, SNH_LOG)
        for t in self.tets:
            t.__class__ = Tet


# ---- the designed states -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(name, hessians=False):
    """designed_states.reference for id 2"""
    V, T, x = D.mesh(name)
    return MeshRef(V, T, MU, LAM, D.RHO, D.DT).evaluate(x, V, hessians=hessians)


@functools.lru_cache(maxsize=None)
def pd_min_eig(name):
    """per tet: the smallest eigenvalue of the reference's 9x9 dP/dF, in units of mu"""
    mu, lam = mpf(MU), mpf(LAM)
    return np.array([np.linalg.eigvalsh(dPdF_fd(F, mu, lam)).min() / MU for F in reference(name)["Fmp"]])


def pd_mask(name):
    """designed_states.pd_mask for id 2: every eigenvalue of dP/dF >= 0.1 mu"""
    return pd_min_eig(name) >= 0.1


def elastic_escale(name):
    V, T, _ = D.mesh(name)
    vol = np.array([abs(np.linalg.det((V[t[1:]] - V[t[0]]).T)) / 6 for t in T])
    return D.DT * D.DT * vol * reference(name)["S_Psi"]


def normalised_errors(name, psi_w, g, H=None):
    """designed_states.normalised_errors for id 2 (a closed form without a polar factor: no kappa_R in the gradient's bound)"""
    ref = reference(name, hessians=H is not None)
    n = len(D.mesh(name)[1])
    out = {}
    if psi_w is not None:
        err = np.array([float(abs(mpf(float(psi_w[e])) - ref["psi_w"][e])) for e in range(n)])
        out["psi"] = err / (EPS * elastic_escale(name))
    ge = R.g_err(np.asarray(g).reshape(4 * n, 3), ref["g"]).reshape(n, 12).max(axis=1)
    out["g"] = ge / (EPS * ref["kDm"] * ref["gscale"])
    if H is not None:
        ok = pd_mask(name)
        hn = np.abs(ref["H"]).reshape(n, -1).max(axis=1)
        out["H"] = np.where(ok, np.abs(H - ref["H"]).reshape(n, -1).max(axis=1) / (EPS * ref["kR"] * ref["kDm"] ** 2 * hn), np.nan)
    return out


# ---- the plain float64 evaluation that defines the constants ---------------------------------------------------------------
def f64_density(F, mu=MU, lam=LAM):
    C = D._cof(F)
    J = F[0] @ C[0]
    S = (F * F).sum()
    a = alpha(mu, lam)
    return (mu * (S - 3 - np.log(S + 1)) + lam * (J - a) ** 2) / 2, mu * (1 - 1 / (S + 1)) * F + lam * (J - a) * C


def spectral_coefficients(s, mu=MU, lam=LAM):
    """-> dPsi/dsigma (3,), d2Psi/dsigma2 (3,3), B-left (3,) for the pairs (0,1), (1,2), (2,0): StableNHEnergy.cpp:102-114,
    :134-171, :204-216, in their order of operations (float64; s may hold mpf as well: only + - * / are used)"""
    J = s[0] * s[1] * s[2]
    pn = [s[1] * s[2], s[2] * s[0], s[0] * s[1]]
    Sp1 = s[0] * s[0] + s[1] * s[1] + s[2] * s[2] + 1
    a = alpha(mu, lam)
    tau, t = mu * (1 - 1 / Sp1), lam * (J - a)
    d = [s[i] * tau + t * pn[i] for i in range(3)]
    r = mu / (Sp1 * Sp1)
    A = [[None] * 3 for _ in range(3)]
    for i in range(3):
        A[i][i] = mu + lam * pn[i] * pn[i] - (Sp1 - 2 * s[i] * s[i]) * r
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        A[i][j] = A[j][i] = s[k] * (lam * (2 * J - a)) + 2 * pn[k] * r
    tb = mu - mu / Sp1
    bl = [(tb - t * s[2]) / 2, (tb - t * s[0]) / 2, (tb - t * s[1]) / 2]
    return d, A, bl


def spectral_blocks(s, mu=MU, lam=LAM):
    """(A (3,3), B (3,4)) in the layout of spectral_blocks in elem_math.hpp, unprojected, weight 1, float64"""
    d, A, bl = spectral_coefficients(np.asarray(s, dtype=np.float64), mu, lam)
    B = np.empty((3, 4))
    for c in range(3):
        cp = (c + 1) % 3
        r = (d[c] + d[cp]) / (2 * (s[c] + s[cp]))
        B[c] = bl[c] + r, bl[c] - r, bl[c] - r, bl[c] + r
    return np.array(A, dtype=np.float64), B


def spectral_dPdF(U, s, V, mu=MU, lam=LAM):
    return D.spectral_dPdF(SNH_LOG, U, s, V, mu, lam, blocks=spectral_blocks(s, mu, lam))


def f64_element(X4, x4, xt4, hessian=False):
    """designed_states.f64_element for id 2"""
    Dm = (X4[1:] - X4[0]).T
    A = np.linalg.inv(Dm)
    vol = np.linalg.det(Dm) / 6
    F = (x4[1:] - x4[0]).T @ A
    w = D.DT * D.DT * vol
    psi, P = f64_density(F)
    g = np.empty((4, 3))
    g[1:] = w * (A @ P.T)
    g[0] = -g[1:].sum(axis=0)
    g += D.RHO * abs(vol) / 4 * (x4 - xt4)
    if not hessian:
        return w * psi, g.reshape(12), None
    G = np.zeros((9, 12))                       # dF_ij / dx_kc
    for i in range(3):
        for j in range(3):
            for k in range(3):
                G[3 * i + j, 3 * (k + 1) + i] = A[k, j]
                G[3 * i + j, i] -= A[k, j]
    return w * psi, g.reshape(12), G.T @ (w * spectral_dPdF(*D.lapack_svd(F))) @ G


def lapack_errors(name, hessian=False):
    V, T, x = D.mesh(name)
    res = [f64_element(V[t], x[t], V[t], hessian) for t in T]
    return normalised_errors(name, np.array([r[0] for r in res]), np.array([r[1] for r in res]),
                             np.array([r[2] for r in res]) if hessian else None)


@functools.lru_cache(maxsize=None)
def lapack_constants():
    """-> ((K_PSI, K_P, K_H), the families that set them) by their definition: designed_states.lapack_constants for id 2"""
    worst = {"psi": (0.0, None), "g": (0.0, None), "H": (0.0, None)}
    for name in D.ASSERTED:
        err = lapack_errors(name, hessian=name in D.PD_CANDIDATES)
        for k, v in err.items():
            if np.isfinite(v).any() and float(np.nanmax(v)) > worst[k][0]:
                worst[k] = (float(np.nanmax(v)), name)
    return tuple(4 * worst[k][0] for k in ("psi", "g", "H")), tuple(worst[k][1] for k in ("psi", "g", "H"))
