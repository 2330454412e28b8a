"""Designed deformation states for the element kernels: small meshes of disjoint tets, one mesh per family of singular
values, F = U diag(sigma) V^T with random rotations, rest shapes cycling through the unit tet, a scaled one (edge 0.03, the
bunny's) and a skewed one (kappa(Dm) ~ 30), laid out on a 3-D grid with offsets <= 8 so that storing x does not wipe out a
sigma of 1e-6.  Deterministic (seeded).  The reference values come from tests/elem_reference.py, always from the stored
doubles, never from the designed sigma.

The three constants of the bounds are NOT tuned to the kernels: each is 4 x the largest normalised error of a plain float64
evaluation of the same closed forms on LAPACK's SVD (numpy.linalg.svd) against the 60-digit reference, over all asserted
families and both materials (`lapack_constants`, recomputed and compared by tests/test_elem_reference.py).  The factor 4
covers a different operation order and the Jacobi rotations of svd3.

  energy     |Psi_e - ref| <= K_PSI eps S_Psi                                  (mesh: summed, with the inertia scale)
  gradient   max|g_e - ref| <= K_P eps kappa_R kappa(Dm) gscale_e               (Stable Neo-Hookean: without kappa_R)
  Hessian    max|H_e - FD|  <= K_H eps kappa_R kappa(Dm)^2 max|H_FD|            (where the projection is the identity)"""
import functools

import numpy as np

from tests import elem_reference as R

K_PSI = 4 * 6.737     # wide_10, Stable Neo-Hookean
K_P = 4 * 15.60       # scale_1e-1, Fixed-Corotational (a skewed rest tet)
K_H = 4 * 16.89       # pd_c, Stable Neo-Hookean

SEED = 20240611
N_TETS = 24
YM, PR, RHO, DT = 100.0, 0.4, 1.0, 0.05
MU, LAM = YM / 2.0 / (1.0 + PR), YM * PR / (1.0 + PR) / (1.0 - 2.0 * PR)      # Mesh.cpp:741-744, as dot_amd.scene.lame
EPS = R.EPS

UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=float)
REST_SHAPES = (UNIT, 0.03 * UNIT, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5.3, 0, 1]], dtype=float))   # kappa(Dm): 1, 1, 30.1


def _two_small(r, sign):
    return (1.0, r, sign * 0.6 * r)


# name -> singular values (signed sigma_2), or ("noise", a) for F = I + a N(0,1)
FAMILIES = {
    "rest": (1, 1, 1), "scale_1e-3": (1e-3,) * 3, "scale_1e1": (10,) * 3, "scale_1e3": (1e3,) * 3,
    "two_equal_hi": (2, 2, .5), "two_equal_lo": (2, .5, .5), "gap_1e-8": (1.5, 1 + 1e-8, 1), "gap_1e-12": (1.5, 1 + 1e-12, 1),
    "small_1e-4": (1.2, .8, 1e-4), "small_1e-8": (1.2, .8, 1e-8), "small_0": (1.2, .8, 0.0), "inverted": (1.2, .8, -.5),
    "near_reflection": (1, 1, -.999), "generic": (3, .7, .2), "noise_0.5": ("noise", 0.5),
    # two singular values small against the largest: an element squashed towards a line
    "thin_1e-3": (1, 1e-3, 5e-4), "thin_2e-4_inv": (1, 2e-4, -1e-4), "thin_2e-6": (1, 2e-6, 1e-6), "thin_1e-9_rank1": (1, 1e-9, 0.0),
    "wide_30": (30, 1, 1 / 30), "wide_10": (10, 1, 1), "scale_1e-1": (.1,) * 3, "flip_sum_1e-3": (1, .5005, -.4995),
    **{f"two_small_{r:g}_{'pos' if s > 0 else 'neg'}": _two_small(r, s) for r in (1e-2, 1e-3, 1e-4, 1e-6) for s in (1, -1)},
    "noise_1e-7": ("noise", 1e-7), "noise_1e-3": ("noise", 1e-3),
    # the polar factor is not defined here: only energy and finiteness are asserted
    "flip_sum_0": (1, .5, -.5), "zero": (0.0, 0.0, 0.0),
    # states where the projection of the Hessian is the identity (screened by the reference, see pd_mask)
    "pd_a": (1.1, 1.05, 1.02), "pd_b": (1.14, 1.14, 1.01), "pd_c": (1.05,) * 3, "pd_d": (1.12, 1.08, 1.03), "pd_e": (1.15, 1.1, 1.05),
    "pd_f": (1.02, 1.01, 1.005), "pd_g": (1.077,) * 3, "pd_h": (1.25, 1, 1), "pd_i": (1.5, 1, 1 / 1.2), "pd_j": (1.1, 1.1, 1.03),
    "pd_k": (1.2, 1.1, .95), "pd_l": (1.3, 1.05, .92),
}
UNDEFINED_R = ("flip_sum_0", "zero")
PD_CANDIDATES = tuple(k for k in FAMILIES if k.startswith("pd_"))
ASSERTED = tuple(k for k in FAMILIES if k not in UNDEFINED_R)


def two_small(name):
    """sigma_1 <= 1e-2 sigma_0: the families where the CPU oracle is the inaccurate side of a comparison"""
    s = FAMILIES[name]
    return s[0] != "noise" and s[0] > 0 and abs(s[1]) <= 1e-2 * s[0]


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> V_rest (4n,3), T (n,4) int32, x (4n,3): the designed positions; tet k has rest shape REST_SHAPES[k % 3]"""
    spec = FAMILIES[name]
    rng = np.random.default_rng(SEED + list(FAMILIES).index(name))
    V, X = [], []
    for k in range(N_TETS):
        shape = REST_SHAPES[k % 3]
        off = 4.0 * np.array([k % 3, (k // 3) % 3, k // 9], dtype=float)
        if spec[0] == "noise":
            F = np.eye(3) + spec[1] * rng.standard_normal((3, 3))
        else:
            F = _rotation(rng) @ np.diag(np.array(spec, dtype=float)) @ _rotation(rng).T
        V.append(shape + off)
        X.append(shape @ F.T + off)
    T = (np.arange(4)[None, :] + 4 * np.arange(N_TETS)[:, None]).astype(np.int32)
    return np.concatenate(V), T, np.concatenate(X)


@functools.lru_cache(maxsize=None)
def reference(name, mat, hessians=False):
    """the 60-digit evaluation of family `name` (x~ = the rest positions: a handle created at rest with v = 0, no gravity)"""
    V, T, x = mesh(name)
    return R.MeshRef(V, T, MU, LAM, RHO, DT, mat).evaluate(x, V, hessians=hessians)


@functools.lru_cache(maxsize=None)
def pd_mask(name, mat):
    """per tet: every eigenvalue of the reference's 9x9 dP/dF >= 0.1 mu, so that the PSD projection is the identity and the
    1e-6 clamp of spectral_blocks is idle (chosen by the reference, not by the kernels)"""
    ref = reference(name, mat)
    mu, lam = R.mpf(MU), R.mpf(LAM)
    return np.array([np.linalg.eigvalsh(R.dPdF_fd(mat, F, mu, lam)).min() >= 0.1 * MU for F in ref["Fmp"]])


# ---- the plain float64 evaluation on LAPACK's SVD that defines the constants ---------------------------------------------
def _cof(F):
    return np.array([[F[(r + 1) % 3, (c + 1) % 3] * F[(r + 2) % 3, (c + 2) % 3] - F[(r + 1) % 3, (c + 2) % 3] * F[(r + 2) % 3, (c + 1) % 3]
                      for c in range(3)] for r in range(3)])


def lapack_svd(F):
    """numpy.linalg.svd with the conventions of the tree: U, V in SO(3), the sign of det F on the last singular value"""
    U, s, Vt = np.linalg.svd(F)
    V = Vt.T.copy()
    s = s.copy()
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]; s[2] = -s[2]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]; s[2] = -s[2]
    return U, s, V


def f64_density(mat, F, mu=MU, lam=LAM):
    """Psi and P of the closed forms of tests/elem_reference.py in float64"""
    C = _cof(F)
    J = F[0] @ C[0]
    if mat == R.FCR:
        U, s, V = lapack_svd(F)
        D = F - U @ V.T
        return mu * (D * D).sum() + lam / 2 * (J - 1) ** 2, 2 * mu * D + lam * (J - 1) * C
    a = 1 + mu / lam
    return (mu * ((F * F).sum() - 3) + lam * (J - a) ** 2) / 2, mu * F + lam * (J - a) * C


def spectral_dPdF(mat, U, s, V, mu=MU, lam=LAM, blocks=None):
    """unprojected 9x9 dP/dF (row 3i+j, column 3k+l) from the spectral formulas in float64: A = d2Psi/dsigma2 on the
    diagonal modes, [[l + r, l - r], [l - r, l + r]] on each pair of off-diagonal modes, l = (Psi_i - Psi_j) / 2 (s_i - s_j)
    in closed form, r = (Psi_i + Psi_j) / 2 (s_i + s_j).  blocks = (A (3,3), B (3,4)) overrides the coefficients (pairs
    (0,1), (1,2), (2,0); b00 b01 b10 b11): the layout of spectral_blocks in elem_math.hpp."""
    J = s[0] * s[1] * s[2]
    pn = np.array([s[1] * s[2], s[2] * s[0], s[0] * s[1]])
    if blocks is None:
        if mat == R.FCR:
            d = 2 * mu * (s - 1) + lam * (J - 1) * pn
            A = lam * np.outer(pn, pn) + 2 * mu * np.eye(3)
            left = lambda k: mu - lam / 2 * s[k] * (J - 1)
            offd = lambda k: lam * (s[k] * (J - 1) + pn[(k + 1) % 3] * pn[(k + 2) % 3])
        else:
            t = lam * (J - (1 + mu / lam))
            d = mu * s + t * pn
            A = lam * np.outer(pn, pn) + mu * np.eye(3)
            left = lambda k: (mu - t * s[k]) / 2
            offd = lambda k: s[k] * lam * (2 * J - (1 + mu / lam))
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            A[i, j] = A[j, i] = offd(k)
        B = np.empty((3, 4))
        for c in range(3):
            cp = (c + 1) % 3
            l, r = left((c + 2) % 3), (d[c] + d[cp]) / (2 * (s[c] + s[cp]))
            B[c] = l + r, l - r, l - r, l + r
    else:
        A, B = blocks
    mode = lambda i, j: np.outer(U[:, i], V[:, j]).reshape(9)
    M = np.zeros((9, 9))
    for i in range(3):
        for j in range(3):
            M += A[i, j] * np.outer(mode(i, i), mode(j, j))
    for c in range(3):
        cp = (c + 1) % 3
        e = (mode(c, cp), mode(cp, c))
        for a in range(2):
            for b in range(2):
                M += B[c, 2 * a + b] * np.outer(e[a], e[b])
    return M


def f64_element(mat, X4, x4, xt4, hessian=False):
    """one tet from the stored doubles, all in float64: dt^2 vol Psi, the 12 gradient entries with the inertia term, and the
    unprojected elastic Hessian G^T (w dP/dF) G on request"""
    Dm = (X4[1:] - X4[0]).T
    A = np.linalg.inv(Dm)
    vol = np.linalg.det(Dm) / 6
    F = (x4[1:] - x4[0]).T @ A
    w = DT * DT * vol
    psi, P = f64_density(mat, F)
    g = np.empty((4, 3))
    g[1:] = w * (A @ P.T)
    g[0] = -g[1:].sum(axis=0)
    g += RHO * abs(vol) / 4 * (x4 - xt4)
    if not hessian:
        return w * psi, g.reshape(12), None
    G = np.zeros((9, 12))                       # dF_ij / dx_kc
    for i in range(3):
        for j in range(3):
            for k in range(3):
                G[3 * i + j, 3 * (k + 1) + i] = A[k, j]
                G[3 * i + j, i] -= A[k, j]
    return w * psi, g.reshape(12), G.T @ (w * spectral_dPdF(mat, *lapack_svd(F))) @ G


def normalised_errors(name, mat, psi_w, g, H=None):
    """per-tet errors of an evaluation (psi_w (n,) or None, g (n,12), H (n,12,12) or None) against the reference, each divided
    by its bound without the constant: -> dict of (n,) arrays 'psi', 'g', 'H' (H: NaN where the projection is not idle)"""
    ref = reference(name, mat, hessians=H is not None)
    V, T, x = mesh(name)
    n = len(T)
    kR = ref["kR"] if mat == R.FCR else np.ones(n)
    out = {}
    if psi_w is not None:
        err = np.array([float(abs(R.mpf(float(psi_w[e])) - ref["psi_w"][e])) for e in range(n)])
        out["psi"] = err / (EPS * elastic_escale(name, mat))
    ge = R.g_err(np.asarray(g).reshape(4 * n, 3), ref["g"]).reshape(n, 12).max(axis=1)
    out["g"] = ge / (EPS * kR * ref["kDm"] * ref["gscale"])
    if H is not None:
        ok = pd_mask(name, mat)
        hn = np.abs(ref["H"]).reshape(n, -1).max(axis=1)
        out["H"] = np.where(ok, np.abs(H - ref["H"]).reshape(n, -1).max(axis=1) / (EPS * ref["kR"] * ref["kDm"] ** 2 * hn), np.nan)
    return out


def elastic_escale(name, mat):
    """per tet dt^2 |vol| S_Psi (the energy scale without the inertia part)"""
    V, T, _ = mesh(name)
    ref = reference(name, mat)
    vol = np.array([abs(np.linalg.det((V[t[1:]] - V[t[0]]).T)) / 6 for t in T])
    return DT * DT * vol * ref["S_Psi"]


def lapack_errors(name, mat, hessian=False):
    V, T, x = mesh(name)
    res = [f64_element(mat, V[t], x[t], V[t], hessian) for t in T]
    return normalised_errors(name, mat, np.array([r[0] for r in res]), np.array([r[1] for r in res]),
                             np.array([r[2] for r in res]) if hessian else None)


@functools.lru_cache(maxsize=None)
def lapack_constants():
    """-> (K_PSI, K_P, K_H) by their definition: 4 x the largest normalised error of the float64 / LAPACK evaluation over the
    asserted families and both materials (K_H: over the tets of the PD candidates where the projection is idle)"""
    worst = {"psi": 0.0, "g": 0.0, "H": 0.0}
    for mat in (R.FCR, R.SNH):
        for name in ASSERTED:
            err = lapack_errors(name, mat, hessian=name in PD_CANDIDATES)
            for k, v in err.items():
                if np.isfinite(v).any():
                    worst[k] = max(worst[k], float(np.nanmax(v)))
    return 4 * worst["psi"], 4 * worst["g"], 4 * worst["H"]
