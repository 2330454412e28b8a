"""Newton-PCG (DOTMI_FLAG_NEWTON_PCG, dotmi_solve_hessian; dot_amd/csrc/k_pcg.hip, dotmi_pcg.hip): the numpy restatement of the device's
conjugate-gradient recurrences -- the single-reduction form of Chronopoulos and Gear, statement for statement, with the operator and
the preconditioner as callables -- and the symmetric scaling of DOT's block solve it is preconditioned with.  TEST INFRASTRUCTURE."""
import numpy as np


def dup_of(T, epart, nV):
    """the number of subdomains of an element partition that hold a vertex (DOTTimeStepper.cpp:47-56)"""
    T, epart = np.asarray(T), np.asarray(epart)
    pairs = np.unique(np.stack([T.ravel(), np.repeat(epart, T.shape[1])], axis=1), axis=0)
    return np.bincount(pairs[:, 0], minlength=nV)


def m_sym(apply_precond, dup):
    """M_sym = D^-1/2 S D^-1/2 from DOT's block solve M = D^-1 S:  M_sym r = sqrt(dup) (.) M (r / sqrt(dup))"""
    sq = np.sqrt(np.asarray(dup, dtype=np.float64))[:, None]
    return lambda r: sq * apply_precond(r / sq)


def pcg(A, M, b, rel_tol, max_iter):
    """H u = b from u = 0.  -> (u, iterations, residuals, state): residuals[k] = |r| / |b| after k iterations (recursive),
    state 1 converged, 2 breakdown, 0 stopped at max_iter.  Per iteration
        w = M r, s = A w, gamma = r.w, delta = w.s, beta = gamma / gamma_old, alpha = gamma / (delta - beta gamma / alpha_old),
        d = w + beta d, Hd = s + beta Hd, u += alpha d, r -= alpha Hd
    with the convergence test |r|^2 <= rel_tol^2 |b|^2 in front of every iteration and behind the last."""
    b = np.asarray(b, dtype=np.float64)
    u, r = np.zeros_like(b), b.copy()
    d, Hd = np.zeros_like(b), np.zeros_like(b)
    bb = float(np.vdot(b, b))
    rr, gamma_old, alpha_old = bb, 1.0, 1.0
    res = [1.0 if bb > 0.0 else 0.0]
    tol2 = rel_tol * rel_tol * bb
    k = 0
    while True:
        if rr <= tol2:
            return u, k, res, 1
        if k >= max_iter:
            return u, k, res, 0
        w = M(r)
        s = A(w)
        gamma, delta = float(np.vdot(r, w)), float(np.vdot(w, s))
        if not (gamma > 0.0 and np.isfinite(gamma)):
            return u, k, res, 2
        beta = 0.0 if k == 0 else gamma / gamma_old
        den = delta if k == 0 else delta - beta * gamma / alpha_old
        if not (den > 0.0 and np.isfinite(den)):
            return u, k, res, 2
        alpha = gamma / den
        d = w + beta * d
        Hd = s + beta * Hd
        u = u + alpha * d
        r = r - alpha * Hd
        rr = float(np.vdot(r, r))
        gamma_old, alpha_old = gamma, alpha
        k += 1
        res.append(np.sqrt(rr / bb))
