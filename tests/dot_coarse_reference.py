"""DOT's time step with the preconditioner as a callable (dotmi_set_dot_coarse; dot_amd/csrc/dotmi_loop.hip, dotmi_devloop.hip,
k_coarse.hip): the numpy restatement.  One step is what OracleSim.step() does (oracle/dot_oracle.c: dor_step_begin, solve_one_step,
line_search, dor_step_end) with the oracle's operators -- energy, gradient, spmv, apply_precond, refactor, target_gres, set_state --
and the two-loop recursion, the step estimate, the halving and the history in numpy:
    initX:      x += dt v + dt^2 g on free vertices
    per iteration, while |g|^2 > targetGRes:
        q = -g;  for the stored pairs newest first:  xi_h = s_h . q / (y_h . s_h),  q -= xi_h y_h
        p = precond(q);  for the stored pairs oldest first:  p += s_h (xi_h - y_h . p / (y_h . s_h))
        alpha = clamp(-p.g / p.Hp, 0.1, 1);  halve while E(x + alpha p) > E(x)  (alpha == 0: the step has failed)
        the pair (alpha p, g_new - g) is stored when y . s > 0, history 5
    refactor at the final x, then the BE update through set_state.
With precond = the oracle's apply_precond this reproduces OracleSim.step() to the iteration (tests/test_dot_coarse_host.py); with
M' = M + Z A0^-1 Z^T (tests/coarse_reference.py: Z frozen at the positions of the last refresh, A0 = Z^T H Z through the same spmv)
it is the parity bar of the device's mode.  TEST INFRASTRUCTURE."""
import numpy as np

from tests import coarse_reference as CR

HIST = 5
ITER_CAP = 10000


def coarse_term(x, dup, part_verts, fixed, spmv):
    """the restatement's r -> Z A0^-1 Z^T r at the positions x on the operator spmv, or None when A0 is not positive definite;
    -> (apply or None, live)"""
    Z, cen, live, w = CR.build_z(x, dup, part_verts, fixed)
    A0 = CR.coarse_matrix(Z, live, spmv)
    return CR.coarse_apply(Z, A0), live


def direction(g, S, Y, precond, spmv, alpha_min=0.1):
    """the two-loop recursion and the step estimate from a gradient and the stored pairs (oldest first) -> (q, z, p, alpha_0)"""
    q = -np.asarray(g, dtype=np.float64)
    m = len(S)
    ys = [float(np.vdot(Y[h], S[h])) for h in range(m)]
    xi = [0.0] * m
    for h in range(m - 1, -1, -1):
        xi[h] = float(np.vdot(S[h], q)) / ys[h]
        q = q - xi[h] * Y[h]
    z = precond(q)
    p = z.copy()
    for h in range(m):
        p = p + S[h] * (xi[h] - float(np.vdot(Y[h], p)) / ys[h])
    Hp = spmv(p)
    pg, pHp = float(np.vdot(p, g)), float(np.vdot(p, Hp))
    return q, z, p, max(alpha_min, min(1.0, -pg / pHp))


class DotStepper:
    """drives an OracleSim through DOT steps with a preconditioner of the caller's.  Created when the oracle's x_n equals its x
    (after its creation or after a step): the object keeps x_n itself, which the oracle does not hand out."""

    def __init__(self, orc, fixed, dt, gravity):
        self.orc = orc
        self.fixed = np.asarray(fixed, dtype=bool)
        self.dt = float(dt)
        self.gdtsq = self.dt * self.dt * np.asarray(gravity, dtype=np.float64)
        self.xn = orc.state()[0].copy()
        self.snapshots = []

    def step(self, precond=None, keep=False, hist=HIST, iter_cap=ITER_CAP):
        """one time step -> dict(iters, halvings, status, E, g2, no_pair, log); precond: r (nV, 3) -> (nV, 3), default the oracle's
        block preconditioner.  keep: self.snapshots[k] = (x, S, Y) in front of iteration k.  hist: pairs kept; iter_cap: the step stops
        after that many iterations (status 2).  no_pair: the iterations, counted from 1, whose accepted trial stored no pair
        (y . s <= 0); log: per iteration (alpha, E, |g|^2) as arrays"""
        orc = self.orc
        M = orc.apply_precond if precond is None else precond
        x, v, _ = orc.state()
        x = x + np.where(self.fixed[:, None], 0.0, self.dt * v + self.gdtsq[None, :])
        lastE = orc.energy(x)
        g = orc.gradient(x)
        g2 = float(np.vdot(g, g))
        S, Y = [], []
        it = halvings = 0
        failed = False
        self.snapshots = []
        no_pair, log = [], []
        tol = orc.target_gres
        while True:
            if keep:
                self.snapshots.append((x.copy(), [s.copy() for s in S], [y.copy() for y in Y]))
            _, _, p, alpha = direction(g, S, Y, M, orc.spmv)
            x0 = x
            x = x0 + alpha * p
            E = orc.energy(x)
            while E > lastE and alpha > 0.0:
                alpha /= 2.0
                halvings += 1
                if alpha == 0.0:
                    failed = True
                    break
                x = x0 + alpha * p
                E = orc.energy(x)
            lastE = E
            s_new = alpha * p
            g_new = orc.gradient(x)
            y_new = g_new - g
            g = g_new
            if float(np.vdot(y_new, s_new)) > 0.0:
                if len(S) == hist:
                    S.pop(0)
                    Y.pop(0)
                S.append(s_new)
                Y.append(y_new)
            elif not failed:
                no_pair.append(it + 1)
            if failed:
                break
            g2 = float(np.vdot(g, g))
            it += 1
            log.append((alpha, E, g2))
            if it >= iter_cap or not g2 > tol:
                break
        status = 2 if (failed or it >= iter_cap) else 0
        if not failed:
            orc.refactor(x)
        v = (x - self.xn) / self.dt
        self.xn = x.copy()
        orc.set_state(x, v, x)
        return dict(iters=it, halvings=halvings, status=status, E=lastE, g2=g2, no_pair=no_pair,
                    log=tuple(np.array(c) for c in zip(*log)) if log else (np.zeros(0),) * 3)


def m_prime(orc, dup, part_verts, fixed):
    """M' = M + Z A0^-1 Z^T at the oracle's current positions and factors (call it after the refresh, before the step): the callable,
    and whether the coarse term is active"""
    apply, _ = coarse_term(orc.state()[0], dup, part_verts, fixed, orc.spmv)
    return CR.precond(orc.apply_precond, apply), apply is not None
