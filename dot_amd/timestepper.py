"""Python-side mirror of the reference's stepper surface over the C ABI.

`DOTTimeStepper` keeps the method names main.cpp calls on `DOT::Optimizer<3>`
(src/TimeStepper/Optimizer.hpp:83-112): setRelGL2Tol, solve, getResult, getIterNum,
getInnerIterAmt, plus the kernel-level hooks.  All numerics run in libdotmi.so on the GPU.
(The C++ adapter with the same surface is dot_amd/host/DotHipTimeStepper.hpp.)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import lib as _lib
from .lib import DotmiError, Mesh, Params, StepStats, dp, ip, up
from .scene import Scene, lame


def tol_for_step(tol, k: int, default: float) -> float:
    """The relative tolerance of time step k under a script's `tol` list (src/main.cpp:108-118): entry k, beyond the list's
    end its last entry; without a list the stepper's own value."""
    if not tol:
        return default
    return tol[k] if k < len(tol) else tol[-1]


class DOTTimeStepper:
    def __init__(self, scene: Scene, epart: np.ndarray, nparts: int, energy: Optional[int] = None,
                 device: int = 0, rank: int = 0, world: int = 1, comm_id: Optional[bytes] = None,
                 history: int = 5, rel_tol: float = 1e-5, iter_cap: int = 10000, flags: int = 0, allreduce=None,
                 alpha_min: float = 0.1, vpart: Optional[np.ndarray] = None, mu: Optional[np.ndarray] = None,
                 lam: Optional[np.ndarray] = None):
        """allreduce: optional callable(np.ndarray) that sums the array over the ranks IN PLACE (world > 1): the
        library then stages its collectives through host memory and calls it instead of RCCL
        (dotmi_params::allreduce) -- e.g. a torch.distributed gloo all_reduce.
        mu, lam: optional per-element Lame parameters, shape (nT,) (dotmi_mesh::mu / ::lambda); either one left out is
        the constant that the scene's YM and PR give.
        flags: _lib.DOTMI_FLAG_NEWTON_PCG_DIST is the Newton-PCG step on sharded handles -- with world / rank and comm_id or the allreduce
        hook, or _lib.FLAG_FORCE_DIST on one rank; every rank passes it or none (it adds collectives)."""
        L = _lib.load()
        cfg = scene.cfg
        self.scene = scene
        self.nV, self.nT = scene.V_rest.shape[0], scene.T.shape[0]
        self.dt = cfg.dt
        self.rel_tol = rel_tol
        self.frameAmt = int(cfg.duration / cfg.dt)  # Optimizer::setTime, Optimizer.cpp:249-257
        self.globalIterNum = 0
        self.innerIterAmt = 0
        mu0, lam0 = lame(cfg.YM, cfg.PR)
        # keep every array alive for the lifetime of the handle
        self._X = np.ascontiguousarray(scene.V_rest, dtype=np.float64)
        self._T = np.ascontiguousarray(scene.T, dtype=np.int32)
        self._mu = self._per_element(mu, mu0, "mu")
        self._lam = self._per_element(lam, lam0, "lam")
        self._fixed = np.ascontiguousarray(scene.fixed, dtype=np.uint8)
        # (epart None: no element partition -- an LBFGS-PD or LBFGS-HI handle, _lib.FLAG_LBFGS_PD / _HI, builds no subdomains)
        self._epart = np.ascontiguousarray(epart, dtype=np.int32) if epart is not None else None
        self.nparts = int(nparts)
        self._vpart = np.ascontiguousarray(vpart, dtype=np.int32) if vpart is not None else None
        m = Mesh(self.nV, self.nT, dp(self._X), ip(self._T), dp(self._mu), dp(self._lam), cfg.rho,
                 up(self._fixed), ip(self._epart) if epart is not None else None, self.nparts, ip(self._vpart) if vpart is not None else None)
        p = Params()
        p.energy = cfg.energy_id if energy is None else energy
        p.dt = cfg.dt
        p.gravity[0], p.gravity[1], p.gravity[2] = 0.0, (-9.80665 if cfg.with_gravity else 0.0), 0.0
        p.relTol = rel_tol
        p.history = history
        p.iterCap = iter_cap
        p.alphaMin = alpha_min   # 0.1 = DOT's clamp (Optimizer.cpp:1085); 1.0 = the unit first step of LBFGS-H (:1088)
        p.device = device
        p.rank, p.world = rank, world
        self._comm = C.create_string_buffer(comm_id, 128) if comm_id is not None else None
        p.comm_id = C.cast(self._comm, C.c_void_p) if self._comm is not None else None
        p.flags = flags
        self._arcb = None
        self._ar_error = None
        if allreduce is not None:
            def _cb(ctx, buf, n, _f=allreduce):
                # an exception cannot cross the C frame: ctypes would print and swallow it and the library would carry
                # on with this rank's un-reduced partial sums.  Record it, poison the payload (NaN spreads through
                # every later sum, so the step fails its convergence test on this rank) and re-raise from _check.
                a = np.ctypeslib.as_array(buf, shape=(n,))
                try:
                    if self._ar_error is None:
                        _f(a)
                    else:
                        a[:] = np.nan
                except BaseException as e:   # noqa: BLE001 - must not propagate into the C caller
                    self._ar_error = e
                    a[:] = np.nan
            self._arcb = _lib.ALLREDUCE_CB(_cb)          # kept alive with the handle
            p.allreduce = C.cast(self._arcb, C.c_void_p)
        x0 = np.ascontiguousarray(scene.x0, dtype=np.float64)
        h = C.c_void_p()
        rc = L.dotmi_create(C.byref(m), C.byref(p), dp(x0), C.byref(h))
        if rc != 0:
            raise DotmiError(f"dotmi_create failed ({rc}): {L.dotmi_last_error(None).decode()}")
        self._h = h
        self._L = L
        self.last_stats: Optional[StepStats] = None
        if cfg.bdf2:
            self.setTimeIntegration(_lib.TIT_BDF2)

    def _per_element(self, a, const, name):
        if a is None and const is None:
            raise ValueError(f"{name} must be given")
        if a is None:
            return np.full(self.nT, const, dtype=np.float64)
        a = np.array(a, dtype=np.float64)   # a private copy, kept alive with the handle
        if a.shape != (self.nT,):
            raise ValueError(f"{name} must have shape ({self.nT},), got {a.shape}")
        return a

    # ---- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.dotmi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if getattr(self, "_ar_error", None) is not None:
            e, self._ar_error = self._ar_error, None
            raise DotmiError(f"{what}: the all-reduce hook raised {type(e).__name__}: {e}") from e
        if rc < 0:
            raise DotmiError(f"{what} failed ({rc}): {self._L.dotmi_last_error(self._h).decode()}")
        return rc

    # ---- Optimizer surface ----------------------------------------------------------------------
    @property
    def targetGRes(self) -> float:
        return self._L.dotmi_target_gres(self._h)

    def getIterNum(self) -> int:
        return self.globalIterNum

    def getInnerIterAmt(self) -> int:
        return self.innerIterAmt

    def getResult(self) -> np.ndarray:
        """result.V (nV,3)"""
        x = np.empty((self.nV, 3))
        self._check(self._L.dotmi_get_state(self._h, dp(x), None, None), "get_state")
        return x

    def getState(self):
        x, v, xt = (np.empty((self.nV, 3)) for _ in range(3))
        self._check(self._L.dotmi_get_state(self._h, dp(x), dp(v), dp(xt)), "get_state")
        return x, v, xt

    def setState(self, x, v, xn=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        v = np.ascontiguousarray(v, dtype=np.float64)
        xn_ = np.ascontiguousarray(xn, dtype=np.float64) if xn is not None else None
        self._check(self._L.dotmi_set_state(self._h, dp(x), dp(v), dp(xn_) if xn_ is not None else None),
                    "set_state")

    def setDirichlet(self, idx, pos):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        self._check(self._L.dotmi_set_dirichlet(self._h, idx.size, ip(idx), dp(pos)), "set_dirichlet")

    def refix(self, fixed):
        """fixed set changed: DOTTimeStepper::updatePrecondMtrAndFactorize (DOTTimeStepper.cpp:185-270)"""
        self._fixed = np.ascontiguousarray(fixed, dtype=np.uint8)
        self._check(self._L.dotmi_refix(self._h, up(self._fixed)), "refix")

    # ---- tolerance, time step and materials of the live handle (include/dotmi.h) -----------------
    def setRelGL2Tol(self, relTol: float = 1e-5):
        """Optimizer::setRelGL2Tol (Optimizer.cpp:222-228): the next step's tolerance"""
        self._check(self._L.dotmi_set_rel_tol(self._h, relTol), "set_rel_tol")
        self.rel_tol = relTol

    def setTime(self, duration: float, dt: float):
        """Optimizer::setTime (Optimizer.cpp:249-257): dt with x~, the tolerance and the factors built with it; frameAmt"""
        self._check(self._L.dotmi_set_time_step(self._h, dt), "set_time_step")
        self.dt = dt
        self.frameAmt = int(duration / dt)

    def setTimeIntegration(self, kind: int):
        """_lib.TIT_BE or _lib.TIT_BDF2 for the next steps (dotmi_set_time_integration; Config::timeIntegrationType, whose enum has
        TIT_BE alone in the reference).  A switch to BDF2 starts with a backward-Euler step; so does setState under BDF2."""
        self._check(self._L.dotmi_set_time_integration(self._h, kind), "set_time_integration")

    def timeIntegration(self) -> int:
        return int(self._L.dotmi_time_integration(self._h))

    def timeIntegrationInfo(self):
        """(kind, levels: 1 when level n-1 exists, else the next step is a start step; the effective step dt_e the next step's launches
        take; the size of the step between the two levels, 0 without) (dotmi_time_integration_info)"""
        k, lv, de, dp_ = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        self._check(self._L.dotmi_time_integration_info(self._h, C.cast(C.byref(k), _lib.c_ip), C.cast(C.byref(lv), _lib.c_ip),
                                                        C.cast(C.byref(de), _lib.c_dp), C.cast(C.byref(dp_), _lib.c_dp)),
                    "time_integration_info")
        return k.value, lv.value, de.value, dp_.value

    def getHistory(self):
        """BDF2's level n-1: (x_prev (nV,3), v_prev (nV,3), dt_prev), or None while there is none (dotmi_get_history)"""
        xp, vp = np.empty((self.nV, 3)), np.empty((self.nV, 3))
        dtp = C.c_double()
        n = self._check(self._L.dotmi_get_history(self._h, dp(xp), dp(vp), C.cast(C.byref(dtp), _lib.c_dp)), "get_history")
        return (xp, vp, dtp.value) if n else None

    def setHistory(self, x_prev, v_prev, dt_prev: float):
        """level n-1 of a BDF2 handle after setState: the next step is a BDF2 step, not a start step (dotmi_set_history)"""
        xp = np.ascontiguousarray(x_prev, dtype=np.float64)
        vp = np.ascontiguousarray(v_prev, dtype=np.float64)
        self._check(self._L.dotmi_set_history(self._h, dp(xp), dp(vp), dt_prev), "set_history")

    def setLame(self, mu, lam):
        """per-element Lame parameters, shape (nT,) each (dotmi_set_lame); the factors are refreshed at the current positions"""
        mu = self._per_element(mu, None, "mu")
        lam = self._per_element(lam, None, "lam")
        self._check(self._L.dotmi_set_lame(self._h, dp(mu), dp(lam)), "set_lame")
        self._mu, self._lam = mu, lam

    def solve(self, maxIter: int = 1) -> int:
        """Optimizer::solve (Optimizer.cpp:327-368): script move, one time step (BE, or BDF2 after setTimeIntegration). 0 stepped, 1 all frames
        done, 2 stepped but hit the iteration cap / line-search failure."""
        flag = 0
        for _ in range(maxIter):
            x = self.getResult()
            idx, pos = self.scene.scripter.step(x, self.dt)
            if idx.size:
                self.setDirichlet(idx, pos)
            if getattr(self.scene.scripter, "changed", False):
                self.refix(self.scene.scripter.fixed)      # updatePrecondMtrAndFactorize
            if self.globalIterNum >= self.frameAmt:
                self.globalIterNum += 1
                return 1
            tol = self.scene.cfg.tol
            if tol:                                        # the script's tolerance schedule (main.cpp:108-118)
                t = tol_for_step(tol, self.globalIterNum, self.rel_tol)
                if t != self.rel_tol:
                    self.setRelGL2Tol(t)
            st = self.step()
            if st.status == 2:
                flag = 2
            self.globalIterNum += 1
        return flag

    def step(self) -> StepStats:
        """fullyImplicit + BE update without the script move."""
        st = StepStats()
        self._check(self._L.dotmi_step(self._h, C.byref(st)), "step")
        self.innerIterAmt += st.iters
        self.last_stats = st
        return st

    def iterLog(self):
        cap = 10001
        a, e, g = (np.zeros(cap) for _ in range(3))
        n = self._L.dotmi_last_iter_log(self._h, cap, dp(a), dp(e), dp(g))
        return a[:n], e[:n], g[:n]

    # ---- kernel-level hooks ---------------------------------------------------------------------
    def computeEnergyVal(self, x) -> float:
        x = np.ascontiguousarray(x, dtype=np.float64)
        E = C.c_double()
        self._check(self._L.dotmi_eval_energy(self._h, dp(x), C.cast(C.byref(E), _lib.c_dp)), "eval_energy")
        return E.value

    def computeGradient(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        g = np.empty((self.nV, 3))
        self._check(self._L.dotmi_eval_gradient(self._h, dp(x), dp(g)), "eval_gradient")
        return g

    def computeElemHessians(self, x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        H = np.empty((self.nT, 12, 12))
        self._check(self._L.dotmi_eval_elem_hessians(self._h, dp(x), dp(H)), "eval_elem_hessians")
        return H

    def updatePrecondMtrAndFactorize(self, x=None):
        xp = dp(np.ascontiguousarray(x, dtype=np.float64)) if x is not None else None
        self._check(self._L.dotmi_refactor(self._h, xp), "refactor")

    def applyPrecond(self, r) -> np.ndarray:
        r = np.ascontiguousarray(r, dtype=np.float64)
        p = np.empty((self.nV, 3))
        self._check(self._L.dotmi_apply_precond(self._h, dp(r), dp(p)), "apply_precond")
        return p

    def probeDirection(self, x, S=None, Y=None):
        """one solve_oneStep up to its first trial from a given iterate + history -> dict(g, q, z, p, alpha0, E)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        m = 0 if S is None else len(S)
        Sa = np.ascontiguousarray(S, dtype=np.float64).reshape(m, -1) if m else None
        Ya = np.ascontiguousarray(Y, dtype=np.float64).reshape(m, -1) if m else None
        out = {k: np.empty((self.nV, 3)) for k in ("g", "q", "z", "p")}
        a0, E = C.c_double(), C.c_double()
        self._check(self._L.dotmi_probe_direction(
            self._h, dp(x), m, dp(Sa) if m else None, dp(Ya) if m else None, dp(out["g"]), dp(out["q"]),
            dp(out["z"]), dp(out["p"]), C.cast(C.byref(a0), _lib.c_dp), C.cast(C.byref(E), _lib.c_dp)),
            "probe_direction")
        out["alpha0"], out["E"] = a0.value, E.value
        return out

    def icInfo(self):
        """LBFGS-HI (_lib.FLAG_LBFGS_HI): (colours, shift, attempts) of the last incomplete factorisation (dotmi_ic_info)"""
        nc, sh, na = C.c_int32(), C.c_double(), C.c_int32()
        self._check(self._L.dotmi_ic_info(self._h, C.cast(C.byref(nc), _lib.c_ip), C.cast(C.byref(sh), _lib.c_dp),
                                          C.cast(C.byref(na), _lib.c_ip)), "ic_info")
        return nc.value, sh.value, na.value

    def icFactor(self) -> np.ndarray:
        """LBFGS-HI: the factor's blocks (nL + nV, 3, 3) in plan order, lower blocks then diagonals (dotmi_ic_factor)"""
        nb = self._check(self._L.dotmi_ic_factor(self._h, 0, None), "ic_factor")
        F = np.empty((nb, 3, 3))
        self._check(self._L.dotmi_ic_factor(self._h, nb, dp(F)), "ic_factor")
        return F

    def solveHessian(self, b, rel_tol: float = 1e-8, max_iter: int = 500):
        """H u = b with the handle's current projected Hessian by conjugate gradients on the subdomain factors (dotmi_solve_hessian)
        -> (u (nV,3), iterations, |r|/|b|).  self.last_solve_status is the call's return value: 0 converged, 2 stopped at max_iter
        or broke down (u is then the last iterate).  On world > 1 every rank calls it together with the same b."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        u = np.empty((self.nV, 3))
        it, res = C.c_int32(), C.c_double()
        rc = self._check(self._L.dotmi_solve_hessian(self._h, dp(b), dp(u), rel_tol, max_iter, C.cast(C.byref(it), _lib.c_ip),
                                                     C.cast(C.byref(res), _lib.c_dp)), "solve_hessian")
        self.last_solve_status = rc
        return u, it.value, res.value

    def setPCG(self, rel_tol: float = 1e-3, max_iter: int = 500, check_every: int = 8):
        """the solves of a _lib.FLAG_NEWTON_PCG / _NEWTON_PCG_DIST step: forcing term, iteration cap; iterations between two read-backs (dotmi_set_pcg)"""
        self._check(self._L.dotmi_set_pcg(self._h, rel_tol, max_iter, check_every), "set_pcg")

    def pcgInfo(self):
        """(solves, iterations of all solves, iterations and |r|/|b| of the last one) since create (dotmi_pcg_info)"""
        ns, ni, li, lr = C.c_int64(), C.c_int64(), C.c_int32(), C.c_double()
        self._check(self._L.dotmi_pcg_info(self._h, C.byref(ns), C.byref(ni), C.cast(C.byref(li), _lib.c_ip),
                                           C.cast(C.byref(lr), _lib.c_dp)), "pcg_info")
        return ns.value, ni.value, li.value, lr.value

    def setPCGCoarse(self, mode: int = 1):
        """the rigid-mode coarse term of the PCG's preconditioner, M = M_sym + Z A0^-1 Z^T: 0 off (the default), 1 on
        (dotmi_set_pcg_coarse).  A0 is rebuilt by the first solve after every refresh of H."""
        self._check(self._L.dotmi_set_pcg_coarse(self._h, mode), "set_pcg_coarse")

    def pcgCoarseInfo(self):
        """(dimension 6 nParts, subdomains the last build dropped, active, builds since create) (dotmi_pcg_coarse_info)"""
        dim, dr, ac, nb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._L.dotmi_pcg_coarse_info(self._h, C.cast(C.byref(dim), _lib.c_ip), C.cast(C.byref(dr), _lib.c_ip),
                                                  C.cast(C.byref(ac), _lib.c_ip), C.byref(nb)), "pcg_coarse_info")
        return dim.value, dr.value, ac.value, nb.value

    def pcgCoarseMatrix(self) -> np.ndarray:
        """the last assembled coarse matrix A0 = Z^T H Z, dense (6 nParts, 6 nParts) (dotmi_pcg_coarse_matrix)"""
        nc = self._check(self._L.dotmi_pcg_coarse_matrix(self._h, 0, None), "pcg_coarse_matrix")
        A0 = np.empty((nc, nc))
        self._check(self._L.dotmi_pcg_coarse_matrix(self._h, nc * nc, dp(A0)), "pcg_coarse_matrix")
        return A0

    def pcgApplyPrecond(self, r) -> np.ndarray:
        """one application of the PCG's preconditioner as the solve uses it: M_sym r, plus the coarse term when it is active
        (dotmi_pcg_apply_precond)"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        w = np.empty((self.nV, 3))
        self._check(self._L.dotmi_pcg_apply_precond(self._h, dp(r), dp(w)), "pcg_apply_precond")
        return w

    def setDotCoarse(self, mode: int = 1):
        """the rigid-mode coarse term in DOT's own block preconditioner, M' = M + Z A0^-1 Z^T: 0 off (the default), 1 on
        (dotmi_set_dot_coarse).  step(), applyPrecond() and probeDirection() then use M'; A0 is built behind every refresh of H."""
        self._check(self._L.dotmi_set_dot_coarse(self._h, mode), "set_dot_coarse")

    def setDotCoarseMode(self, mode: int):
        """the same term by mode: 0 off, 1 additive (as setDotCoarse(1)), 2 balanced, M'' = C + (I - C H) M (I - H C) with
        C = Z A0^-1 Z^T (dotmi_set_dot_coarse_mode).  In mode 2 W = H Z is rebuilt with A0 behind every refresh of H."""
        self._check(self._L.dotmi_set_dot_coarse_mode(self._h, mode), "set_dot_coarse_mode")

    def dotCoarseMode(self) -> int:
        """0, 1 or 2: what setDotCoarse / setDotCoarseMode (or FLAG_DOT_COARSE) has left on the handle (dotmi_dot_coarse_mode)"""
        return int(self._L.dotmi_dot_coarse_mode(self._h))

    def dotCoarseInfo(self):
        """(dimension 6 nParts, subdomains the last build dropped, active, coarse builds since create, ms of the last build)
        (dotmi_dot_coarse_info)"""
        dim, dr, ac, nb, ms = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
        self._check(self._L.dotmi_dot_coarse_info(self._h, C.cast(C.byref(dim), _lib.c_ip), C.cast(C.byref(dr), _lib.c_ip),
                                                  C.cast(C.byref(ac), _lib.c_ip), C.byref(nb), C.cast(C.byref(ms), _lib.c_dp)),
                    "dot_coarse_info")
        return dim.value, dr.value, ac.value, nb.value, ms.value

    def multiply(self, p) -> np.ndarray:
        p = np.ascontiguousarray(p, dtype=np.float64)
        out = np.empty((self.nV, 3))
        self._check(self._L.dotmi_spmv(self._h, dp(p), dp(out)), "spmv")
        return out

    def features(self):
        A = np.empty((self.nT, 9)); vol = np.empty(self.nT); mass = np.empty(self.nV)
        self._check(self._L.dotmi_get_features(self._h, dp(A), dp(vol), dp(mass)), "get_features")
        return A, vol, mass

    def partMatrix(self, part: int, inverse: bool = False):
        n = self._L.dotmi_part_size(self._h, part)
        M = np.empty((n, n))
        l2g = np.empty(n // 3, dtype=np.int32)
        self._check(self._L.dotmi_part_matrix(self._h, part, int(inverse), dp(M), ip(l2g)), "part_matrix")
        return M, l2g

    def backsolveForm(self) -> int:
        """0: explicit inverse in one pass; 1: two-level form (dotmi_backsolve_form)"""
        return int(self._L.dotmi_backsolve_form(self._h))

    def loopForms(self) -> int:
        """which forms of its kernels this handle's loop launches, as a bit mask (dotmi_loop_forms): 1 / 2 / 4 = the vertex gather, the
        early merge and the direction kernel in their wide form (by size, or forced with DOTMI_WIDE_FORMS); 8 = split merge; bits
        16-17 = the two-level backward kernel's width (0 none, 1 / 2 / 3 = 32 / 64 / 128)"""
        return int(self._L.dotmi_loop_forms(self._h))

    def benchPrecond(self, reps: int = 50):
        ms = C.c_double(); nb = C.c_int64()
        self._check(self._L.dotmi_bench_precond(self._h, reps, C.cast(C.byref(ms), _lib.c_dp), C.byref(nb)),
                    "bench_precond")
        return ms.value, nb.value

    def benchEnergy(self, reps: int = 50):
        ms = C.c_double(); nb = C.c_int64()
        self._check(self._L.dotmi_bench_energy(self._h, reps, C.cast(C.byref(ms), _lib.c_dp), C.byref(nb)),
                    "bench_energy")
        return ms.value, nb.value


def comm_unique_id() -> bytes:
    L = _lib.load()
    buf = C.create_string_buffer(128)
    rc = L.dotmi_comm_unique_id(buf)
    if rc != 0:
        raise DotmiError("dotmi_comm_unique_id failed")
    return buf.raw
