"""The rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse): the measurements behind
profiles/newton_pcg_coarse.txt (one GPU), with the scripts and frames of tools/pcg_measure.py:
  python tools/pcg_coarse_measure.py steps   <workload> [frames]   Newton-PCG steps at eta 1e-3 with the mode off and on: CG iterations
                                                                   and ms per step, the refresh beside them
  python tools/pcg_coarse_measure.py solve   <workload>            one solve at 1e-3 and 1e-8, off and on: ms, iterations, us per
                                                                   iteration; ms per coarse build (host clock, against an application
                                                                   that builds nothing)
  python tools/pcg_coarse_measure.py kernels <workload> [mode]     a few solves at check_every 4 with the mode 0 / 1, to run under
                                                                   `rocprofv3 --kernel-trace --stats`
A library without the entries (DOTMI_LIBRARY pointing at an older build) gives the mode-off rows only."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from dot_amd import lib as dl  # noqa: E402
from dot_amd.timestepper import DOTTimeStepper  # noqa: E402
from dot_amd.workloads import load_workload  # noqa: E402
from tools.pcg_measure import scripted, solve_state  # noqa: E402


def main():
    what, name = sys.argv[1], sys.argv[2]
    has = hasattr(dl.load(), "dotmi_set_pcg_coarse")
    modes = (0, 1) if has else (0,)
    if what == "steps":
        frames = int(sys.argv[3]) if len(sys.argv) > 3 else 5
        sc, ep, n = load_workload(name)
        print(f"{name}: nV {sc.V_rest.shape[0]}, nT {sc.T.shape[0]}, {n} subdomains, {frames} frames, eta 1e-3, check_every 4, "
              f"library {os.path.basename(dl.LIB_PATH)}")
        for mode in modes:
            sc, ep, n = load_workload(name)
            ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_NEWTON_PCG, iter_cap=200)
            ts.setPCG(1e-3, 500, 4)
            if mode:
                ts.setPCGCoarse(1)
            rows = []
            for k in range(frames):
                scripted(sc, ts)
                st = ts.step()
                rows.append((st.iters, st.ls_halvings, int(st.backsolve_launches), st.ms_total, st.ms_factor + st.ms_hessian, st.status))
                if st.status != 0:
                    break
            print(f"  coarse {'on ' if mode else 'off'}: Newton " + " ".join(f"{r[0]:d}" for r in rows) + "  halvings " +
                  " ".join(f"{r[1]:d}" for r in rows) + "  CG iterations " + " ".join(f"{r[2]:d}" for r in rows) + "  status " +
                  " ".join(f"{r[5]:d}" for r in rows))
            print("      ms per step " + " ".join(f"{r[3]:.2f}" for r in rows) + "  of it refresh (device) " +
                  " ".join(f"{r[4]:.2f}" for r in rows) + (f"  coarse info {ts.pcgCoarseInfo()}" if mode else ""))
            ts.close()
        return
    sc, ts, n, b = solve_state(name)
    print(f"{name}: nV {sc.V_rest.shape[0]}, {n} subdomains, two-level form {ts.backsolveForm()}, library {os.path.basename(dl.LIB_PATH)}")
    if what == "kernels":
        mode = int(sys.argv[3]) if len(sys.argv) > 3 else 1
        ts.setPCG(1e-3, 500, 4)
        if mode:
            ts.setPCGCoarse(1)
        tot = 0
        for _ in range(6):
            ts.updatePrecondMtrAndFactorize()                  # (a refresh in front of every solve: six coarse builds in the trace)
            u, it, res = ts.solveHessian(b, 1e-8, 500)
            tot += it
        print(f"mode {mode}: 6 solves at 1e-8, {tot} iterations")
        ts.close()
        return
    for tol in (1e-3, 1e-8):
        for mode in modes:
            if has:
                ts.setPCGCoarse(mode)
            ts.setPCG(1e-3, 500, 8)
            u, it, res = ts.solveHessian(b, tol, 500)          # warm (and the build)
            reps = 20
            t0 = time.perf_counter()
            for _ in range(reps):
                ts.solveHessian(b, tol, 500)
            ms = 1e3 * (time.perf_counter() - t0) / reps
            true = np.linalg.norm(b - ts.multiply(u)) / np.linalg.norm(b)
            print(f"  rel_tol {tol:g} coarse {'on ' if mode else 'off'}: {ms:.3f} ms per solve (host clock, the two {b.nbytes // 1024} KB copies "
                  f"included), {it} iterations, {1e3 * ms / it:.1f} us per iteration, recursive {res:.2e}, true {true:.2e}")
    if has:
        ts.setPCGCoarse(1)
        r = np.random.default_rng(0).standard_normal(b.shape)
        ts.pcgApplyPrecond(r)
        tb = ta = tf = 0.0
        reps = 10
        for _ in range(reps):
            t0 = time.perf_counter()
            ts.updatePrecondMtrAndFactorize()
            t1 = time.perf_counter()
            ts.pcgApplyPrecond(r)                               # stale: builds
            t2 = time.perf_counter()
            ts.pcgApplyPrecond(r)                               # builds nothing
            t3 = time.perf_counter()
            tf, tb, ta = tf + t1 - t0, tb + t2 - t1, ta + t3 - t2
        print(f"  refresh of H and the subdomain factors {1e3 * tf / reps:.3f} ms; one application with a coarse build {1e3 * tb / reps:.3f} ms, "
              f"without {1e3 * ta / reps:.3f} ms: {1e3 * (tb - ta) / reps:.3f} ms per coarse build (host clock); info {ts.pcgCoarseInfo()}")
    ts.close()


if __name__ == "__main__":
    main()
