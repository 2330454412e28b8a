"""Newton-PCG measurements behind profiles/newton_pcg.txt (one GPU):
  python tools/pcg_measure.py solve   [workload]            per solve at 1e-8: ms, iterations, us per iteration for check_every 1, 2, 4, 8
  python tools/pcg_measure.py kernels [workload]            a few solves at check_every 4, to run under `rocprofv3 --kernel-trace --stats`
  python tools/pcg_measure.py steps   <workload> [frames] [exact]   Newton and CG iterations per step for eta 1e-2, 1e-3, 1e-6, beside
                                                            DOTMI_FLAG_NEWTON on one subdomain"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from dot_amd import lib as dl  # noqa: E402
from dot_amd.timestepper import DOTTimeStepper  # noqa: E402
from dot_amd.workloads import load_workload  # noqa: E402


def scripted(sc, ts):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)


def solve_state(name):
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n)
    for _ in range(2):
        scripted(sc, ts)
        ts.step()
    scripted(sc, ts)
    ts.updatePrecondMtrAndFactorize()
    return sc, ts, n, -ts.computeGradient(ts.getResult())


def main():
    mode = sys.argv[1]
    name = sys.argv[2] if len(sys.argv) > 2 else "bar17K_twist"
    if mode in ("solve", "kernels"):
        sc, ts, n, b = solve_state(name)
        print(f"{name}: nV {sc.V_rest.shape[0]}, {n} subdomains, two-level form {ts.backsolveForm()}")
        for every in ((4,) if mode == "kernels" else (1, 2, 4, 8)):
            ts.setPCG(1e-3, 500, every)
            u, it, res = ts.solveHessian(b, 1e-8, 500)          # warm
            reps = 5 if mode == "kernels" else 20
            t0 = time.perf_counter()
            for _ in range(reps):
                ts.solveHessian(b, 1e-8, 500)
            ms = 1e3 * (time.perf_counter() - t0) / reps
            true = np.linalg.norm(b - ts.multiply(u)) / np.linalg.norm(b)
            print(f"check_every {every}: {ms:.3f} ms per solve (host clock, the two {b.nbytes // 1024} KB copies included), {it} iterations, "
                  f"{1e3 * ms / it:.1f} us per iteration, recursive {res:.2e}, true {true:.2e}")
        bms, nb = ts.benchPrecond(20)
        print(f"block solve alone: {1e3 * bms:.1f} us for {nb / 1e6:.1f} MB")
        ts.close()
        return
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    sc, ep, n = load_workload(name)
    print(f"{name}: nV {sc.V_rest.shape[0]}, nT {sc.T.shape[0]}, {n} subdomains, {frames} frames")
    runs = [(f"PCG eta {eta:g}", dl.FLAG_NEWTON_PCG, eta) for eta in (1e-2, 1e-3, 1e-6)] + [("exact, one subdomain", dl.FLAG_NEWTON, None)]
    if len(sys.argv) > 4 and sys.argv[4] == "exact":      # (only the one-subdomain run)
        runs = runs[-1:]
    for label, flag, eta in runs:
        sc, ep, n = load_workload(name)
        if eta is None:
            ep, n = np.zeros(sc.T.shape[0], dtype=np.int32), 1
        ts = DOTTimeStepper(sc, ep, n, flags=flag, iter_cap=200)
        if eta is not None:
            ts.setPCG(eta, 500, 4)
        rows = []
        for k in range(frames):
            scripted(sc, ts)
            st = ts.step()
            rows.append((st.iters, st.ls_halvings, int(st.backsolve_launches), st.ms_total, st.ms_factor + st.ms_hessian, st.status))
            if st.status != 0:      # (the cap of 200 Newton iterations, or the line search ran out: no point in going on)
                break
        print(f"  {label}: storage {ts._L.dotmi_factor_storage_bytes(ts._h) / 1e6:.0f} MB")
        print("    Newton iterations " + " ".join(f"{r[0]:d}" for r in rows) + "  halvings " + " ".join(f"{r[1]:d}" for r in rows))
        print("    block-solve applications " + " ".join(f"{r[2]:d}" for r in rows) + "  status " + " ".join(f"{r[5]:d}" for r in rows))
        print("    ms per step " + " ".join(f"{r[3]:.2f}" for r in rows) + "  of it refresh (device) " + " ".join(f"{r[4]:.2f}" for r in rows))
        ts.close()


if __name__ == "__main__":
    main()
