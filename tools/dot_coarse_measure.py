"""The rigid-mode coarse term of DOT's block preconditioner (dotmi_set_dot_coarse): the measurements behind profiles/dot_coarse.txt
(one GPU):
  python tools/dot_coarse_measure.py steps   <workload> [frames] [reps]   DOT steps with the mode off and on, alternating fresh handles
                                                                          in one process: iterations and halvings per step, ms per
                                                                          step and us per iteration over steps 2..N, the coarse
                                                                          build beside ms_factor
  python tools/dot_coarse_measure.py kernels <workload> <mode> [frames]   the same steps with the mode 0 / 1 / 2, to run under
                                                                          `rocprofv3 --kernel-trace --stats`
  python tools/dot_coarse_measure.py balanced <workload> [frames] [reps]  `steps` with the modes 0 / 1 / 2 alternating (mode 2: the
                                                                          balanced form; profiles/dot_coarse_balanced.txt)
  python tools/dot_coarse_measure.py sharded <workload> [frames] [reps] [off]
                                                                          `steps` on one rank under DOTMI_FLAG_FORCE_DIST, without and
                                                                          with DOTMI_FLAG_DOT_COARSE (profiles/dot_coarse_sharded.txt);
                                                                          `off`: the rows without the flag only (an older library
                                                                          ignores the bit)
A library without the entries (DOTMI_LIBRARY pointing at an older build) gives the mode-off rows only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from dot_amd import lib as dl  # noqa: E402
from dot_amd.timestepper import DOTTimeStepper  # noqa: E402
from dot_amd.workloads import load_workload  # noqa: E402


def run(name, mode, frames, sharded=False):
    sc, ep, n = load_workload(name)
    print(f"  ... {name}: a handle with the coarse term {('off', 'on', 'balanced')[mode]}", file=sys.stderr, flush=True)
    ts = DOTTimeStepper(sc, ep, n, flags=(dl.FLAG_FORCE_DIST | (dl.FLAG_DOT_COARSE if mode else 0)) if sharded else 0)
    if mode and not sharded:
        ts.setDotCoarseMode(mode) if mode == 2 else ts.setDotCoarse(mode)
    rows = []
    for _ in range(frames):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        build = ts.dotCoarseInfo()[4] if mode else 0.0
        rows.append((st.iters, st.ls_halvings, st.status, st.ms_total, st.ms_loop, st.ms_hessian, st.ms_factor, build))
    info = ts.dotCoarseInfo() if mode else None
    ts.close()
    return rows, info, (sc.V_rest.shape[0], sc.T.shape[0], n)


def main():
    what, name = sys.argv[1], sys.argv[2]
    has = hasattr(dl.load(), "dotmi_set_dot_coarse")
    if what == "kernels":
        mode = int(sys.argv[3])
        frames = int(sys.argv[4]) if len(sys.argv) > 4 else 4
        rows, info, _ = run(name, mode, frames)
        print(f"{name} mode {mode}: iterations " + " ".join(str(r[0]) for r in rows) + f"  info {info}")
        return
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    sharded = what == "sharded"
    modes = (0, 1) if has and not (sharded and "off" in sys.argv[5:]) else (0,)
    if what == "balanced" and hasattr(dl.load(), "dotmi_dot_coarse_mode"):
        modes = (0, 1, 2)
    res = {m: [] for m in modes}
    for _ in range(reps):                       # off, on, off, on, ...: the two share whatever else the machine is doing
        for m in modes:
            res[m].append(run(name, m, frames, sharded))
    nV, nT, n = res[0][0][2]
    print(f"{name}{', one rank under DOTMI_FLAG_FORCE_DIST' if sharded else ''}: nV {nV}, nT {nT}, {n} subdomains, {frames} frames x {reps} "
          f"runs per mode, library {dl.LIB_PATH}")
    for m in modes:
        rows0, info, _ = res[m][0]
        same = all([r[:3] for r in rr[0]] == [r[:3] for r in rows0] for rr in res[m])
        per_step = [np.mean([r[3] for r in rr[0][1:]]) for rr in res[m]]
        loop_us = [1e3 * sum(r[4] for r in rr[0][1:]) / max(1, sum(r[0] for r in rr[0][1:])) for rr in res[m]]
        fact = np.median([r[6] for rr in res[m] for r in rr[0][1:]])
        hess = np.median([r[5] for rr in res[m] for r in rr[0][1:]])
        build = np.median([r[7] for rr in res[m] for r in rr[0][1:]])
        print(f"  coarse {('off', 'on ', 'balanced')[m]}: iterations " + " ".join(f"{r[0]}" + (f"({r[1]})" if r[1] else "") for r in rows0) +
              "  status " + " ".join(str(r[2]) for r in rows0) + ("" if same else "  (the runs differ in their counts!)"))
        print("      ms per step (steps 2..N), per run " + " ".join(f"{v:.3f}" for v in per_step) + f"  median {np.median(per_step):.3f}")
        print("      us per iteration (ms_loop / iterations, steps 2..N), per run " + " ".join(f"{v:.1f}" for v in loop_us) +
              f"  median {np.median(loop_us):.1f}")
        print(f"      refresh: ms_hessian {hess:.3f} (H and the fill), ms_factor {fact:.3f}" +
              (f", coarse build {build:.3f} ms behind it; info {info}" if m else ""))


if __name__ == "__main__":
    main()
