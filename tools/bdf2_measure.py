"""BDF2 beside backward Euler (dotmi_set_time_integration): the measurements behind profiles/bdf2.txt (one GPU):
  python tools/bdf2_measure.py ab <other libdotmi.so> [frames] [reps] [workloads]
        backward-Euler steps of this tree's library and of another build of the same ABI (the parent commit's), alternating, one fresh
        process per run (the library is chosen at import: DOTMI_LIBRARY): iterations per step, ms per step over steps 2..N; then BDF2
        at the same dt on this tree's library
  python tools/bdf2_measure.py run <workload> <be|bdf2> [frames]
        one such run; prints one JSON line
  python tools/bdf2_measure.py kernels <workload> [frames]
        `frames` backward-Euler steps, then the switch and `frames` BDF2 steps on one handle, to run under
        `rocprofv3 --kernel-trace --stats`: init_x / be_update beside bdf2_init_x / bdf2_update / bdf2_predict"""
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def run(name, bdf2, frames):
    from dot_amd import lib as dl
    from dot_amd.timestepper import DOTTimeStepper
    from dot_amd.workloads import load_workload
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n)
    if bdf2:
        ts.setTimeIntegration(dl.TIT_BDF2)
    rows = []
    for _ in range(frames):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        rows.append((st.iters, st.ls_halvings, st.status, st.ms_total))
    x = ts.getResult()
    ts.close()
    return {"workload": name, "bdf2": bool(bdf2), "library": os.path.basename(os.path.dirname(dl.LIB_PATH)) + "/" + os.path.basename(dl.LIB_PATH),
            "iters": [r[0] for r in rows], "halvings": [r[1] for r in rows], "status": [r[2] for r in rows],
            "ms": [round(r[3], 4) for r in rows], "x_sum": float(np.abs(x).sum())}


def child(name, kind, frames, library=None):
    env = dict(os.environ)
    if library:
        env["DOTMI_LIBRARY"] = library
    else:
        env.pop("DOTMI_LIBRARY", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "run", name, kind, str(frames)], env=env, capture_output=True,
                         text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def summary(r):
    ms = np.array(r["ms"][2:])
    it = sum(r["iters"][2:])
    return (f"iterations/frame {it / len(ms):6.2f}  ms/step median {np.median(ms):7.3f} (min {ms.min():7.3f} max {ms.max():7.3f})  "
            f"us/iteration {1e3 * ms.sum() / max(it, 1):7.1f}")


def main():
    what = sys.argv[1]
    if what == "run":
        print(json.dumps(run(sys.argv[2], sys.argv[3] == "bdf2", int(sys.argv[4]) if len(sys.argv) > 4 else 12)), flush=True)
        return
    if what == "kernels":
        from dot_amd import lib as dl
        from dot_amd.timestepper import DOTTimeStepper
        from dot_amd.workloads import load_workload
        name, frames = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 6
        sc, ep, n = load_workload(name)
        ts = DOTTimeStepper(sc, ep, n)
        for kind in (dl.TIT_BE, dl.TIT_BDF2):
            ts.setTimeIntegration(kind)
            its = []
            for _ in range(frames):
                idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
                ts.setDirichlet(idx, pos)
                its.append(ts.step().iters)
            print(f"{name} {'BDF2' if kind else 'backward Euler'}: iterations {its}")
        ts.close()
        return
    other = os.path.abspath(sys.argv[2])
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 22
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    names = sys.argv[5].split(",") if len(sys.argv) > 5 else ["bar17K_twist", "monkey18K_stiff"]
    for name in names:
        print(f"== {name}: {frames} frames per run, steps 2..{frames - 1} timed, {reps} alternations ==", flush=True)
        ref = None
        for rep in range(reps):
            for tag, lib in (("parent", other), ("this  ", None)):
                r = child(name, "be", frames, lib)
                ref = ref or r
                same = r["iters"] == ref["iters"] and r["halvings"] == ref["halvings"] and r["x_sum"] == ref["x_sum"]
                print(f"  backward Euler  {tag} #{rep}  {summary(r)}  iterations, halvings and sum|x| equal to the first run: {same}", flush=True)
        r = child(name, "bdf2", frames)
        print(f"  BDF2            this      {summary(r)}  status {sorted(set(r['status']))}", flush=True)
        print(f"  iterations per step  backward Euler {ref['iters']}\n                       BDF2           {r['iters']}", flush=True)


if __name__ == "__main__":
    main()
