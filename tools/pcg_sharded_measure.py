"""The cost of the sharded Newton-PCG's structure on one rank of one box, behind profiles/newton_pcg_sharded.txt:
  python tools/pcg_sharded_measure.py [--parent-lib <libdotmi.so of the parent commit>] [--reps R] [frames] [workloads ...]
Per workload, every configuration in a process of its own (the library and the sharding mode are fixed when it starts):
  parent   DOTMI_FLAG_NEWTON_PCG on the parent commit's library (only with --parent-lib)
  plain    DOTMI_FLAG_NEWTON_PCG on this library: the flag off -- the parent's iterations, its time within noise
  repl     DOTMI_FLAG_NEWTON_PCG_DIST | FORCE_DIST, DOTMI_SHARD_ELEMS=0: replicated Hessian, one collective of n doubles per CG iteration
  rows     the same with DOTMI_SHARD_ELEMS=1 DOTMI_SHARD_HESS=1: sharded Hessian rows, a second collective of n + 2 doubles
The collectives are RCCL's on a communicator of one rank: what is measured is the cost of the structure (launches, packets,
staging kernels), not of any link.  --reps R runs the set of configurations R times, alternating, and prints the spread.
  python tools/pcg_sharded_measure.py run <workload> <frames> <config>      one configuration (what the first form starts)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"parent": ("NEWTON_PCG", None), "plain": ("NEWTON_PCG", None), "repl": ("DIST", ("0", "0")), "rows": ("DIST", ("1", "1"))}


def run(name, frames, config):
    from dot_amd import lib as dl
    from dot_amd.timestepper import DOTTimeStepper
    from dot_amd.workloads import load_workload
    sc, ep, n = load_workload(name)
    flags = dl.FLAG_NEWTON_PCG if CONFIGS[config][0] == "NEWTON_PCG" else (dl.DOTMI_FLAG_NEWTON_PCG_DIST | dl.FLAG_FORCE_DIST)
    ts = DOTTimeStepper(sc, ep, n, flags=flags, iter_cap=200)
    rows = []
    for _ in range(frames):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        rows.append(dict(newton=st.iters, halvings=st.ls_halvings, cg=int(st.backsolve_launches), ms=st.ms_total, ms_loop=st.ms_loop,
                         ms_refresh=st.ms_hessian + st.ms_factor, calls=int(st.collective_calls), bytes=int(st.collective_bytes),
                         status=st.status))
    ts.close()
    print("RESULT " + json.dumps(dict(nV=int(sc.V_rest.shape[0]), nT=int(sc.T.shape[0]), parts=int(n), rows=rows)))


def main():
    args = sys.argv[1:]
    if args and args[0] == "run":
        return run(args[1], int(args[2]), args[3])
    parent, reps = None, 1
    while args and args[0] in ("--parent-lib", "--reps"):
        if args[0] == "--parent-lib":
            parent = os.path.abspath(args[1])
        else:
            reps = int(args[1])
        args = args[2:]
    frames = int(args[0]) if args else 5
    names = args[1:] or ["bar17K_twist", "monkey18K_stiff"]
    configs = (["parent"] if parent else []) + ["plain", "repl", "rows"]
    for name in names:
        seen = {c: [] for c in configs}
        for rep in range(reps):
            for config in configs:
                env = dict(os.environ)
                if config == "parent":
                    env["DOTMI_LIBRARY"] = parent
                if CONFIGS[config][1]:
                    env["DOTMI_SHARD_ELEMS"], env["DOTMI_SHARD_HESS"] = CONFIGS[config][1]
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "run", name, str(frames), config], env=env,
                                     capture_output=True, text=True, timeout=600)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
                if out.returncode != 0 or not line:
                    print(f"{name} {config}: failed ({out.returncode})\n{out.stderr[-2000:]}")
                    return 1
                r = json.loads(line[0][7:])
                rows = r["rows"]
                if config == configs[0]:
                    print(f"{name}: nV {r['nV']}, nT {r['nT']}, {r['parts']} subdomains, {frames} frames, repetition {rep + 1} of {reps}")
                cg, loop = sum(x["cg"] for x in rows[1:]), sum(x["ms_loop"] - x["ms_refresh"] for x in rows[1:])
                us, ms = 1e3 * loop / max(cg, 1), sum(x["ms"] for x in rows[1:]) / max(len(rows) - 1, 1)
                seen[config].append((us, ms))
                print(f"  {config:6s} Newton " + " ".join(str(x["newton"]) for x in rows) + " | CG " + " ".join(str(x["cg"]) for x in rows) +
                      " | ms per step " + " ".join(f"{x['ms']:.2f}" for x in rows) + " | collectives per step " +
                      " ".join(str(x["calls"]) for x in rows) + f" | {us:.1f} us per CG iteration (loop less refresh, frames 2-{frames}), "
                      f"{ms:.2f} ms per step (frames 2-{frames})")
        if reps > 1:
            for config in configs:
                us, ms = [v[0] for v in seen[config]], [v[1] for v in seen[config]]
                print(f"  {config:6s} over {reps} repetitions: {min(us):.1f} - {max(us):.1f} us per CG iteration, {min(ms):.2f} - {max(ms):.2f} ms per step")
    return 0


if __name__ == "__main__":
    sys.exit(main())
