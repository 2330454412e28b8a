#!/usr/bin/env python
"""bench.py -- ms/time-step (and L-BFGS iterations/frame) of the DOT hot path on N MI355X.

A "step" = one backward-Euler time step of the workload: scripted handle move + dotmi_step
(L-BFGS-H solve to the reference's tolerance + Hessian refresh + subdomain refactorisation).
State, mesh, Hessians and factors are resident in HBM before the timed region starts; per step the
host hands over only the scripted handle positions (~24 KB) and reads back a few hundred bytes of
reduction partials per line-search trial.

    python bench.py --gpus 1 --steps 20 --warmup 3 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the
steps and prints the line; besides the contract's keys it carries what the timed steps themselves report:
  roofline      the dominant hand-written kernel pair (subdomain back-solve), algorithmic bytes /
                measured HIP-event time on the library's stream, against 8 TB/s
`--dump-outputs DIR` writes the state the last timed step left (positions, velocities) and its energy / gradient
norm / iterations as DIR/<name>.npy (float64).
`--full` adds everything that takes runs of its own and writes bench_detail.json:
  workloads     short runs of the other configurations (--extra-workloads)
  roofline_by_kernel  every kernel class launched back to back on the resident state (dotmi_bench_kernel)
  cpu_baseline  the CPU oracle (a port of the reference algorithm, oracle/dot_oracle.c) timed on the
                host cores of this box on a bounded sample of the same workload -- headline leg: with the
                reference's own CHOLMODSolver (oracle/_ref) doing the subdomain factorisations and solves;
                variant: the port's own envelope Cholesky (--no-cpu-baseline leaves it out)

`python bench.py --gpus N` with N > 1 and no launcher starts its N ranks itself (torch.distributed.run on
127.0.0.1); it refuses to run when the box has fewer GPUs, and n_gpus is checked against ncclCommCount.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DEFAULT_WORKLOAD = "bar17K_twist"  # BASELINE.json configs[1]
# also reported (short runs, every N) in the `workloads` array of the JSON line: BASELINE.json configs[0] (north_star names
# it next to bar17K_twist), configs[2] (the horse: horse7K red-refined once, 249 k tets, as the stand-in for the 136K mesh
# the reference checkout lacks), configs[3] (stiff monkey, 64 subdomains) and configs[4], the 1 M-tet bar whose 4.5 GB of
# factors cannot sit in the 256 MB Infinity Cache -- the three BASELINE.json assigns to 4 / 8 GPUs
EXTRA_WORKLOADS = "bunny5K_LTSS,horse7K_stretch@r1:64,monkey18K_stiff,synbar:140x35x35:256"
EXTRA_STEPS = {"bunny5K_LTSS": (12, 2), "horse7K_stretch@r1:64": (8, 2), "monkey18K_stiff": (5, 1),
               "synbar:140x35x35:256": (6, 2)}   # (steps, warmup)
# the reference's own code (TBB + CHOLMOD/MKL) on 8 vCPU of the build container, ms per time step
REFERENCE_ANCHOR = {
    "bar17K_twist": {"ms_per_step": [924, 1331], "iters": [16, 20, 25, 26, 26, 26, 26, 27, 27, 27]},
    "bunny5K_LTSS": {"ms_per_step": [160, 360], "iters": [11, 10, 9, 9, 9, 10, 11, 11, 12, 12]},
    "monkey18K_stiff": {"ms_per_step": [4024, 10152], "iters": [108, 85, 98, 88, 145, 135, 145, 162, 131, 126]},
}
FP64_VECTOR_PEAK = 78.6  # TFLOP/s, FP64 vector (the same figure as the FP64 matrix peak on this part)
FP64_MFMA_PEAK = 78.6   # TFLOP/s, MI355X FP64 matrix = vector peak (256 CUs x 4 SIMD x 16 lanes x 2 x 2.4 GHz)
HBM_PEAK_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (6.29 TB/s measured copy)


def source_id():
    """sha256 (12 hex) over the device sources the kernels are built from: PMC files carry the id of the build they were
    measured on, and a traffic figure is only reported when it matches the build that runs"""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "dot_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "dot_amd", "csrc", "*.hpp"))):
        with open(f, "rb") as fh:
            hsh.update(os.path.basename(f).encode())
            hsh.update(fh.read())
    return hsh.hexdigest()[:12]


def plan_launch(gpus, env, device_count, argv):
    """What `python bench.py --gpus N` has to do before anything touches a GPU -> (action, payload):
      ("run", None)         this process is one of the N ranks (or N == 1) and goes on
      ("reexec", [cmd...])  N > 1 and no launcher started us: start N ranks of this script under torch.distributed.run
      ("fail", message)     the request cannot be met (fewer GPUs than ranks, launcher / --gpus mismatch)
    n_gpus in the JSON line is then always the number of ranks that ran (and equals the size of the RCCL communicator)."""
    if gpus < 1:
        return "fail", f"--gpus {gpus}: need at least one GPU"
    launched = "WORLD_SIZE" in env and "RANK" in env
    world = int(env.get("WORLD_SIZE", "1")) if launched else 1
    if launched and world != gpus:
        return "fail", f"--gpus {gpus} but the launcher started WORLD_SIZE={world} ranks"
    if device_count is not None and device_count < (1 if launched else gpus):
        return "fail", f"--gpus {gpus} but this box has {device_count} GPU(s)"
    if launched and device_count is not None and int(env.get("LOCAL_RANK", "0")) >= device_count:
        return "fail", f"LOCAL_RANK {env.get('LOCAL_RANK')} but this box has {device_count} GPU(s)"
    if gpus > 1 and not launched:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        return "reexec", [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
                          "--master-addr", "127.0.0.1", "--master-port", str(port)] + list(argv)
    return "run", None


def compact_line(full):
    """The driver-facing JSON line: the contract's keys plus numbers-only `roofline`, `roofline_factor`, `cpu_baseline` and a
    one-row-per-workload summary.  Everything else (roofline_by_kernel, PMC sources, notes) is in bench_detail.json."""
    keep = ("metric", "value", "unit", "n_gpus", "rccl_ranks", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "ms_per_step_p50", "ms_per_step_p95", "iters_per_frame", "step_breakdown_ms", "us_per_iter")
    out = {k: full[k] for k in keep if k in full}
    out["data"] = "reference input mesh (fixture), scripted handles"
    r = full["roofline"]
    out["roofline"] = {"bound": "hbm", "kernel": "backsolve_ctl_kernel", "achieved": r["achieved"], "peak": r["peak"],
                       "unit": "GB/s", "frac": r["frac"], "traffic": r["traffic"],
                       "traffic_source": r.get("traffic_source"),
                       "algorithmic_bytes_per_launch": r["algorithmic_bytes_per_launch"], "avg_launch_ms": r["avg_launch_ms"],
                       "launches_timed": r["launches_timed"], "launches_total": r["launches_total"],
                       "launches_stopped": r["launches_stopped"], "launches_held": r.get("launches_held", 0),
                       "launches_held_rejected": r.get("launches_held_rejected", 0)}
    f = full["roofline_factor"]
    out["roofline_factor"] = {"bound": "mfma", "kernel": f.get("kernel_name", "tile_task_kernel"), "achieved": f["achieved"], "peak": f["peak"],
                              "unit": "TFLOP/s", "frac": f["frac"], "flop": f["flop_per_factorisation"], "avg_ms": f["avg_ms"]}
    if full.get("roofline_loop"):
        lr = full["roofline_loop"]
        out["roofline_loop"] = {k: lr[k] for k in ("algorithmic_bytes_per_iteration", "us_per_iter", "achieved", "frac")}
    # the ALU side for the element kernels where a PMC flop count of this build is committed (FP64 vector peak)
    # (the fixed-corotational workloads' element pass -- the SVD inside -- and the headline's one-launch element pass + gather; every
    # other row is in bench_detail.json)
    alu = [{"kernel": r["kernel"], "workload": w.get("workload"), "flop": r["fp64_flop"], "us": r["us"],
            "frac_alu": r["frac_of_fp64_vector_peak"], "frac_hbm": r["frac_of_hbm_peak"]}
           for w in (full.get("workloads") or [{"workload": full["config"]["workload"], "energy": full["config"].get("energy"),
                                               "roofline_by_kernel": full.get("roofline_by_kernel")}])
           if "error" not in w
           for r in (w.get("roofline_by_kernel") or [])
           if r.get("fp64_flop") and ((w.get("energy") == "FCR" and r["kernel"] == "elem_step") or
                                      (w.get("workload") == full["config"]["workload"] and r["kernel"] == "elem_vertex"))]
    if alu:
        out["roofline_alu"] = alu
    if "collectives" in full:
        c = full["collectives"]
        out["collectives"] = {k: c[k] for k in ("allreduce_calls_per_step", "payload_MB_per_step", "est_ms_per_step") if k in c}
    if "cpu_baseline" in full:
        c = full["cpu_baseline"]
        cb = {k: c[k] for k in ("value", "unit", "cores", "kind", "leg", "sample") if k in c}
        a = c.get("reference_anchor") or {}
        if a.get("ms_per_step"):
            cb["reference_anchor_ms"] = a["ms_per_step"]
            cb["reference_anchor_cores"] = a.get("cores")
        rc = c.get("reference_cholmod") or {}
        if "factorize_ms_all_subdomains" in rc:
            cb["reference_cholmod"] = {"factorize_ms": rc["factorize_ms_all_subdomains"], "solve_ms": rc["solve_ms_all_subdomains"],
                                       "cores": rc["cores"], "nnz_L": rc.get("nnz_L")}
        for k in ("variants",):
            if k in c:
                cb[k] = c[k]
        out["cpu_baseline"] = cb
    if full.get("workloads"):
        out["workloads"] = [{"name": w["workload"], "ms_per_step": w["ms_per_step"], "iters": w["iters_per_frame"],
                             "us_per_iter": w.get("us_per_iter"), "loop_frac": (w.get("roofline_loop") or {}).get("frac"),
                             "backsolve_frac": w["roofline"]["frac"],
                             "factor_ms": w["step_breakdown_ms"]["subdomain_factor"],
                             "factor_frac": (w.get("roofline_factor") or {}).get("frac"),
                             **({"allreduce_per_step": w["collectives"]["allreduce_calls_per_step"],
                                 "payload_MB_per_step": w["collectives"]["payload_MB_per_step"]} if "collectives" in w else {})}
                            if "error" not in w else {"name": w["workload"], "error": w["error"][:120]}
                            for w in full["workloads"]]
    out["detail"] = "bench_detail.json"
    return out


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each array as dirname/<name>.npy in float64.  An array above its even share of `limit` keeps a
    fixed sample of its rows (seed 0, sorted), so that two runs of the same arguments write the same rows."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    share = limit // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        if a.nbytes > share:
            row = a.nbytes // a.shape[0]
            keep = np.sort(np.random.default_rng(0).choice(a.shape[0], max(share // row, 1), replace=False))
            a = a[keep]
        np.save(os.path.join(dirname, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default=DEFAULT_WORKLOAD)
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also the extra workloads, the per-kernel rooflines, the CPU baseline and bench_detail.json")
    ap.add_argument("--extra-workloads", default=EXTRA_WORKLOADS,
                    help="(--full) comma list of further workloads reported in the `workloads` array, or `none`")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) leave out the CPU baseline")
    ap.add_argument("--cpu-steps", type=int, default=12)
    ap.add_argument("--cpu-threads", type=int, default=0)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.distributed as dist

    from dot_amd import lib as dl
    from dot_amd.workloads import WORKLOADS, load_workload
    from dot_amd.timestepper import DOTTimeStepper, comm_unique_id

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    action, payload = plan_launch(args.gpus, os.environ, torch.cuda.device_count(), sys.argv)
    if action == "fail":
        raise SystemExit("bench.py: " + payload)
    if action == "reexec":
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, RCCL) and hand
        # their output through; this process never touches a GPU
        import subprocess
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        raise SystemExit(subprocess.call(payload, env=env))
    world = int(os.environ.get("WORLD_SIZE", "1")) if "RANK" in os.environ else 1
    rank = int(os.environ.get("RANK", "0")) if world > 1 else 0
    local_rank = int(os.environ.get("LOCAL_RANK", "0")) if world > 1 else 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl")

    def fresh_comm_id():
        """a new RCCL unique id per handle (an id serves ONE communicator), made on rank 0 and broadcast"""
        if world <= 1:
            return None
        buf = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            buf.copy_(torch.frombuffer(bytearray(comm_unique_id()), dtype=torch.uint8))
        dist.broadcast(buf, 0)
        return bytes(buf.cpu().numpy().tobytes())

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    SRC_ID = source_id()
    stale = {}

    flops_by_kernel = {}

    def pmc_by_kernel(workload):
        """HBM bytes per launch of every kernel class from the PMC counters (FETCH_SIZE / WRITE_SIZE need their own
        rocprofv3 passes, so they are collected separately on the same kernels + workload by tools/pmc_kernels.sh and
        committed under profiles/): -> ({bench kernel name: bytes}, file) or ({}, None)"""
        import glob
        for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_*.json")), reverse=True):
            with open(f) as fh:
                rec = json.load(fh)
            if rec.get("workload") != workload or "kernels" not in rec:
                continue
            if rec.get("source_id") != SRC_ID:
                # measured on another build of the kernels: not reported as this run's traffic
                stale.setdefault(workload, os.path.relpath(f, ROOT) + f" (source_id {rec.get('source_id')}, running {SRC_ID})")
                continue
            K = rec["kernels"]

            def pick(cls, must=None, total=False, key="hbm_bytes_per_launch"):
                import re
                inst = {k: v for k, v in K.get(cls, {}).items()
                        if key in v and (must is None or re.search(must, k))}
                if not inst:
                    return None
                vals = [v[key] for v in inst.values()]
                return int(sum(vals)) if total else int(vals[0])
            # (round 6) FP64 vector operations per launch from the same file's third pass: the ALU side of the roofline
            flop = {"elem_energy_grad": pick("elem_pass", r"<\d, true, \d, false,", key="fp64_flop_per_launch"),
                    "elem_energy": pick("elem_pass", r"<\d, false,", key="fp64_flop_per_launch"),
                    "elem_step": pick("elem_pass", r"<\d, true, \d, true,", key="fp64_flop_per_launch"),
                    "elem_hessian": pick("elem_hessian", key="fp64_flop_per_launch"),
                    "dirstep": pick("dirstep", key="fp64_flop_per_launch"), "spmv_zp": pick("spmv_zp", key="fp64_flop_per_launch"),
                    "elem_vertex": pick("elem_vertex", key="fp64_flop_per_launch")}
            flops_by_kernel[workload] = {k: v for k, v in flop.items() if v}
            # elem_patch_kernel<MAT, GRAD, EPT, FUSE (step inside), PIPE>
            out = {"elem_energy_grad": pick("elem_pass", r"<\d, true, \d, false,"), "elem_energy": pick("elem_pass", r"<\d, false,"),
                   "elem_step": pick("elem_pass", r"<\d, true, \d, true,"), "gather_early": pick("vertex_gather", "<true>"),
                   "dirstep": pick("dirstep"), "elem_vertex": pick("elem_vertex"),
                   "spmv_zp": pick("spmv_zp"), "merge_early": pick("merge_early"),
                   "vertex_gather": pick("vertex_gather", "<false>"), "spmv_dots": pick("spmv_dots"),
                   "backsolve": pick("backsolve", total=True), "merge": pick("merge", "<false>"),
                   "build_qpad": pick("build_qpad", "<false>"), "build_p": pick("build_p", "<false>"),
                   "step_forward": pick("step_forward"), "elem_hessian": pick("elem_hessian"), "assemble": pick("assemble")}
            # big meshes (split merge): the coalesced reduce of the tile partials is the first half of either merge form
            rp = pick("reduce_partial")
            if rp:
                if out.get("merge_early"):
                    out["merge_early"] += rp
                if not out.get("merge") and pick("merge_split"):
                    out["merge"] = pick("merge_split") + rp
            return {k: v for k, v in out.items() if v}, os.path.relpath(f, ROOT)
        return {}, None

    def pmc_traffic(workload):
        """HBM bytes of one back-solve (all its launches) from the newest committed PMC file of this workload"""
        t, f = pmc_by_kernel(workload)
        if "backsolve" in t:
            return t["backsolve"], f
        return None, ("stale: " + stale[workload]) if workload in stale else None

    def kernel_rooflines(ts, rec):
        """SURVEY.md section 8(d) "per kernel class": every hot kernel of the path launched back to back on this
        workload's resident data (dotmi_bench_kernel: HIP events around `reps` launches on the library's stream),
        its algorithmic bytes (or flop) from the section 8(d) formulas, and the fraction of the 8 TB/s HBM peak."""
        out = []
        L = dl.load()
        if not hasattr(L, "dotmi_bench_kernel"):
            return out
        import ctypes as C
        traffic, tsrc = pmc_by_kernel(rec["workload"]) if world == 1 else ({}, None)
        for kind, name in enumerate(dl.BENCH_KERNELS):
            ms, nbytes = C.c_double(), C.c_int64()
            rc = L.dotmi_bench_kernel(ts._h, kind, 20, C.byref(ms), C.byref(nbytes))
            if rc != 0 or ms.value <= 0:
                continue
            gbs = nbytes.value / (ms.value * 1e-3) / 1e9
            row = {"kernel": name, "us": round(1e3 * ms.value, 2), "algorithmic_bytes": int(nbytes.value),
                   "GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                   "traffic": traffic.get(name), "traffic_source": tsrc if name in traffic else None}
            fl = flops_by_kernel.get(rec["workload"], {}).get(name)
            if fl:
                # the ALU side: FP64 vector operations as executed (PMC: ADD + MUL + 2 FMA + TRANS wave
                # instructions x 64) against the FP64 vector peak -- what bounds the fixed-corotational element pass (SVD inside)
                tf = fl / (ms.value * 1e-3) / 1e12
                row.update({"fp64_flop": int(fl), "fp64_TFLOPs": round(tf, 2), "frac_of_fp64_vector_peak": round(tf / FP64_VECTOR_PEAK, 4)})
            out.append(row)
        return out

    def reference_cholmod_leg(sc2, ep2, nparts, orc):
        """Reference CHOLMODSolver (analyze once, then factorize + solve) on each subdomain's own-element matrix of the
        bench workload at the oracle's current state, one thread, timed inside oracle/ref_linsys.cpp."""
        from tests import oracle_py as O
        if not O.ref_solver_available():
            return {"error": "oracle/_ref/librefsolver.so or the image's MKL not present"}
        nT = sc2.T.shape[0]
        He = np.zeros((nT, 144))
        x = np.ascontiguousarray(orc.state()[0])
        O.lib().dor_eval_elem_hessians(orc.h, O._dp(x), O._dp(He))
        _, _, mass, _, _ = orc.features()
        tf = tsv = 0.0
        nnzL = 0
        for p in range(nparts):
            el = np.nonzero(ep2 == p)[0]
            verts = np.unique(sc2.T[el])
            loc = -np.ones(sc2.V_rest.shape[0], dtype=np.int64)
            loc[verts] = np.arange(verts.size)
            f_ms, s_ms, nz = O.ref_linsys_time(loc[sc2.T[el]].astype(np.int32), sc2.fixed[verts], He[el], mass[verts], 3, 10)
            tf += f_ms; tsv += s_ms; nnzL += nz
        return {"factorize_ms_all_subdomains": round(tf, 2), "solve_ms_all_subdomains": round(tsv, 2), "cores": 1,
                "subdomains": int(nparts), "nnz_L": int(nnzL),
                "what": "src/LinSysSolver/CHOLMODSolver.cpp (reference, compiled in place) on vendored CHOLMOD 3.0.12 + MKL, "
                        "one thread: best of 3 numeric factorisations / best of 10 solves per subdomain, summed over the subdomains (own-element matrices, "
                        "the pattern of H_s); the reference runs them concurrently under TBB"}

    def run_workload(name, steps, warmup, full=True, dump_dir=None):
        """-> (record, per-step stats, scene, timestepper is closed).  A trailing "+owner" (N > 1) runs the workload with
        DOTMI_FLAG_OWNER_EXCHANGE: interface-only vector collectives, the dot products in their tails.  full: also the
        per-kernel rooflines; dump_dir: write the outputs of the last timed step there (write_outputs)"""
        owner = name.endswith("+owner")
        label = name
        if owner:
            name = name[:-len("+owner")]
        sc, ep, nparts = load_workload(name)
        cfg = sc.cfg
        # one rank: dotmi_step returns with the end-of-step refresh queued (DOTMI_FLAG_ASYNC_REFRESH), so moving the handles
        # for the next step overlaps the factorisation; the timed region ends with a device-wide synchronisation, so every
        # refresh is inside it.  BENCH_SYNC_REFRESH=1 keeps the synchronous return.
        async_refresh = world == 1 and os.environ.get("BENCH_SYNC_REFRESH", "0") != "1"
        ts = DOTTimeStepper(sc, ep, nparts, device=local_rank, rank=rank, world=world, comm_id=fresh_comm_id(),
                            flags=dl.FLAG_TIME_BACKSOLVE | (dl.FLAG_ASYNC_REFRESH if async_refresh else 0) |
                            (dl.FLAG_OWNER_EXCHANGE if owner and world > 1 else 0))
        # the size of the communicator as RCCL reports it: n_gpus in the line is the ranks that really cooperate
        _L = dl.load()
        rr = int(_L.dotmi_comm_ranks(ts._h)) if hasattr(_L, "dotmi_comm_ranks") else world   # (a DOTMI_LIBRARY build without the entry)
        if rr != world:
            raise SystemExit(f"bench.py: {world} ranks were started but the RCCL communicator has {rr}")
        # scripted (Dirichlet) vertices are never moved by the solver: the scripter keeps their positions itself, as
        # the reference's host mesh does, instead of reading all positions back every step
        cached = cfg.script != "rubberBandPull"
        if cached:
            sc.scripter.track(sc.x0)

        def one_step():
            x = None if cached else ts.getResult()
            idx, pos = sc.scripter.step(x, cfg.dt)
            if idx.size:
                ts.setDirichlet(idx, pos)
            return ts.step()

        for _ in range(warmup):
            one_step()
        sync()
        t0 = time.perf_counter()
        stats, walls = [], []
        for _ in range(steps):
            c0 = time.perf_counter()
            stats.append(one_step())            # (the last step's refresh is covered by the sync() below)
            walls.append(time.perf_counter() - c0)
        sync()
        elapsed = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        if dump_dir:
            # before the per-kernel rooflines below: their launches run on the live state
            x, v, _ = ts.getState()
            last = stats[-1]
            write_outputs(dump_dir, {"positions": x, "velocities": v,
                                     "last_step": [last.E, last.g2, last.iters, last.ls_halvings]})
        iters = [s.iters for s in stats]
        # ---- roofline of the dominant hand-written kernel, measured inside the timed region -----------------
        pre_ms = sum(s.ms_precond for s in stats)
        pre_n = sum(s.precond_launches for s in stats)
        bytes_per_launch = stats[0].precond_bytes   # 8 x structural non-zeros of the inverse factors of THIS rank's parts
        avg_ms = pre_ms / max(pre_n, 1)
        achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if pre_n else 0.0
        # SURVEY.md section 8(d) prices the back-solve as a dense two-pass triangular solve: sum_s n_s^2 * 8 bytes
        L = dl.load()
        ns = [L.dotmi_part_size(ts._h, p) for p in range(nparts)]
        dense_bytes = int(sum(8 * n * n + 16 * n for n in ns))
        nmax = int(L.dotmi_padded_size(ts._h))
        traffic, traffic_src = pmc_traffic(name) if world == 1 else (None, None)
        # ---- N > 1: what the step spends in collectives (rank 0's view) ---------------------------------------------
        collectives = None
        if world > 1:
            calls = sum(s.collective_calls for s in stats)
            tms, tn = sum(s.ms_collective for s in stats), sum(s.collective_timed for s in stats)
            tb = sum(s.collective_timed_bytes for s in stats)
            collectives = {
                "allreduce_calls_per_step": round(calls / steps, 1),
                "payload_MB_per_step": round(sum(s.collective_bytes for s in stats) / steps / 1e6, 3),
                "timed": int(tn), "avg_ms_timed": round(tms / max(tn, 1), 5),
                "avg_payload_bytes_timed": int(tb / max(tn, 1)),
                # every 8th all-reduce is bracketed with HIP events on the library's stream; scaled to all of them
                "est_ms_per_step": round(tms / max(tn, 1) * calls / steps, 3),
                "note": "device time between events around ncclAllReduce on rank 0: includes waiting for the slowest rank",
            }
        two_level = hasattr(ts, "backsolveForm") and hasattr(dl.load(), "dotmi_backsolve_form") and ts.backsolveForm() == 1
        roofline = {
            "bound": "hbm", "kernel": ("twolevel_forward_kernel -> backsolve_kernel / backsolve_ctl_kernel -> twolevel_backward_kernel: the "
            "block solve in its two-level form (leaves against the separator complement; DESIGN.md section 4a), timed from the first "
            "kernel's start to the last one's end") if two_level else
            "backsolve_kernel / backsolve_ctl_kernel (the same tiles with the loop controller as "
            "workgroup 0): subdomain back-solve p_s = X_s^T (X_s r_s), nested-dissection block-sparse inverse factors, "
            "one streaming pass", "form": "two-level" if two_level else "one-pass",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": int(bytes_per_launch), "avg_launch_ms": round(avg_ms, 5),
            "bytes_definition": ("8 x (structural non-zeros of the leaves' and the separator complement's inverse factors, each once, "
                                 "+ 2 x the packed panels L_GD X_DD)") if two_level else
            "8 x structural non-zeros of the block-sparse X_s this launch streams (each once)",
            # the same launch priced with SURVEY 8(d)'s dense formula (what a dense forward + backward substitution
            # would have to read): > 1 means the dissection layout + single pass read that many times fewer bytes
            "dense_8d_bytes_per_launch": dense_bytes,
            "frac_if_priced_as_dense_8d": round(dense_bytes / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if pre_n else 0.0,
            # every 8th back-solve of the timed region is bracketed with HIP events (an event record costs ~6 us
            # of stream time, so bracketing all of them would inflate the metric by ~3%)
            # launches_total: the back-solves that ran to their end (one per L-BFGS iteration); launches_stopped: the
            # speculative ones of the early order that the controller stopped (one per rejected trial + one per step,
            # DESIGN.md section 5) -- they are not among the timed launches
            "launches_timed": int(pre_n), "launches_total": int(sum(s.backsolve_launches for s in stats)),
            "launches_stopped": int(sum(s.backsolve_stopped for s in stats)),
            # held: slots whose tiles waited for the controller's verdict (the trial was expected to be rejected);
            # held_rejected: those of them that were rejected and left without streaming (part of launches_stopped)
            "launches_held": int(sum(s.backsolve_held for s in stats)),
            "launches_held_rejected": int(sum(s.backsolve_held_rejected for s in stats)),
            # paired line-search trials: slots that evaluated alpha_0 / 2 in full and the energy of
            # alpha_0 in one launch; redone: the full step was acceptable after all and took the next slot (paired slots wait
            # like held ones and are counted among them)
            "slots_paired": int(sum(getattr(s, "paired_slots", 0) for s in stats)),
            "slots_paired_redone": int(sum(getattr(s, "paired_redone", 0) for s in stats)),
            "share_of_step_time": round(avg_ms * sum(s.backsolve_launches for s in stats) / (1e3 * elapsed), 3),
        }
        w = np.array(walls) * 1e3
        rec = {
            "workload": label, "rccl_ranks": rr, "nV": int(sc.V_rest.shape[0]), "nT": int(sc.T.shape[0]), "energy": cfg.energy,
            "subdomains": int(nparts), "dt": cfg.dt, "script": cfg.script, "steps": steps, "warmup": warmup,
            "ms_per_step": round(1e3 * elapsed / steps, 3), "ms_per_step_p50": round(float(np.percentile(w, 50)), 3),
            "ms_per_step_p95": round(float(np.percentile(w, 95)), 3),
            "iters_per_frame": round(float(np.mean(iters)), 2), "iters": iters,
            "halvings_per_frame": round(float(np.mean([s.ls_halvings for s in stats])), 2),
            "step_breakdown_ms": {
                "lbfgs_loop": round(float(np.mean([s.ms_loop for s in stats])), 3),
                "hessian_assembly": round(float(np.mean([s.ms_hessian for s in stats])), 3),
                "subdomain_factor": round(float(np.mean([s.ms_factor for s in stats])), 3),
                "back_solve_kernels": round(avg_ms * float(np.mean([s.backsolve_launches for s in stats])), 3),
            },
            "roofline": roofline,
            "collectives": collectives,
            "_ns": [int(v) for v in ns],
            "factor_storage_bytes": int(L.dotmi_factor_storage_bytes(ts._h)),
            "part_sizes": {"live_min": int(min(ns)), "live_mean": round(float(np.mean(ns)), 1), "live_max": int(max(ns)),
                           "padded": nmax},
        }
        # ---- second roofline: the once-per-step factorisation against the dense FP64 matrix-core peak ----------------
        fact_ms = float(np.mean([s.ms_factor for s in stats]))
        fact_tf = stats[0].factor_flops / (fact_ms * 1e-3) / 1e12 if fact_ms > 0 else 0.0
        rec["roofline_factor"] = {
            "bound": "mfma", "kernel_name": {1: "tile_task_kernel", 2: "tile_flow_kernel", 3: "tile_gemm_kernel + tile_task_kernel"}.get(int(L.dotmi_factor_kind(ts._h)) if hasattr(L, "dotmi_factor_kind") else 0, "?"),
            "kernel": "tile_task_kernel / tile_flow_kernel: block-sparse inverse-Cholesky of the subdomain blocks as 64x64 "
            "tile tasks (v_mfma_f64_16x16x4_f64 from LDS), once per step",
            "achieved": round(fact_tf, 2), "peak": FP64_MFMA_PEAK, "unit": "TFLOP/s", "frac": round(fact_tf / FP64_MFMA_PEAK, 4),
            "flop_per_factorisation": float(stats[0].factor_flops), "avg_ms": round(fact_ms, 4),
            "note": "flop as executed on the tiles that can be non-zero in each subdomain (padding only inside 64-tiles)",
            # for scale: a dense potrf + trtri on the live sizes would be (2/3) sum n_s^3 flop
            "dense_potrf_trtri_flop_on_live_sizes": float(sum(2.0 / 3.0 * n ** 3 for n in ns)),
            "factor_storage_bytes": rec.get("factor_storage_bytes"),
        }
        target = ts.targetGRes
        rec["roofline_by_kernel"] = kernel_rooflines(ts, rec) if full and (rank == 0 or world == 1) else None
        # ---- the loop as a whole: device time of the L-BFGS loop per iteration (comparable across rounds where
        # a chaotic workload's iteration count moves) and the algorithmic bytes one iteration's launches read and write -- the
        # back-solve's structural non-zeros + the four vector kernels' section 8(d) bytes in the forms the loop launches -- over it
        it_mean = float(np.mean(iters))
        us_iter = 1e3 * float(np.mean([s.ms_loop for s in stats])) / max(it_mean, 1.0)
        rec["us_per_iter"] = round(us_iter, 2)
        byk = {r["kernel"]: r for r in (rec["roofline_by_kernel"] or [])}
        loop_k = ("spmv_zp", "elem_step", "gather_early", "merge_early")
        if all(k in byk for k in loop_k):
            lb = int(bytes_per_launch + sum(byk[k]["algorithmic_bytes"] for k in loop_k))
            rec["roofline_loop"] = {"bound": "hbm", "algorithmic_bytes_per_iteration": lb, "us_per_iter": round(us_iter, 2),
                                    "achieved": round(lb / (us_iter * 1e-6) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": round(lb / (us_iter * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                                    "what": "back-solve + spmv_zp + element pass with the step + gather + merge_early, "
                                            "algorithmic bytes of one iteration over the loop's device time per iteration (incl. "
                                            "rejected trials, the start-of-step evaluation and the launch gaps)"}
        rec["spec"] = {"slots": int(sum(getattr(s, "spec_slots", 0) for s in stats)),
                       "redone": int(sum(getattr(s, "spec_redone", 0) for s in stats))}
        if rec["collectives"] is None:
            del rec["collectives"]
        ts.close()
        return rec, stats, sc, nparts, target, elapsed

    rec, stats, sc, nparts, target_gres, elapsed = run_workload(args.workload, args.steps, args.warmup, full=args.full,
                                                                dump_dir=args.dump_outputs if rank == 0 else None)
    cfg = sc.cfg
    ms_per_step = rec["ms_per_step"]
    iters = rec["iters"]
    roofline = rec["roofline"]
    avg_ms = roofline["avg_launch_ms"]

    roofline_factor = rec["roofline_factor"]
    del rec["_ns"]

    # ---- the other configurations BASELINE.json / north_star name, short runs (every rank takes part) --------------
    extra = []
    if args.full and args.extra_workloads and args.extra_workloads != "none":
        names = args.extra_workloads.split(",")
        if world > 1:
            # N > 1: the two configurations meant to scale also under the owner exchange (interface-only collectives), next to
            # the replicated-vector sharding, so that a multi-GPU run measures both
            names += [n_ + "+owner" for n_ in names if n_.startswith("synbar") or "@r" in n_]
        for name in names:
            if name == args.workload:
                continue
            st_, wu_ = EXTRA_STEPS.get(name.replace("+owner", ""), (6, 2))
            try:
                r2 = run_workload(name, st_, wu_)[0]
            except Exception as e:   # noqa: BLE001  (an extra workload must not cost the line its headline)
                # N > 1: the other ranks are inside this workload's collectives -- a rank that carried on alone would leave
                # them waiting for ever, so the error ends this rank and the launcher takes the job down
                if name.endswith("+owner") and world == 1:
                    extra.append({"workload": name, "error": repr(e)})
                    continue
                raise
            r2.pop("_ns", None)
            extra.append(r2)

    out = None
    if rank == 0:
        out = {
            "metric": "ms_per_time_step", "value": ms_per_step, "unit": "ms", "n_gpus": world, "rccl_ranks": rec["rccl_ranks"],
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": False, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "mesh fixture tests/golden/meshes (reference input mesh), scripted handles",
            "config": {
                "workload": args.workload, "nV": rec["nV"], "nT": rec["nT"],
                "energy": cfg.energy, "subdomains": int(nparts), "dt": cfg.dt, "script": cfg.script,
                "rel_tol": 1e-5, "target_gres": target_gres,
                "parallelism": f"{nparts} subdomains sharded over {world} GPU(s), RCCL all-reduce" if world > 1
                               else f"{nparts} subdomains on 1 GPU",
            },
            "ms_per_step_p50": rec["ms_per_step_p50"], "ms_per_step_p95": rec["ms_per_step_p95"],
            "iters_per_frame": rec["iters_per_frame"], "iters": iters,
            "step_breakdown_ms": rec["step_breakdown_ms"],
            "us_per_iter": rec.get("us_per_iter"),
            "roofline": roofline,
            "roofline_factor": roofline_factor,
            "roofline_loop": rec.get("roofline_loop"),
            "spec": rec.get("spec"),
        }
        if "collectives" in rec:
            out["collectives"] = rec["collectives"]
        out["roofline_by_kernel"] = rec.get("roofline_by_kernel")
        if extra:
            out["workloads"] = [rec] + extra
        # ---- CPU baseline on this box's host cores: bounded sample of the same workload ---------------
        if args.full and not args.no_cpu_baseline and world == 1:
            from tests import oracle_py as O
            threads = args.cpu_threads or min(os.cpu_count() or 1, 16)
            O.lib().dor_set_threads(threads)
            nwarm = min(args.warmup, 2)

            def cpu_leg(reference_cholmod):
                """the oracle on `threads` host threads over a bounded sample of the workload; with reference_cholmod the
                subdomain factorisations / solves run in the reference's own CHOLMODSolver (one object per subdomain,
                OpenMP over the subdomains as the reference's TBB loops DOTTimeStepper.cpp:363-377, :406-431)"""
                sc2, ep2, _ = load_workload(args.workload)
                orc = O.OracleSim(sc2.V_rest, sc2.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc2.fixed, sc2.x0,
                                  ep2, nparts, cfg.with_gravity)
                if reference_cholmod and O.use_reference_cholmod(orc) != 0:
                    raise RuntimeError("the reference CHOLMODSolver could not factorise a subdomain")
                times, cits, tf, tsv = [], [], [], []
                budget_t0 = time.perf_counter()
                for k in range(nwarm + args.cpu_steps):
                    x = orc.state()[0]
                    idx, pos = sc2.scripter.step(x, cfg.dt)
                    orc.move(idx, pos)
                    c0 = time.perf_counter()
                    so = orc.step()
                    if k >= nwarm:
                        times.append(time.perf_counter() - c0)
                        cits.append(so.iters)
                        tf.append(so.ms_factor)
                        tsv.append(so.ms_backsolve)
                    if time.perf_counter() - budget_t0 > (15.0 if reference_cholmod else 30.0) and len(times) >= 3:
                        break
                if orc.factor_failed():   # steps timed on a failed factorisation are not a baseline
                    raise RuntimeError("a subdomain factorisation failed during the CPU leg")
                return sc2, ep2, orc, times, cits, float(np.mean(tf)), float(np.mean(tsv))

            sc2, ep2, orc, times, cits, tf_, ts_ = cpu_leg(False)
            out["cpu_baseline"] = {
                "value": round(1e3 * float(np.mean(times)), 2), "unit": "ms", "cores": threads, "kind": "port",
                "sample": f"steps {nwarm}..{nwarm + len(times) - 1} of {args.workload} (same partition, same tolerance), "
                          f"oracle/dot_oracle.c with OpenMP (own envelope Cholesky), iters/step {cits}",
                "factor_ms": round(tf_, 2), "backsolve_ms": round(ts_, 2),
                # the reference's own code cannot be built on this box (TBB); what BASELINE.md section 2 measured with it
                "reference_anchor": dict(REFERENCE_ANCHOR.get(args.workload, {}), cores=8, source="BASELINE.md section 2: "
                                         "the reference's unmodified sources, 8 vCPU Xeon 2.1 GHz, OMP_NUM_THREADS=8, MKL sequential"),
            }
            # second variant: the same stepping leg with the reference's CHOLMODSolver doing the linear
            # algebra of the subdomains (oracle/_ref/librefsolver.so = src/LinSysSolver/CHOLMODSolver.cpp compiled in place)
            if O.ref_solver_available():
                try:
                    _, _, orc2, times2, cits2, tf2, ts2 = cpu_leg(True)
                    orc2.close()
                    # this leg is the headline baseline: the reference's own linear algebra under the
                    # restated stepper is the closest thing to the reference's CPU path that runs on this box; the port
                    # with its own envelope Cholesky (factor ~60 ms instead of ~9) becomes the variant
                    cbp = out["cpu_baseline"]
                    port_variant = {"kind": "port", "leg": "port (own envelope Cholesky)", "value": cbp["value"], "unit": "ms", "cores": threads, "steps": len(times),
                                    "factor_ms": cbp["factor_ms"], "backsolve_ms": cbp["backsolve_ms"]}
                    cbp.update({
                        "value": round(1e3 * float(np.mean(times2)), 2), "kind": "port", "leg": "port+reference_cholmod",
                        "sample": f"steps {nwarm}..{nwarm + len(times2) - 1} of {args.workload} (same partition, same tolerance), "
                                  f"oracle/dot_oracle.c with OpenMP over the subdomains, factorisations and solves in the "
                                  f"reference's CHOLMODSolver (oracle/_ref, vendored CHOLMOD + MKL), iters/step {cits2}",
                        "factor_ms": round(tf2, 2), "backsolve_ms": round(ts2, 2),
                        "iters_equal_port": cits2 == cits[:len(cits2)]})
                    cbp["variants"] = [port_variant]
                except Exception as e:   # noqa: BLE001 - optional leg (needs oracle/_ref + the image's MKL)
                    out["cpu_baseline"]["variants"] = [{"kind": "port", "leg": "port+reference_cholmod", "error": f"{type(e).__name__}: {e}"}]
            # the one piece of the reference that IS compiled here, timed on the same subdomains: CHOLMODSolver
            # factorize + solve (oracle/_ref/librefsolver.so = src/LinSysSolver/CHOLMODSolver.cpp on the vendored CHOLMOD)
            try:
                out["cpu_baseline"]["reference_cholmod"] = reference_cholmod_leg(sc2, ep2, nparts, orc)
            except Exception as e:   # noqa: BLE001 - the leg is optional (needs oracle/_ref + the image's MKL)
                out["cpu_baseline"]["reference_cholmod"] = {"error": f"{type(e).__name__}: {e}"}
        line = compact_line(out)
        if args.full:
            # the full record (per-kernel rooflines, PMC sources, per-workload detail, the long explanatory strings) goes to a
            # side file; the ONE stdout line stays below 4 KB so that the driver's parser gets all of it
            try:
                with open(os.path.join(ROOT, "bench_detail.json"), "w") as fh:
                    json.dump(out, fh, indent=1)
            except OSError:
                pass
        else:
            del line["detail"]
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
