"""The sharded (N > 1) sequencing of libdotmi with REAL partial ownership, on a one-GPU box: two processes, each with its
own handle on the same device (rank 0 / rank 1 of world 2), the library's collectives routed through the host
all-reduce hook (dotmi_params::allreduce) into a torch.distributed gloo all_reduce.  RCCL refuses two ranks on one
device, so this is the only way to execute the world > 1 code path -- ownership of parts / elements / vertex slices,
merge over owned parts only, div_dup after the all-reduce, the [g ; E] packing, rank 0's control scalars adopted by
every rank, joint failure -- before an 8-GPU node is available.  """
import os
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, initfile, outdir, workload, shard_elems, steps, material=None, rank_env=None):
    """material: optional (kind, seed) of a per-element Lame field of tests/materials.py, rebuilt here from its name
    rank_env: environment switches of the ranks' handles only (the single-GPU run they are compared with keeps the caller's)"""
    sys.path.insert(0, ROOT)
    os.environ.update(rank_env or {})
    owner = shard_elems.startswith("owner")   # DOTMI_FLAG_OWNER_EXCHANGE: interface-only exchange, owner-summed dot products
    if owner:
        shard_elems = "1"
    os.environ["DOTMI_SHARD_ELEMS"] = shard_elems
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist
    from tests.workloads import load_workload
    from dot_amd.timestepper import DOTTimeStepper

    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    calls = [0]
    nbytes = [0]

    def allreduce(a):
        calls[0] += 1
        nbytes[0] += a.nbytes
        dist.all_reduce(torch.from_numpy(a))

    from dot_amd import lib as dl
    sc, ep, n = load_workload(workload)
    mu = lam = None
    if material is not None:
        from tests.materials import field
        mu, lam = field(sc, *material)
    ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world, allreduce=allreduce,
                        flags=dl.FLAG_OWNER_EXCHANGE if owner else 0, mu=mu, lam=lam)
    calls[0] = nbytes[0] = 0          # (the collectives of dotmi_create are not the loop's)
    its, halv, Es = [], [], []
    for _ in range(steps):
        x = ts.getResult()
        idx, pos = sc.scripter.step(x, sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        its.append(st.iters); halv.append(st.ls_halvings); Es.append(st.E)
    loop_calls, loop_bytes = calls[0], nbytes[0]
    r = np.random.default_rng(3).standard_normal(sc.x0.shape) * (1 - sc.fixed[:, None])
    z = ts.applyPrecond(r)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), x=ts.getResult(), v=ts.getState()[1], its=its, halv=halv, E=Es,
             z=z, calls=loop_calls, bytes=loop_bytes, forms=ts.loopForms())
    ts.close()
    dist.barrier()
    dist.destroy_process_group()


# (workload, steps, sharded element pass + refresh, world).  The last two are the configurations BASELINE.json assigns to
# 4 / 8 GPUs, reduced to what one GPU holds several times over: the stiff monkey (64 subdomains, back-tracking) on two
# ranks and the synthetic bar with the sharded element pass / sharded Hessian refresh on FOUR ranks (four processes on
# one device).
# "owner" (round 4): DOTMI_FLAG_OWNER_EXCHANGE -- the loop's vector collectives carry only the entries of vertices held by
# more than one rank, the dot products travel inside those packets (taken before the exchange where they are linear in the
# exchanged vector), the positions are made whole once per step.
CASES = [("bunny5K_LTSS", 4, "0", 2), ("bunny5K_LTSS", 4, "1", 2), ("horse7K_stretch", 4, "0", 2),
         ("horse7K_stretch", 4, "1", 2), ("monkey18K_stiff", 1, "0", 2), ("synbar:40x10x10:32", 2, "1", 4),
         ("bunny5K_LTSS", 4, "owner", 2), ("horse7K_stretch", 4, "owner", 2), ("bar17K_twist", 2, "owner", 4),
         ("synbar:40x10x10:32", 2, "owner", 4), ("monkey18K_stiff", 1, "owner", 3),
         # eight ranks, what `bench.py --gpus 8` hands a node: bunny5K / 8 leaves every rank ONE subdomain, bar17K / 32 four
         ("bunny5K_LTSS", 3, "0", 8), ("bar17K_twist", 2, "0", 8), ("bar17K_twist", 2, "owner", 8),
         ("synbar:40x10x10:32", 2, "1", 8), ("synbar:40x10x10:32", 2, "owner", 8)]


@pytest.mark.parametrize("workload,steps,shard_elems,world", CASES)
def test_ranks_on_one_gpu_reproduce_the_single_gpu_run(workload, steps, shard_elems, world):
    _ranks_reproduce_the_single_gpu_run(workload, steps, shard_elems, world)


def test_ranks_with_per_element_materials_reproduce_the_single_gpu_run():
    """A random Lame field per element (tests/materials.py) with the sharded element pass and refresh: each rank's refresh
    evaluates only the elements its vertices need (hessElems, a strict subset of the mesh on two ranks), so the element Hessian
    kernel must read the material of element elist[i], not of element i."""
    _ranks_reproduce_the_single_gpu_run("bunny5K_LTSS", 4, "1", 2, material=("random", 0))


def _ranks_reproduce_the_single_gpu_run(workload, steps, shard_elems, world, material=None, rank_env=None):
    """-> per rank, what its handle's loop launched (DOTTimeStepper.loopForms)"""
    import torch.multiprocessing as mp
    from tests.workloads import load_workload
    from dot_amd.timestepper import DOTTimeStepper

    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        initfile = os.path.join(d, "init")
        procs = [ctx.Process(target=_worker, args=(r, world, initfile, d, workload, shard_elems, steps, material, rank_env))
                 for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive, "a rank hung (ranks branched apart?)"
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        R = [np.load(os.path.join(d, f"rank{r}.npz")) for r in range(world)]
    forms = [int(R[r]["forms"]) for r in range(world)]
    # the ranks hold the same replicated state, bit for bit
    for r in range(1, world):
        for k in ("x", "v", "its", "halv", "E", "z"):
            assert np.array_equal(R[0][k], R[r][k]), (r, k)
    # the loop runs on the device; replicated element pass: ONE collective per slot (+ the end-of-batch agreement);
    # sharded element pass: z + alpha_0 scalars + staged [g ; 0 ; E] per slot
    # owner exchange: packed [z ; y_i.z] + two scalars + packed [g ; E ; statistics] per slot, the positions once per step
    per_iter = {"0": 1, "1": 3, "owner": 3}[shard_elems]
    assert all(int(R[r]["calls"]) == int(R[0]["calls"]) for r in range(world))
    assert int(R[0]["calls"]) >= per_iter * int(R[0]["its"].sum())
    if shard_elems.startswith("owner"):
        # what travels per L-BFGS iteration: two packed vectors of the shared vertices' entries instead of two full ones
        # (+ one full vector per step); measured against the sharded path on the same workload below the bound 2 n x 8
        n3 = 3 * load_workload(workload)[0].x0.shape[0]
        per_it = (int(R[0]["bytes"]) - steps * 8 * n3) / max(1, int(R[0]["calls"]) // per_iter)
        assert per_it < 0.75 * 2 * 8 * n3, (per_it, 2 * 8 * n3)
    # and it is the single-GPU run up to the summation order of the exchanged vectors
    sc, ep, n = load_workload(workload)
    mu = lam = None
    if material is not None:
        from tests.materials import field
        mu, lam = field(sc, *material)
    ts = DOTTimeStepper(sc, ep, n, mu=mu, lam=lam)
    its, halv = [], []
    for _ in range(steps):
        x = ts.getResult()
        idx, pos = sc.scripter.step(x, sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        st = ts.step()
        its.append(st.iters); halv.append(st.ls_halvings)
    if workload == "monkey18K_stiff":
        # ~100 iterations with as many back-tracking halvings in one step: the summation order of the exchanged vectors
        # (all-reduce vs single-GPU merge) is amplified by the line search -- same
        # tolerance reached, iteration count in the same range
        assert all(abs(a - b) <= 0.25 * b for a, b in zip(R[0]["its"].tolist(), its))
        ts.close()
        return forms
    assert its == R[0]["its"].tolist() and halv == R[0]["halv"].tolist()
    assert np.abs(ts.getResult() - R[0]["x"]).max() < 1e-9
    r = np.random.default_rng(3).standard_normal(sc.x0.shape) * (1 - sc.fixed[:, None])
    z = ts.applyPrecond(r)
    # the factors were refreshed at end-of-step positions that agree to ~1e-10: the block solve amplifies that by the
    # conditioning of the subdomain matrices
    assert np.abs(z - R[0]["z"]).max() <= 1e-6 * np.abs(z).max()
    ts.close()
    return forms


def _worker_disagree(rank, world, initfile, outdir):
    sys.path.insert(0, ROOT)
    os.environ["DOTMI_SHARD_ELEMS"] = "0"
    # the build with the fault-injection hook (the product library has none): this process reports its iteration count
    # shifted by delta.  world 2: (0, +1).  world 3: (0, -1, +1) -- the sum over the ranks is then world x rank 0's
    # value, the pattern the first version of the check let rank 0 pass
    os.environ["DOTMI_LIBRARY"] = os.path.join(ROOT, "dot_amd", "libdotmi_testhooks.so")
    os.environ["DOTMI_TEST_ITER_DELTA"] = str({2: (0, 1), 3: (0, -1, 1)}[world][rank])
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist
    from tests.workloads import load_workload
    from dot_amd.timestepper import DOTTimeStepper
    from dot_amd.lib import DotmiError

    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    sc, ep, n = load_workload("bunny5K_LTSS")
    ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world,
                        allreduce=lambda a: dist.all_reduce(torch.from_numpy(a)))
    msg = ""
    try:
        ts.step()
    except DotmiError as e:
        msg = str(e)
    with open(os.path.join(outdir, f"rank{rank}.txt"), "w") as f:
        f.write(msg)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_that_disagree_fail_together_instead_of_hanging(world):
    """The sharded loop ends every batch of slots with an all-reduce of the ranks' loop states, their squares and an error
    flag; ranks whose states differ (forced through the hook of libdotmi_testhooks.so) make EVERY rank return
    DOTMI_E_DEVICE from the same collective -- nobody is left waiting in the next all-reduce.  world 3 reports
    (k, k-1, k+1) iterations: the sums alone equal 3 x rank 0's values, the variance test still fails everywhere."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        procs = [ctx.Process(target=_worker_disagree, args=(r, world, os.path.join(d, "init"), d)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive, "a rank hung"
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        msgs = [open(os.path.join(d, f"rank{r}.txt")).read() for r in range(world)]
    assert all("different states" in m for m in msgs), msgs


def _worker_rccl(rank, world, port, outdir, workload, steps):
    sys.path.insert(0, ROOT)
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    import torch
    import torch.distributed as dist
    from tests.workloads import load_workload
    from dot_amd.timestepper import DOTTimeStepper, comm_unique_id

    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    buf = torch.zeros(128, dtype=torch.uint8, device="cuda")
    if rank == 0:
        buf.copy_(torch.frombuffer(bytearray(comm_unique_id()), dtype=torch.uint8))
    dist.broadcast(buf, 0)
    sc, ep, n = load_workload(workload)
    ts = DOTTimeStepper(sc, ep, n, device=rank, rank=rank, world=world, comm_id=bytes(buf.cpu().numpy().tobytes()))
    its = []
    for _ in range(steps):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        its.append(ts.step().iters)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), x=ts.getResult(), its=its)
    ts.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_real_rccl_ranks_when_the_box_has_two_gpus():
    """The same run over RCCL itself (ncclAllReduce on the handles' streams, one process per GPU) -- skipped on a one-GPU
    box, active by itself on any box with two or more."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    import torch.multiprocessing as mp
    from tests.workloads import load_workload
    from dot_amd.timestepper import DOTTimeStepper
    workload, steps, world = "bunny5K_LTSS", 3, 2
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        procs = [ctx.Process(target=_worker_rccl, args=(r, world, 29611, d, workload, steps)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive and all(p.exitcode == 0 for p in procs)
        R = [np.load(os.path.join(d, f"rank{r}.npz")) for r in range(world)]
    assert np.array_equal(R[0]["x"], R[1]["x"]) and np.array_equal(R[0]["its"], R[1]["its"])
    sc, ep, n = load_workload(workload)
    ts = DOTTimeStepper(sc, ep, n)
    its = []
    for _ in range(steps):
        idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
        ts.setDirichlet(idx, pos)
        its.append(ts.step().iters)
    assert its == R[0]["its"].tolist() and np.abs(ts.getResult() - R[0]["x"]).max() < 1e-9
    ts.close()
