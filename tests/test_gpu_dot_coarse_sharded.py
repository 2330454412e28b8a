"""DOTMI_FLAG_DOT_COARSE: the rigid-mode coarse term M' = M + Z A0^-1 Z^T on SHARDED handles (dotmi_coarse.hip, k_coarse.hip,
zfinish_kernel<DEV, COARSE> and the zsum branch of merge_tiles_early_kernel<NT, true> in k_loopvec.hip, the four call sites in
dotmi_loop.hip / dotmi_devloop.hip; DESIGN.md sections 6 and 9).

1. one rank under DOTMI_FLAG_FORCE_DIST, both values of DOTMI_SHARD_ELEMS: one application against (the sharded application without
   the term) + the restated Z A0^-1 Z^T r; four steps against a plain handle with setDotCoarse(1), in the early and the q-based
   order, the host loop and the split merge; two runs bit-identical.
2. real partial ownership, the worker pattern of tests/test_gpu_two_ranks.py (processes on one GPU, a gloo all-reduce hook that records
   every call's payload size, a time-limited join): ranks bit-identical, the single-GPU setDotCoarse(1) run's iterations and
   halvings, A0 on every rank, the iteration count on 32 subdomains, the payload histogram against a run without the flag.
3. dotCoarseInfo on a rank, one build per refresh, a subdomain dropped through dotmi_refix.
4. refusals at create.

Shapes: synbar:16x5x5:4 (nc = 24), synbar:48x4x4:12 (nc = 72: a 64-row block boundary inside A0), bunny5K_LTSS / 8 (dup <= 5),
synbar:96x4x4:32 (nc = 192)."""
import collections
import os
import sys
import tempfile

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from dot_amd.workloads import load_workload
from tests import coarse_reference as CR
from tests import dot_coarse_reference as DR
from tests import pcg_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAR4, BAR12, BAR32, BUNNY = "synbar:16x5x5:4", "synbar:48x4x4:12", "synbar:96x4x4:32", "bunny5K_LTSS"
SHARDED = dl.FLAG_FORCE_DIST | dl.FLAG_DOT_COARSE
_plain = {}


def scripted(sc, ts):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    ts.setDirichlet(idx, pos)


def part_verts(T, ep, n):
    T, ep = np.asarray(T), np.asarray(ep)
    return [np.unique(T[ep == s]) for s in range(n)]


def random_free(fixed, seed):
    v = np.random.default_rng(seed).standard_normal((fixed.size, 3))
    v[fixed] = 0.0
    return v


def run_steps(name, steps, flags=0, set_mode=False, refix_part=None):
    """scripted steps on a fresh handle -> dict(counts, xs, A0 before any step, infos).  refix_part: that subdomain's vertices are fixed
    through dotmi_refix behind the first step"""
    sc, ep, n = load_workload(name)
    ts = DOTTimeStepper(sc, ep, n, flags=flags)
    if set_mode:
        ts.setDotCoarse(1)
    out = dict(counts=[], xs=[], infos=[ts.dotCoarseInfo()], A0=ts.pcgCoarseMatrix() if (set_mode or flags & dl.FLAG_DOT_COARSE) else None)
    for k in range(steps):
        scripted(sc, ts)
        st = ts.step()
        out["counts"].append((st.iters, st.ls_halvings, st.status))
        out["xs"].append(ts.getResult().copy())
        out["infos"].append(ts.dotCoarseInfo())
        if k == 0 and refix_part is not None:
            fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
            fixed[part_verts(sc.T, ep, n)[refix_part]] = 1
            ts.refix(fixed)
            out["infos"].append(ts.dotCoarseInfo())
    ts.close()
    return out


def plain_run(name, steps, refix_part=None):
    """the single-GPU handle with setDotCoarse(1), default forms, once per configuration (call it before any monkeypatch.setenv)"""
    key = (name, steps, refix_part)
    if key not in _plain:
        _plain[key] = run_steps(name, steps, set_mode=True, refix_part=refix_part)
    return _plain[key]


# ---- 1. one rank under FORCE_DIST ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", ["0", "1"])
@pytest.mark.parametrize("name", [BAR4, BAR12])
def test_sharded_application_is_the_plain_sharded_one_plus_the_restated_coarse_term(name, shard, monkeypatch):
    """dotmi_apply_precond on a FORCE_DIST | DOT_COARSE handle against the same entry on a FORCE_DIST handle plus Z A0^-1 Z^T r restated
    on a plain handle's dotmi_spmv at the same positions: 1e-10 of the largest entry (the bound of tests/test_gpu_dot_coarse.py)"""
    sc, ep, n = load_workload(name)
    nV = sc.V_rest.shape[0]
    fixed = np.asarray(sc.fixed, dtype=bool)

    def moved(flags):
        ts = DOTTimeStepper(sc, ep, n, flags=flags)
        scripted(sc, ts)
        ts.updatePrecondMtrAndFactorize()
        return ts
    plain = moved(0)
    monkeypatch.setenv("DOTMI_SHARD_ELEMS", shard)
    off, on = moved(dl.FLAG_FORCE_DIST), moved(SHARDED)
    assert np.array_equal(off.getResult(), plain.getResult()) and np.array_equal(on.getResult(), plain.getResult())
    apply, live = DR.coarse_term(plain.getResult(), R.dup_of(sc.T, ep, nV), part_verts(sc.T, ep, n), fixed, plain.multiply)
    assert live.all() and apply is not None
    assert on.dotCoarseInfo()[:4] == (6 * n, 0, 1, 2) and off.dotCoarseInfo()[:4] == (0, 0, 0, 0)   # (create's refresh and the explicit one)
    r = random_free(fixed, 11)
    z_off, z_on = off.applyPrecond(r), on.applyPrecond(r)
    want = z_off + apply(r)
    err = np.abs(z_on - want).max() / np.abs(want).max()
    print(f"{name}, DOTMI_SHARD_ELEMS={shard}: nc {6 * n}, application against the restatement {err:.2e}; the coarse term is "
          f"{np.abs(z_on - z_off).max() / np.abs(z_on).max():.2e} of it")
    assert err <= 1e-10
    assert np.abs(z_on - z_off).max() > 1e-6 * np.abs(z_on).max()            # (the term is not a rounding matter)
    assert np.array_equal(on.applyPrecond(r), z_on)
    assert np.array_equal(z_on[fixed], z_off[fixed])
    with pytest.raises(DotmiError, match="dotmi_set_dot_coarse.*single-rank"):     # the setter keeps refusing: the flag is the only way
        on.setDotCoarse(0)
    for ts in (plain, off, on):
        ts.close()


FORMS = [("early order", {}, 0), ("q-based order", {"DOTMI_EARLY_BACKSOLVE": "0"}, 0), ("host loop", {}, dl.FLAG_HOST_LOOP),
         ("split merge", {"DOTMI_SPLIT_MERGE": "1"}, 0)]


@pytest.mark.parametrize("form,env,flags", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("shard", ["0", "1"])
@pytest.mark.parametrize("name", [BAR4, BAR12])
def test_four_sharded_steps_take_the_plain_handles_iterations_and_halvings(name, shard, form, env, flags, monkeypatch):
    """FORCE_DIST | DOT_COARSE on one rank against a plain handle with setDotCoarse(1): same iterations and halvings, positions within
    1e-9 (the standing bound of the sharded path, tests/test_gpu_two_ranks.py); in the early order twice, bit for bit"""
    want = plain_run(name, 4)
    monkeypatch.setenv("DOTMI_SHARD_ELEMS", shard)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = run_steps(name, 4, flags=SHARDED | flags)
    err = max(np.abs(a - b).max() for a, b in zip(got["xs"], want["xs"]))
    print(f"{name}, DOTMI_SHARD_ELEMS={shard}, {form}: {got['counts']}, plain {want['counts']}, positions {err:.2e}")
    assert all(i[2] == 1 and i[1] == 0 for i in got["infos"])
    assert [i[3] for i in got["infos"]] == [1, 2, 3, 4, 5]                      # one build per refresh, from create's on
    assert got["counts"] == want["counts"]
    assert err < 1e-9
    dA = np.abs(got["A0"] - want["A0"]).max() / np.abs(want["A0"]).max()
    assert dA <= 1e-12, dA
    if form == "early order":
        again = run_steps(name, 4, flags=SHARDED | flags)
        assert again["counts"] == got["counts"]
        for a, b in zip(again["xs"], got["xs"]):
            assert np.array_equal(a, b)


def test_flag_on_a_single_rank_handle_is_create_followed_by_the_setter():
    want = plain_run(BAR4, 4)
    got = run_steps(BAR4, 4, flags=dl.FLAG_DOT_COARSE)
    assert got["counts"] == want["counts"] and [i[:4] for i in got["infos"]] == [i[:4] for i in want["infos"]]
    for a, b in zip(got["xs"], want["xs"]):
        assert np.array_equal(a, b)
    sc, ep, n = load_workload(BAR4)
    ts = DOTTimeStepper(sc, ep, n, flags=dl.FLAG_DOT_COARSE)
    ts.setDotCoarse(0)                                                          # ... and can still be toggled
    assert ts.dotCoarseInfo()[:3] == (0, 0, 0)
    ts.close()


# ---- 2. real partial ownership ----------------------------------------------------------------------------------------------------------------
def _worker(rank, world, initfile, outdir, workload, shard, steps, refix_part):
    sys.path.insert(0, ROOT)
    os.environ["DOTMI_SHARD_ELEMS"] = shard
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    sizes = []

    def allreduce(a):
        sizes.append(a.nbytes)
        dist.all_reduce(torch.from_numpy(a))

    sc, ep, n = load_workload(workload)
    fixed0 = np.asarray(sc.fixed, dtype=bool)
    out = {}
    for tag, flags in (("off", 0), ("on", dl.FLAG_DOT_COARSE)):
        if tag == "off" and refix_part is not None:
            continue
        sc, ep, n = load_workload(workload)                          # (a fresh scripter)
        ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world, allreduce=allreduce, flags=flags)
        infos = [ts.dotCoarseInfo()[:4]]
        if flags:
            out["A0"] = ts.pcgCoarseMatrix()
        del sizes[:]                                                 # (the collectives of dotmi_create are not the loop's)
        its, halv, Es = [], [], []
        for k in range(steps):
            scripted(sc, ts)
            st = ts.step()
            its.append(st.iters); halv.append(st.ls_halvings); Es.append(st.E)
            infos.append(ts.dotCoarseInfo()[:4])
            if k == 0 and refix_part is not None:
                fixed = np.asarray(sc.fixed, dtype=np.uint8).copy()
                fixed[part_verts(sc.T, ep, n)[refix_part]] = 1
                ts.refix(fixed)
                infos.append(ts.dotCoarseInfo()[:4])
        hist = collections.Counter(sizes)
        z = ts.applyPrecond(random_free(fixed0, 3))
        out.update({f"{tag}_x": ts.getResult(), f"{tag}_v": ts.getState()[1], f"{tag}_its": its, f"{tag}_halv": halv, f"{tag}_E": Es,
                    f"{tag}_z": z, f"{tag}_infos": np.array(infos), f"{tag}_hist": np.array(sorted(hist.items())).reshape(-1, 2)})
        ts.close()
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


def run_ranks(workload, steps, shard, world, refix_part=None):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        procs = [ctx.Process(target=_worker, args=(r, world, os.path.join(d, "init"), d, workload, shard, steps, refix_part))
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
        return [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(world)]


def check_histogram(off, on, n3, nc, n_pairs, steps, shard, its_off, its_on):
    """off / on: {payload bytes: calls} of the loop's collectives without and with the flag.  The z packet grows from 8 n to
    8 (n + nc) and nothing else changes: per slot one z packet and, with the sharded element pass, one [g ; 0 ; E] packet and one
    pair of alpha_0 scalars; per refresh the factorisations' joint verdict (2 doubles) and, with the sharded Hessian only, the pairs'
    blocks; per batch of slots the agreement (9 doubles).  The start of a step sends one z packet (and one gradient packet) more"""
    zoff, zon, g, two, agree, pairs = 8 * n3, 8 * (n3 + nc), 8 * (n3 + 2), 16, 72, 8 * 36 * n_pairs
    assert len({zoff, zon, g, two, agree, pairs}) == 6
    extra = {pairs} if shard == "1" else set()
    assert set(on) == {zon if s == zoff else s for s in off} | extra, (sorted(off), sorted(on))
    assert set(off) == ({zoff, two, agree} | ({g} if shard == "1" else set())), sorted(off)
    for hist, z, its in ((off, zoff, its_off), (on, zon, its_on)):
        slots = hist[z] - steps                                       # (one z packet at the start of every step)
        assert slots >= its
        if shard == "1":
            assert hist[g] == steps + slots and hist[two] == slots + steps, hist
        else:
            assert hist[two] == steps, hist
        assert hist[agree] >= steps
    if shard == "1":
        assert on[pairs] == steps                                     # one per refresh


CASES = [(BAR4, 2, "0", 2), (BAR12, 3, "1", 3), (BUNNY, 3, "0", 2), (BUNNY, 3, "1", 2), (BAR32, 2, "1", 4)]


@pytest.mark.parametrize("workload,steps,shard,world", CASES)
def test_ranks_with_the_coarse_term_agree_and_reproduce_the_single_gpu_run(workload, steps, shard, world):
    want = plain_run(workload, steps)
    Rk = run_ranks(workload, steps, shard, world)
    sc, ep, n = load_workload(workload)
    n3, nc = 3 * sc.V_rest.shape[0], 6 * n
    n_pairs = CR.plan(sc.T, ep, n, sc.V_rest.shape[0])["sizes"][0]
    # the ranks hold the same replicated state, bit for bit, and the same whole A0
    for r in range(1, world):
        for k in ("on_x", "on_v", "on_its", "on_halv", "on_E", "on_z", "A0", "on_infos", "on_hist", "off_hist", "off_its"):
            assert np.array_equal(Rk[0][k], Rk[r][k]), (r, k)
    its, halv = Rk[0]["on_its"].tolist(), Rk[0]["on_halv"].tolist()
    err = np.abs(Rk[0]["on_x"] - want["xs"][-1]).max()
    dA = np.abs(Rk[0]["A0"] - want["A0"]).max() / np.abs(want["A0"]).max()
    print(f"{workload}, DOTMI_SHARD_ELEMS={shard}, world {world}: iterations {its} (single GPU {[c[0] for c in want['counts']]}, without "
          f"the term {Rk[0]['off_its'].tolist()}), positions {err:.2e}, A0 against the single-GPU handle's {dA:.2e} relative")
    assert Rk[0]["A0"].shape == (nc, nc) and dA <= 1e-12
    assert its == [c[0] for c in want["counts"]] and halv == [c[1] for c in want["counts"]]
    assert err < 1e-9
    # dotCoarseInfo on a rank: the dimension, active, one build per refresh
    assert Rk[0]["on_infos"].tolist() == [[nc, 0, 1, 1 + k] for k in range(steps + 1)]
    assert Rk[0]["off_infos"].tolist() == [[0, 0, 0, 0]] * (steps + 1)
    if n == 32:
        assert sum(its) <= 0.8 * int(Rk[0]["off_its"].sum())
    check_histogram(dict(Rk[0]["off_hist"].tolist()), dict(Rk[0]["on_hist"].tolist()), n3, nc, n_pairs, steps, shard,
                    int(Rk[0]["off_its"].sum()), sum(its))


# ---- 3. a subdomain dropped through dotmi_refix -----------------------------------------------------------------------------------------------
def test_subdomain_fixed_through_refix_is_dropped_on_all_ranks_and_the_steps_agree():
    want = plain_run(BAR4, 3, refix_part=0)
    Rk = run_ranks(BAR4, 3, "1", 2, refix_part=0)
    for k in ("on_x", "on_v", "on_its", "on_halv", "on_E", "on_z", "on_infos"):
        assert np.array_equal(Rk[0][k], Rk[1][k]), k
    # create, step 0, refix (subdomain 0 dropped from here on), steps 1 and 2: a build behind each
    assert Rk[0]["on_infos"].tolist() == [[24, 0, 1, 1], [24, 0, 1, 2], [24, 1, 1, 3], [24, 1, 1, 4], [24, 1, 1, 5]]
    assert [i[:4] for i in want["infos"]] == [tuple(i) for i in Rk[0]["on_infos"].tolist()]
    err = np.abs(Rk[0]["on_x"] - want["xs"][-1]).max()
    print(f"subdomain 0 fixed behind step 0: {Rk[0]['on_its'].tolist()} iterations, positions {err:.2e}")
    assert Rk[0]["on_its"].tolist() == [c[0] for c in want["counts"]] and Rk[0]["on_halv"].tolist() == [c[1] for c in want["counts"]]
    assert err < 1e-9


# ---- 4. refusals at create ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(dl.FLAG_FORCE_DIST | dl.FLAG_OWNER_EXCHANGE, "OWNER_EXCHANGE"), (dl.FLAG_GSDD, "GSDD"),
                                        (dl.FLAG_NEWTON_PCG, "NEWTON_PCG"), (dl.FLAG_LBFGS_PD, "LBFGS_PD")])
def test_flag_is_refused_at_create_with_these_flags(flags, word):
    sc, ep, n = load_workload(BAR4)
    pd = flags == dl.FLAG_LBFGS_PD
    with pytest.raises(DotmiError, match="DOTMI_FLAG_DOT_COARSE: not with DOTMI_FLAG_" + word):
        DOTTimeStepper(sc, None if pd else ep, 1 if pd else n, flags=flags | dl.FLAG_DOT_COARSE, alpha_min=1.0 if pd else 0.1)


def test_flag_is_refused_at_create_on_a_vertex_partition_and_above_256_subdomains():
    sc, ep, n = load_workload(BAR4)
    vpart = np.full(sc.V_rest.shape[0], n, dtype=np.int32)
    np.minimum.at(vpart, np.asarray(sc.T).ravel(), np.repeat(ep, 4))
    with pytest.raises(DotmiError, match="DOTMI_FLAG_DOT_COARSE: not with a vertex partition"):
        DOTTimeStepper(sc, None, n, vpart=vpart, flags=dl.FLAG_DOT_COARSE)
    sc, ep, n = load_workload("synbar:40x3x3:257")
    assert n == 257
    for flags in (dl.FLAG_DOT_COARSE, SHARDED):
        with pytest.raises(DotmiError, match="DOTMI_FLAG_DOT_COARSE: at most 256 subdomains"):
            DOTTimeStepper(sc, ep, n, flags=flags)
