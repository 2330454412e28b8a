"""The log-regularised Stable Neo-Hookean material (DOTMI_ENERGY_SNH_LOG = 2) on the device, through the C ABI.

The frozen C oracle knows ids 0 and 1 only, so the parity bar is the 60-digit reference of tests/snhlog_reference.py (bounds and
constants derived there on the CPU, never measured on the kernels) and the numpy restatement of DOT's step
(tests/dot_coarse_reference.py) driven by a handle's own operators.  Shapes: the 24-tet designed-state meshes,
synbar:8x3x3:4 and synbar:16x5x5:4 (synbar:48x4x4:12 for the coarse term, whose A0 then crosses a row block)."""
import dataclasses
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd import scene
from dot_amd.timestepper import DOTTimeStepper, DotmiError
from tests import designed_states as D
from tests import dot_coarse_reference as DR
from tests import elem_reference as R
from tests import snhlog_reference as S
from tests.test_gpu_designed_states import BIT_PAIRS, LATE, crushed_start
from tests.test_gpu_materials import FORMS
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = D.EPS
BAR_S, BAR4, BAR12 = "synbar:8x3x3:4", "synbar:16x5x5:4", "synbar:48x4x4:12"


def load_log(name, script=None):
    """a workload with the variant switched on beside its `energy SNH`"""
    sc, ep, n = load_workload(name)
    assert sc.cfg.energy == "SNH"
    if script is not None:
        _, dims, _ = name.split(":")
        V, T = scene.synthetic_bar(*(int(t) for t in dims.split("x")))
        sc = scene.build_scene(dataclasses.replace(sc.cfg, script=script), V, T)
    sc.cfg.snh_log = True
    assert sc.cfg.energy_id == dl.ENERGY_SNH_LOG
    return sc, ep, n


def scripted(sc, ts, *more):
    idx, pos = sc.scripter.step(ts.getResult(), sc.cfg.dt)
    for t in (ts,) + more:
        t.setDirichlet(idx, pos)


def designed_handle(name, snh_log=True):
    V, T, x = D.mesh(name)
    cfg = scene.Config(energy="SNH", script="null", dt=D.DT, rho=D.RHO, YM=D.YM, PR=D.PR, with_gravity=False, snh_log=snh_log)
    assert scene.lame(cfg.YM, cfg.PR) == (D.MU, D.LAM)
    scn = scene.Scene(cfg=cfg, V_rest=V, T=T, scripter=scene.AnimScripter("null", V, [np.array([], dtype=np.int32)] * 2), x0=V.copy())
    ep = (np.arange(len(T)) * 4 // len(T)).astype(np.int32)
    return scn, DOTTimeStepper(scn, ep, 4), x


# ---- 1, 2. the element functions on the designed states ----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(D.FAMILIES))
def family(request):
    scn, ts, x = designed_handle(request.param)
    yield request.param, ts, x
    ts.close()


def test_energy_against_the_reference_potential(family):
    """|E - E_ref| <= K_PSI eps sum_e (dt^2 vol S_Psi + inertia scale), every family"""
    name, ts, x = family
    ref = S.reference(name)
    E = ts.computeEnergyVal(x)
    err = float(abs(R.mpf(E) - ref["E"]))
    print(f"energy id 2 {name}: err / (eps scale) {err / (EPS * ref['escale'].sum()):.3g}  (K_PSI {S.K_PSI:.3g})")
    assert np.isfinite(E) and err <= S.K_PSI * EPS * ref["escale"].sum()


def test_gradient_per_tet_against_the_reference(family):
    """max|g_e - g_ref,e| <= K_P eps kappa(Dm) scale_e per tet; on the two families without a polar factor: finite only"""
    name, ts, x = family
    g = ts.computeGradient(x)
    assert np.isfinite(g).all()
    if name in D.UNDEFINED_R:
        return
    err = S.normalised_errors(name, None, g.reshape(-1, 12))["g"]
    print(f"gradient id 2 {name}: {err.max():.3g}  (K_P {S.K_P:.3g})")
    assert err.max() <= S.K_P, (int(err.argmax()), err.max())


def test_element_hessians(family):
    """everywhere: finite, symmetric to 1e-12 |H|, smallest eigenvalue of every 12x12 >= -K_H eps |H|; on the pd_* tets where the
    projection is the identity: against the reference's finite-difference Hessian, K_H eps kappa_R kappa(Dm)^2 |H_ref|"""
    name, ts, x = family
    H = ts.computeElemHessians(x)
    assert np.isfinite(H).all()
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(H).max()
    w = np.linalg.eigvalsh((H + H.transpose(0, 2, 1)) / 2)
    hn = np.abs(w).max(axis=1)
    print(f"hessian id 2 {name}: smallest eigenvalue / (eps |H|) {(w[:, 0] / np.maximum(EPS * hn, 1e-300)).min():.3g}")
    assert (w[:, 0] >= -S.K_H * EPS * hn).all(), (w[:, 0], hn)
    if name in D.PD_CANDIDATES:
        err = S.normalised_errors(name, None, ts.computeGradient(x).reshape(-1, 12), H)["H"]
        ok = S.pd_mask(name)
        print(f"hessian id 2 {name}: {ok.sum()} PD tets, vs FD {np.nanmax(err):.3g}  (K_H {S.K_H:.3g})")
        assert ok.any() and np.nanmax(err) <= S.K_H


def test_fixed_vertices_get_exact_zeros():
    """corner 0 of every third tet fixed (dotmi_refix): exact zeros in the gradient there, every other entry within its bound;
    exact zeros in the fixed rows of H p after a refresh"""
    name = "thin_1e-3"
    scn, ts, x = designed_handle(name)
    try:
        fixed = np.zeros(len(x), dtype=np.uint8)
        fixed[::12] = 1
        fx = fixed.astype(bool)
        V, T, _ = D.mesh(name)
        x = x.copy(); x[fx] = V[fx]
        ts.refix(fixed)
        g = ts.computeGradient(x)
        assert np.abs(g[fx]).max() == 0.0
        ref = S.MeshRef(V, T, D.MU, D.LAM, D.RHO, D.DT).evaluate(x, V)
        err = R.g_err(g, ref["g"]); err[fx] = 0
        err = err.reshape(len(T), 12).max(axis=1) / (EPS * ref["kDm"] * ref["gscale"])
        print(f"gradient id 2 with fixed corners {name}: {err.max():.3g}")
        assert err.max() <= S.K_P
        # and in the Hessian the refresh assembles from this material's element Hessians: the fixed rows are the identity's, so
        # H p is exactly zero there for a p that vanishes on them
        ts.updatePrecondMtrAndFactorize()
        p = np.random.default_rng(4).standard_normal(x.shape)
        p[fx] = 0.0
        Hp = ts.multiply(p)
        assert np.abs(Hp[fx]).max() == 0.0 and np.abs(Hp[~fx]).min() > 0.0
    finally:
        ts.close()


# ---- 3. every form of the element pass, from a crushed start -----------------------------------------------------------------------------
def elastic_energy_60(sc, x):
    """sum_e dt^2 vol Psi_e at 60 digits (the closed form needs no SVD) and the bound's scale: sum_e dt^2 |vol| S_Psi with the
    singular values from LAPACK (a scale needs no more)"""
    mu, lam = scene.lame(sc.cfg.YM, sc.cfg.PR)
    X = R.MeshRef._mp(x)
    E, scale = R.mpf(0), 0.0
    for t4 in sc.T:
        t = S.Tet(sc.V_rest[t4], mu, lam, sc.cfg.rho, sc.cfg.dt)
        F = t.F([X[v] for v in t4])
        E += t.w * S.energy_density(F, t.mu, t.lam)[0]
        s = [R.mpf(float(v)) for v in np.linalg.svd(R.to_np(F), compute_uv=False)]
        scale += abs(float(t.w)) * t.scales(F, s)[3]
    return E, scale


def run_form(kind, env, flags, monkeypatch, snh_log=True):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        sc, ep, n = load_log(BAR_S)
        sc.cfg.snh_log = snh_log
        ts = DOTTimeStepper(sc, ep, n, flags=flags)
        try:
            ts.setState(crushed_start(sc, kind), np.zeros_like(sc.x0))
            out = []
            for _ in range(2):
                xt = ts.getState()[2]
                st = ts.step()
                out.append(dict(status=st.status, iters=st.iters, halvings=st.ls_halvings, g2=st.g2, E0=st.E0, x=ts.getResult(), xt=xt))
            return sc, out
        finally:
            ts.close()


@pytest.mark.parametrize("kind", ["line", "noise"])
def test_crushed_start_through_every_form(kind, monkeypatch):
    """synbar:8x3x3:4 from the two crushed starts of tests/test_gpu_designed_states.py, v = 0, two steps, every form of
    tests/test_gpu_materials.py with id 2.  The pairs that are bit-identical for the other materials are here; vertex against
    element patches take the same iterations and halvings, positions within 1e-9 (1e-6 with back-tracking).  Each form's energy at
    the start of its first step -- evaluated by the form's own kernel at x~ (v = 0: the point initX forms, where the inertia
    term vanishes) -- is the 60-digit value of THIS material and more than 1e-6 away from a plain Stable Neo-Hookean handle's:
    a dispatch that fell through to id 1 shows here."""
    runs = {form: run_form(kind, env, flags, monkeypatch)[1] for form, env, flags in FORMS + [LATE]}
    sc, plain = run_form(kind, {"DOTMI_VERTEX_PATCHES": "0"}, 0, monkeypatch, snh_log=False)
    base = runs["element-patches"]
    for form, out in runs.items():
        print(f"crushed start id 2 {kind} {form}: status {[o['status'] for o in out]} iterations {[o['iters'] for o in out]} "
              f"halvings {[o['halvings'] for o in out]} max|dx| vs element patches "
              f"{[float(np.abs(o['x'] - b['x']).max()) for o, b in zip(out, base)]}")
        assert all(np.isfinite(o["x"]).all() for o in out), form
    for form, twin in BIT_PAIRS:
        for o, b in zip(runs[form], runs[twin]):
            assert (o["iters"], o["halvings"], o["g2"]) == (b["iters"], b["halvings"], b["g2"]), (form, twin)
            assert np.array_equal(o["x"], b["x"]), (form, twin)
    quiet = all(o["halvings"] == 0 for o in base)
    for k, (o, b) in enumerate(zip(runs["vertex-patches"], base)):
        assert (o["iters"], o["halvings"]) == (b["iters"], b["halvings"]), k
        assert np.abs(o["x"] - b["x"]).max() < (1e-9 if quiet else 1e-6), k
    xt = base[0]["xt"]
    E_ref, scale = elastic_energy_60(sc, xt)
    for form, out in runs.items():
        assert np.array_equal(out[0]["xt"], xt), form
        err = float(abs(R.mpf(out[0]["E0"]) - E_ref))
        rel_plain = abs(out[0]["E0"] - plain[0]["E0"]) / abs(plain[0]["E0"])
        print(f"  {form}: E0 {out[0]['E0']:.17g}, err / (eps scale) {err / (EPS * scale):.3g} (K_PSI {S.K_PSI:.3g}), "
              f"against plain SNH {rel_plain:.3g}")
        assert err <= S.K_PSI * EPS * scale, form
        assert rel_plain > 1e-6, form
    assert np.array_equal(plain[0]["xt"], xt)


# ---- 4. the tolerance ------------------------------------------------------------------------------------------------------------------------
def test_target_gres_is_the_restatement_with_this_materials_blocks():
    """Optimizer::computeCharNormSq (Optimizer.cpp:613-651) in numpy with the id-2 spectral blocks at sigma = 1: 1e-15 relative"""
    sc, ep, n = load_log(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    plain_sc, _, _ = load_workload(BAR4)
    plain = DOTTimeStepper(plain_sc, ep, n)
    try:
        mu, lam = scene.lame(sc.cfg.YM, sc.cfg.PR)
        A, B = S.spectral_blocks(np.ones(3), mu, lam)
        # every sum in the order the reference makes it: the 1e-15 leaves no room for another
        sqH = 0.0
        for v in list(A.reshape(9)) + list(B.reshape(12)):
            sqH += v * v
        V, T = sc.V_rest, sc.T
        ls = [0.0] * len(V)
        for t in T:
            for i in range(4):
                a, b, c = V[t[(i + 1) % 4]], V[t[(i + 2) % 4]], V[t[(i + 3) % 4]]
                u, w = b - a, c - a
                cx, cy, cz = u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]
                ls[t[i]] += 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
        sql = 0.0
        for v in ls:
            sql += v * v
        nV, dtSq = len(V), sc.cfg.dt * sc.cfg.dt
        want = 1e-5 * 1e-5 * sqH * sql * float(nV - 1) / float(nV) * dtSq * dtSq
        print(f"targetGRes id 2 {ts.targetGRes:.17g} restated {want:.17g} plain SNH {plain.targetGRes:.17g}")
        assert abs(ts.targetGRes - want) <= 1e-15 * want
        assert abs(ts.targetGRes - plain.targetGRes) > 1e-3 * want
    finally:
        ts.close(); plain.close()


# ---- 5. steps against the restatement on the handle's own operators ---------------------------------------------------------------------------
class HandleOps:
    """what tests/dot_coarse_reference.DotStepper asks of an OracleSim, from a handle"""

    def __init__(self, ts):
        self.ts = ts

    def state(self):
        return self.ts.getState()

    def set_state(self, x, v, xn=None):
        self.ts.setState(x, v, xn)

    def energy(self, x):
        return self.ts.computeEnergyVal(x)

    def gradient(self, x):
        return self.ts.computeGradient(x)

    def spmv(self, p):
        return self.ts.multiply(p)

    def apply_precond(self, r):
        return self.ts.applyPrecond(r)

    def refactor(self, x):
        self.ts.updatePrecondMtrAndFactorize(x)

    @property
    def target_gres(self):
        return self.ts.targetGRes


def stretch_run(steps=4):
    sc, ep, n = load_log(BAR4, script="stretch")
    ts = DOTTimeStepper(sc, ep, n)
    counts, xs = [], []
    for _ in range(steps):
        scripted(sc, ts)
        st = ts.step()
        counts.append((st.iters, st.ls_halvings, st.status))
        xs.append(ts.getResult().copy())
    ts.close()
    return sc, ep, n, counts, xs


def test_four_stretch_steps_take_the_restatements_iterations():
    """four steps of the stretch script on synbar:16x5x5:4: the device loop against DotStepper on a second handle's operators --
    identical iterations and halvings, positions 1e-9; two device runs bit-identical; |g|^2 <= targetGRes at the end of every
    step with the gradient re-evaluated through dotmi_eval_gradient (on a third handle that runs one step behind, so that it
    still holds the step's x~ when the step's final x is evaluated)"""
    sc, ep, n, counts, xs = stretch_run()
    _, _, _, counts2, xs2 = stretch_run()
    assert counts == counts2 and all(np.array_equal(a, b) for a, b in zip(xs, xs2))
    ops = DOTTimeStepper(sc, ep, n)
    chk = DOTTimeStepper(sc, ep, n)
    try:
        fixed = np.asarray(sc.fixed, dtype=bool)
        st = DR.DotStepper(HandleOps(ops), fixed, sc.cfg.dt, (0.0, -9.80665 if sc.cfg.with_gravity else 0.0, 0.0))
        want, xr = [], []
        for k in range(4):
            scripted(sc, ops)
            r = st.step()
            want.append((r["iters"], r["halvings"], r["status"]))
            xr.append(ops.getResult().copy())
            scripted(sc, chk)
            gk = chk.computeGradient(xs[k])
            g2 = float(np.vdot(gk, gk))
            print(f"step {k}: device {counts[k]} restatement {want[k]} positions {np.abs(xs[k] - xr[k]).max():.2e} "
                  f"|g|^2 {g2:.6g} targetGRes {chk.targetGRes:.6g}")
            assert g2 <= chk.targetGRes, k
            assert chk.step().status == 0 and np.array_equal(chk.getResult(), xs[k])
        assert counts == want
        assert all(c[2] == 0 for c in counts)
        assert max(np.abs(a - b).max() for a, b in zip(xs, xr)) < 1e-9
    finally:
        ops.close(); chk.close()


# ---- 6. the other steppers and the sharded handles: one step, and H is this material's -----------------------------------------------------------
def elem_hessian_operator(sc, ts):
    """p -> (sum_e H_e + M) p from dotmi_eval_elem_hessians at the handle's positions, and the free-vertex mask"""
    x = ts.getResult()
    He = ts.computeElemHessians(x)
    mass = ts.features()[2]

    def apply(p):
        out = np.zeros_like(x)
        np.add.at(out, sc.T, np.einsum("eij,ej->ei", He, p[sc.T].reshape(len(sc.T), 12)).reshape(len(sc.T), 4, 3))
        return out + mass[:, None] * p
    return apply, ~np.asarray(sc.fixed, dtype=bool)


def refreshed_hessian_error(sc, ts, sharded_rows):
    """dotmi_spmv on the refreshed H against sum_e H_e + M on the free rows (p = 0 on fixed vertices), relative to the largest
    entry.  A handle whose Hessian rows are sharded refuses dotmi_spmv; there H u = b is solved (dotmi_solve_hessian, residual
    1e-10 |b|) and the residual taken with the element Hessians' operator -- see test_one_step_... for its bound"""
    H, free = elem_hessian_operator(sc, ts)
    p = np.random.default_rng(7).standard_normal((len(free), 3))
    p[~free] = 0.0
    if not sharded_rows:
        want = H(p)
        return np.abs(ts.multiply(p) - want)[free].max() / np.abs(want).max()
    u, _, res = ts.solveHessian(p, rel_tol=1e-10)
    assert ts.last_solve_status == 0 and res <= 1e-10
    return np.linalg.norm((H(u) - p)[free]) / np.linalg.norm(p)


def one_step(sc, ts, refresh=False, sharded_rows=False):
    scripted(sc, ts)
    st = ts.step()
    assert st.status == 0 and np.isfinite(ts.getResult()).all() and np.isfinite(st.E)
    if refresh:
        ts.updatePrecondMtrAndFactorize()
    err = refreshed_hessian_error(sc, ts, sharded_rows)
    assert err <= (1e-9 if sharded_rows else 1e-12), err
    return st, err


STEPPERS = [("newton-pcg", BAR4, dict(flags=dl.FLAG_NEWTON_PCG, alpha_min=1.0), {}, False),
            ("lbfgs-hi", BAR4, dict(flags=dl.FLAG_LBFGS_HI, alpha_min=1.0), {}, False),
            ("dot-coarse", BAR12, {}, {}, True),
            ("dist-replicated", BAR4, dict(flags=dl.FLAG_FORCE_DIST), {"DOTMI_SHARD_ELEMS": "0", "DOTMI_SHARD_HESS": "0"}, False),
            ("dist-sharded", BAR4, dict(flags=dl.FLAG_FORCE_DIST), {"DOTMI_SHARD_ELEMS": "1", "DOTMI_SHARD_HESS": "1"}, False)]


@pytest.mark.parametrize("tag,name,kw,env,coarse", STEPPERS, ids=[s[0] for s in STEPPERS])
def test_one_step_of_the_other_steppers_and_sharded_handles(tag, name, kw, env, coarse, monkeypatch):
    """one step each with id 2: status 0, finite, and the refreshed H is this material's -- dotmi_spmv against the sum of
    dotmi_eval_elem_hessians, 1e-12.  Two cases reach H differently.  Newton-PCG refreshes H in front of every solve, not behind
    the last update, so it is refreshed at the final x here (dotmi_refactor) before the comparison.  With sharded Hessian rows
    dotmi_spmv is refused; H u = b is solved to a recursive residual of 1e-10 |b| instead and the true residual taken with the
    element Hessians' operator: 1e-9 |b|, ten times the solver's own figure for the gap between a recursive and a true residual
    (eps kappa(H), far below that on 612 vertices) -- the two materials' Hessians differ by more than a tenth."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, ep, n = load_log(name)
    hi = tag == "lbfgs-hi"
    ts = DOTTimeStepper(sc, None if hi else ep, 1 if hi else n, **kw)
    try:
        if coarse:
            ts.setDotCoarse(1)
        st, err = one_step(sc, ts, refresh=tag == "newton-pcg", sharded_rows=tag == "dist-sharded")
        print(f"id 2 {tag} {name}: {st.iters} iterations, {st.ls_halvings} halvings, H p against the element Hessians {err:.2e}")
        if coarse:
            assert ts.dotCoarseInfo()[2] == 1
    finally:
        ts.close()


def _rank_worker(rank, world, initfile, outdir):
    sys.path.insert(0, ROOT)
    os.environ["OMP_NUM_THREADS"] = "2"
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    sc, ep, n = load_log(BAR4)
    ts = DOTTimeStepper(sc, ep, n, device=0, rank=rank, world=world, allreduce=lambda a: dist.all_reduce(torch.from_numpy(a)))
    st, err = one_step(sc, ts)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), x=ts.getResult(), counts=[st.iters, st.ls_halvings], E=st.E, err=err)
    ts.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_through_the_host_hook():
    """two processes, world 2, the collectives through the host all-reduce hook: the ranks hold the same bits and took the
    single-GPU run's iterations and halvings"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with tempfile.TemporaryDirectory() as d:
        procs = [ctx.Process(target=_rank_worker, args=(r, 2, os.path.join(d, "init"), d)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=300)
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.terminate()
        assert not alive, "a rank hung"
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
        res = [dict(np.load(os.path.join(d, f"rank{r}.npz"))) for r in range(2)]
    for k in ("x", "counts", "E"):
        assert np.array_equal(res[0][k], res[1][k]), k
    sc, ep, n = load_log(BAR4)
    ts = DOTTimeStepper(sc, ep, n)
    try:
        st, _ = one_step(sc, ts)
        print(f"id 2 two ranks: {list(res[0]['counts'])}, single GPU {[st.iters, st.ls_halvings]}, "
              f"positions {np.abs(res[0]['x'] - ts.getResult()).max():.2e}")
        assert list(res[0]["counts"]) == [st.iters, st.ls_halvings]
    finally:
        ts.close()


# ---- 7. dotmi_set_lame ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vp", ["1", "0"], ids=["vertex-patches", "element-patches"])
def test_set_lame_equals_a_handle_created_with_the_values(vp, monkeypatch):
    monkeypatch.setenv("DOTMI_VERTEX_PATCHES", vp)
    sc, ep, n = load_log(BAR4)
    rng = np.random.default_rng(2)
    mu0, lam0 = scene.lame(sc.cfg.YM, sc.cfg.PR)
    mu = mu0 * (0.5 + rng.random(len(sc.T)))
    lam = lam0 * (0.5 + rng.random(len(sc.T)))
    a = DOTTimeStepper(sc, ep, n)
    b = DOTTimeStepper(sc, ep, n, mu=mu, lam=lam)
    try:
        x = sc.x0 + 0.01 * rng.standard_normal(sc.x0.shape)
        before = a.computeEnergyVal(x)
        a.setLame(mu, lam)
        assert a.computeEnergyVal(x) == b.computeEnergyVal(x) != before
        assert np.array_equal(a.computeGradient(x), b.computeGradient(x))
        assert np.array_equal(a.computeElemHessians(x), b.computeElemHessians(x))
        assert a.targetGRes == b.targetGRes
        # and through the loop's own kernels (the form under test): one step each, the same bits
        for t in (a, b):
            scripted(sc, t)
        sa, sb = a.step(), b.step()
        assert (sa.status, sa.iters, sa.ls_halvings, sa.E0, sa.E) == (sb.status, sb.iters, sb.ls_halvings, sb.E0, sb.E)
        assert sa.status == 0 and np.array_equal(a.getResult(), b.getResult())
    finally:
        a.close(); b.close()


# ---- 8. refusals and the runner ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    sc, ep, n = load_log(BAR_S)
    with pytest.raises(DotmiError, match=r"failed \(-1\)"):
        DOTTimeStepper(sc, ep, n, energy=3)
    with pytest.raises(DotmiError, match=r"failed \(-1\)"):
        DOTTimeStepper(sc, ep, n, energy=-1)
    sc.cfg.energy = "FCR"
    with pytest.raises(ValueError):
        DOTTimeStepper(sc, ep, n)


def test_headless_runner_takes_snh_log(tmp_path):
    """dot_hip --snh-log on a small SNH script: steps, config.txt echoes `energy SNH` (the variant is no script token), the
    energies differ from the run without the option; with an FCR script the option is an error"""
    from tests.test_host_logic import _write_msh
    exe = os.path.join(ROOT, "dot_amd", "dot_hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "dot_amd", "host")])
    V, T = scene.synthetic_bar(8, 3, 3)
    _write_msh(tmp_path / "bar.msh", V, T)
    text = "energy SNH\ntimeStepper DOT 4\nwarmStart 2\nsize 1\ntime 5 0.025\ndensity 1000\nstiffness 100000 0.4\nscript stretch\nshape input bar.msh\n"
    (tmp_path / "bar.txt").write_text(text)
    (tmp_path / "bar_fcr.txt").write_text(text.replace("energy SNH", "energy FCR"))
    E = {}
    for tag, extra in (("plain", []), ("log", ["--snh-log"])):
        res = subprocess.run([exe, "100", str(tmp_path / "bar.txt"), "--mesh-root", str(tmp_path), "--frames", "2", "--out",
                              str(tmp_path / tag)] + extra, capture_output=True, timeout=300)
        assert res.returncode == 0, res.stderr.decode()
        frames = [l.split() for l in res.stdout.decode().splitlines() if l.startswith("FRAME")]
        assert len(frames) == 2 and all(f[-1] == "0" for f in frames)
        E[tag] = float(frames[-1][frames[-1].index("E") + 1])
        cfg = (tmp_path / tag / "config.txt").read_text().splitlines()
        assert "energy SNH" in cfg and not any("LOG" in l.upper() for l in cfg)
    assert abs(E["log"] - E["plain"]) > 1e-6 * abs(E["plain"])
    bad = subprocess.run([exe, "100", str(tmp_path / "bar_fcr.txt"), "--mesh-root", str(tmp_path), "--snh-log", "--dump-scene", "0"],
                         capture_output=True, timeout=300)
    assert bad.returncode == 1 and b"--snh-log" in bad.stderr
