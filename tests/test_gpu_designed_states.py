"""The element kernels on designed deformation states (tests/designed_states.py) against the 60-digit reference
(tests/elem_reference.py), through the C ABI.  Handles are created at the rest state; only the dotmi_eval_* entries see the
designed positions.  The bounds and their three constants are those of tests/designed_states.py: 4 x what a float64
evaluation on LAPACK's SVD reaches, never anything measured on the kernels.  Today's tolerances are named where used:
1e-12 (symmetry) and 1e-10 (per-tet agreement with the oracle) of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from dot_amd import scene
from dot_amd.timestepper import DOTTimeStepper
from tests import designed_states as D
from tests import elem_reference as R
from tests import oracle_py as O
from tests.test_gpu_materials import FORMS
from tests.workloads import load_workload

pytestmark = pytest.mark.gpu

MATS = [(R.FCR, "FCR"), (R.SNH, "SNH")]
EPS = D.EPS


def make_pair(name, ename):
    V, T, x = D.mesh(name)
    cfg = scene.Config(energy=ename, script="null", dt=D.DT, rho=D.RHO, YM=D.YM, PR=D.PR, with_gravity=False)
    assert scene.lame(cfg.YM, cfg.PR) == (D.MU, D.LAM)
    scn = scene.Scene(cfg=cfg, V_rest=V, T=T, scripter=scene.AnimScripter("null", V, [np.array([], dtype=np.int32)] * 2), x0=V.copy())
    ep = (np.arange(len(T)) * 4 // len(T)).astype(np.int32)
    ts = DOTTimeStepper(scn, ep, 4)
    orc = O.OracleSim(V, T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, scn.fixed, V.copy(), ep, 4, False)
    return scn, ts, orc, x


@pytest.fixture(scope="module", params=[(m, e, n) for m, e in MATS for n in D.FAMILIES], ids=lambda p: f"{p[1]}-{p[2]}")
def family(request):
    mat, ename, name = request.param
    scn, ts, orc, x = make_pair(name, ename)
    yield mat, ename, name, scn, ts, orc, x
    ts.close(); orc.close()


def test_energy_against_the_reference_potential(family):
    """|E - E_ref| <= K_PSI eps sum_e (dt^2 vol S_Psi + inertia scale): every family, the two without a polar factor included"""
    mat, ename, name, scn, ts, orc, x = family
    ref = D.reference(name, mat)
    E = ts.computeEnergyVal(x)
    err = float(abs(R.mpf(E) - ref["E"]))
    bound = D.K_PSI * EPS * ref["escale"].sum()
    print(f"energy {ename} {name}: err / (eps scale) {err / (EPS * ref['escale'].sum()):.3g}  (K_PSI {D.K_PSI:.3g})")
    assert np.isfinite(E) and err <= bound


def test_gradient_per_tet_against_the_reference(family):
    """max|g_e - g_ref,e| <= K_P eps kappa_R kappa(Dm) scale_e per tet (Stable Neo-Hookean, whose closed form has no polar
    factor: without kappa_R).  On the two families where R is not defined: finite only."""
    mat, ename, name, scn, ts, orc, x = family
    g = ts.computeGradient(x)
    assert np.isfinite(g).all()
    if name in D.UNDEFINED_R:
        return
    err = D.normalised_errors(name, mat, None, g.reshape(-1, 12))["g"]
    erro = D.normalised_errors(name, mat, None, orc.gradient(x).reshape(-1, 12))["g"]
    print(f"gradient {ename} {name}: device {err.max():.3g} oracle {erro.max():.3g}  (K_P {D.K_P:.3g})")
    assert err.max() <= D.K_P, (int(err.argmax()), err.max())


@pytest.mark.parametrize("mat,ename", MATS, ids=[m[1] for m in MATS])
def test_fixed_vertices_get_exact_zeros(mat, ename):
    """corner 0 of every third tet fixed (dotmi_refix): exact zeros there, every other entry still within its bound"""
    name = "thin_1e-3"
    scn, ts, orc, x = make_pair(name, ename)
    try:
        fixed = np.zeros(len(x), dtype=np.uint8)
        fixed[::12] = 1
        x = x.copy(); x[fixed.astype(bool)] = D.mesh(name)[0][fixed.astype(bool)]     # fixed vertices sit at their rest position
        ts.refix(fixed)
        g = ts.computeGradient(x)
        assert np.abs(g[fixed.astype(bool)]).max() == 0.0
        V, T, _ = D.mesh(name)
        ref = R.MeshRef(V, T, D.MU, D.LAM, D.RHO, D.DT, mat).evaluate(x, V)
        kR = ref["kR"] if mat == R.FCR else np.ones(len(T))
        err = R.g_err(g, ref["g"]); err[fixed.astype(bool)] = 0
        err = err.reshape(len(T), 12).max(axis=1) / (EPS * kR * ref["kDm"] * ref["gscale"])
        print(f"gradient with fixed corners {ename} {name}: {err.max():.3g}")
        assert err.max() <= D.K_P
    finally:
        ts.close(); orc.close()


def test_element_hessians(family):
    """(a) where the projection is the identity (every eigenvalue of the reference's dP/dF >= 0.1 mu): against the
    finite-difference Hessian of the reference, K_H eps kappa_R kappa(Dm)^2 |H_ref|.
    (b) everywhere: finite; symmetric to 1e-12 |H| (today's bound); smallest eigenvalue of every 12x12 >= -K_H eps |H|, the
    projection's one promise; and today's 1e-10 per-tet agreement with the oracle -- except with two small singular values
    (sigma_1 <= 1e-2 sigma_0), where the oracle's squared-matrix SVD is the inaccurate side (its gradient error there is
    printed by test_gradient_per_tet_against_the_reference), and on the two families without a polar factor."""
    mat, ename, name, scn, ts, orc, x = family
    H = ts.computeElemHessians(x)
    n = len(H)
    assert np.isfinite(H).all()
    assert np.abs(H - H.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(H).max()
    w = np.linalg.eigvalsh((H + H.transpose(0, 2, 1)) / 2)
    hn = np.abs(w).max(axis=1)
    assert (w[:, 0] >= -D.K_H * EPS * hn).all(), (w[:, 0] / (EPS * hn)).min()
    Ho = orc.elem_hessians(x)
    vs_oracle = np.abs(H - Ho).reshape(n, -1).max(axis=1) / np.abs(Ho).reshape(n, -1).max(axis=1)
    print(f"hessian {ename} {name}: device vs oracle {vs_oracle.max():.3g}")
    if not D.two_small(name) and name not in D.UNDEFINED_R:
        assert vs_oracle.max() < 1e-10, (int(vs_oracle.argmax()), vs_oracle.max())
    if name in D.PD_CANDIDATES:
        err = D.normalised_errors(name, mat, None, ts.computeGradient(x).reshape(-1, 12), H)["H"]
        erro = D.normalised_errors(name, mat, None, orc.gradient(x).reshape(-1, 12), Ho)["H"]
        ok = D.pd_mask(name, mat)
        print(f"hessian {ename} {name}: {ok.sum()} PD tets, vs FD device {np.nanmax(err):.3g} oracle {np.nanmax(erro):.3g}  (K_H {D.K_H:.3g})")
        assert not ok.any() or np.nanmax(err) <= D.K_H


@pytest.mark.parametrize("mat,ename", MATS, ids=[m[1] for m in MATS])
def test_at_least_six_families_qualify_for_the_finite_difference_check(mat, ename):
    assert sum(D.pd_mask(n, mat).any() for n in D.PD_CANDIDATES) >= 6


# ---- the fused forms, which only the loop reaches: a crushed start -------------------------------------------------------
# What the suite holds bit-identical on tame states, pair by pair (a form, the form it must reproduce bit for bit):
# paired trials against unpaired on the same patches (tests/test_gpu_round5.py, tests/test_gpu_round6.py), the speculative
# unit step against the element patches it works on (tests/test_gpu_round6.py), the host loop against the device loop in the host loop's order
# of operations, DOTMI_EARLY_BACKSOLVE=0 (test_device_loop_control_is_bit_identical_to_host_loop).  Vertex against element
# patches group their sums differently: same decisions, positions to 1e-9 without back-tracking and 1e-6 with
# (test_vertex_patches_take_the_element_patches_steps) -- today's bounds.
LATE = ("late-backsolve", {"DOTMI_EARLY_BACKSOLVE": "0"}, 0)
BIT_PAIRS = (("pair-trials-element", "element-patches"), ("pair-trials-vertex", "vertex-patches"), ("spec-step", "element-patches"),
             ("host-loop", "late-backsolve"))


def crushed_start(sc, kind):
    x = sc.x0.copy()
    free = ~sc.fixed.astype(bool)
    if kind == "line":
        # every free vertex to 1e-3 of its distance from the bar's axis in y and z: every tet close to a line
        c = (sc.V_rest.min(axis=0) + sc.V_rest.max(axis=0)) / 2
        x[free, 1:] = c[1:] + 1e-3 * (x[free, 1:] - c[1:])
    else:
        T = sc.T
        edges = np.concatenate([np.linalg.norm(sc.V_rest[T[:, a]] - sc.V_rest[T[:, b]], axis=1)
                                for a in range(4) for b in range(a + 1, 4)])
        noise = 0.3 * edges.mean() * np.random.default_rng(3).standard_normal(x.shape)
        x[free] += noise[free]
    return x


def run_form(energy, kind, env, flags, monkeypatch):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        sc, ep, n = load_workload("synbar:8x3x3:4")
        sc.cfg.energy = energy
        ts = DOTTimeStepper(sc, ep, n, flags=flags)
        try:
            ts.setState(crushed_start(sc, kind), np.zeros_like(sc.x0))
            out = []
            for _ in range(2):
                xt = ts.getState()[2]
                st = ts.step()
                out.append(dict(status=st.status, iters=st.iters, halvings=st.ls_halvings, g2=st.g2, x=ts.getResult(), xt=xt))
            return sc, ep, n, out, ts.targetGRes
        finally:
            ts.close()


@pytest.mark.parametrize("kind", ["line", "noise"])
@pytest.mark.parametrize("energy", ["FCR", "SNH"])
def test_crushed_start_through_every_form(energy, kind, monkeypatch):
    """synbar:8x3x3:4 started (i) squashed to a line (sigma ~ (1, 1e-3, 1e-3) in every tet: the thin families inside the
    loop's kernels) and (ii) from rest + 0.3 (mean edge) N(0,1) (seed 3: 83 of 432 tets inverted, min J = -3.3), v = 0, two steps, in the forms of
    tests/test_gpu_materials.py.  The forms the suite holds bit-identical on tame states return the same bits here; the
    sharded form the same iterations and positions to 1e-9; status 0; and the 60-digit gradient at the returned x meets the
    stopping test the step claims.  Iterations against the oracle are printed, not asserted: it shares svd3's old weakness."""
    runs = {form: run_form(energy, kind, env, flags, monkeypatch) for form, env, flags in FORMS + [LATE]}
    sc, ep, n, base, target = runs["element-patches"]
    mat = R.FCR if energy == "FCR" else R.SNH
    for form, (_, _, _, out, _) in runs.items():
        print(f"crushed start {energy} {kind} {form}: status {[o['status'] for o in out]} iterations {[o['iters'] for o in out]} "
              f"halvings {[o['halvings'] for o in out]} max|dx| vs element patches "
              f"{[float(np.abs(o['x'] - b['x']).max()) for o, b in zip(out, base)]}")
    for form, (_, _, _, out, _) in runs.items():
        for k in range(2):
            assert out[k]["status"] == 0 and out[k]["g2"] <= target, (form, k)
    for form, twin in BIT_PAIRS:
        for o, b in zip(runs[form][3], runs[twin][3]):
            assert (o["iters"], o["halvings"], o["g2"]) == (b["iters"], b["halvings"], b["g2"]), (form, twin)
            assert np.array_equal(o["x"], b["x"]), (form, twin)
    quiet = all(o["halvings"] == 0 for o in base)
    for k, (o, b) in enumerate(zip(runs["vertex-patches"][3], base)):
        assert (o["iters"], o["halvings"]) == (b["iters"], b["halvings"]), k
        assert np.abs(o["x"] - b["x"]).max() < (1e-9 if quiet else 1e-6), k
    for k, (o, b) in enumerate(zip(runs["sharded"][3], base)):          # (the sharded element pass works on element patches)
        assert o["iters"] == b["iters"], k
        assert np.abs(o["x"] - b["x"]).max() < 1e-9, k
    dflt = runs["default"][3]
    cfg = sc.cfg
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)
    orc.set_state(crushed_start(sc, kind), np.zeros_like(sc.x0))
    so = [orc.step() for _ in range(2)]
    orc.close()
    print(f"crushed start {energy} {kind}: iterations {[o['iters'] for o in base]} (default form {[o['iters'] for o in dflt]}), "
          f"oracle {[s.iters for s in so]} status {[s.status for s in so]}")
    mu, lam = scene.lame(cfg.YM, cfg.PR)
    mref = R.MeshRef(sc.V_rest, sc.T, mu, lam, cfg.rho, cfg.dt, mat)
    free = ~sc.fixed.astype(bool)
    for form in ("element-patches", "default"):
        for k, o in enumerate(runs[form][3]):
            ref = mref.evaluate(o["x"], o["xt"])
            g = R.g_to_np(ref["g"])[free]
            kR = ref["kR"] if mat == R.FCR else np.ones(len(sc.T))
            slack = np.linalg.norm(D.K_P * EPS * kR * ref["kDm"] * ref["gscale"])
            print(f"  {form} step {k}: |g_ref| {np.linalg.norm(g):.6g}  sqrt(targetGRes) {np.sqrt(target):.6g}  slack {slack:.3g}")
            assert np.linalg.norm(g) <= np.sqrt(target) + slack, (form, k)
