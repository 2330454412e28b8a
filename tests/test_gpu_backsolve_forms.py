"""Every tile form of the subdomain back-solve (dot_amd/csrc/k_backsolve.hip: the packs backsolve_wave_tile_t<1,32> / <2,16>, the
256-thread backsolve_tile<256,{1,2,3,5},...> and <256,6,8,RLDS>, the 512-thread <512,{4,5},8>, the two-phase backsolve_long_kernel
with two and with three column chunks) on the factor AS STORED, component by component.

One handle per case of tests/backsolve_cases.py, in form 0 of the block solve (DOTMI_TWO_LEVEL=0), at the rest state, no step.  Every
subdomain's X_s is read back once (dotmi_part_matrix(inverse=1)); what one application of the preconditioner must compute from those
doubles is z = (sum_s X_s^T X_s r_s) / dup, and every component of the device's z is held to the a-priori rounding bound of that
expression (tests/backsolve_reference.py: derived there, no constant from a run): dense right-hand sides against a longdouble
evaluation, and unit vectors e_j for rows j picked from the job table -- first and last row of a tile, both sides of every pass
boundary, a diagonal in every column chunk of the two-phase tiles --, where a wrong or dropped entry of row j is the leading term of
its component's bound (tests/test_backsolve_reference.py shows that on the CPU: a zeroed entry leaves the bound, 50 of 50).
Which forms each case reaches is pinned on the CPU in tests/test_backsolve_reference.py.

Out of scope: the two-level form (no explicit X_s; tests/test_gpu_two_level.py), the in-loop backsolve_ctl_kernel (same tile bodies,
held to the host loop by the bit-identity tests), GSDD's per-part launch -- the only way to backsolve_tile<512,1,32> and <512,2,16>
--, and the factorisation's accuracy: nothing here asks whether X^T X = H^-1; tests/test_gpu_factor_accuracy.py does, on the
H_s the device assembled, with a bound derived the same way."""
import numpy as np
import pytest

from dot_amd.timestepper import DOTTimeStepper
from tests import backsolve_cases as BC
from tests import backsolve_reference as BR

pytestmark = pytest.mark.gpu


class Solved:
    pass


@pytest.fixture(scope="module", params=list(BC.CASES))
def solved(request):
    """the case's plan, its handle and the factors read back once"""
    c = Solved()
    c.case = request.param
    c.plan = P = BC.Plan(c.case)
    mp = pytest.MonkeyPatch()
    for k, v in dict(BC.CASES[c.case][1], DOTMI_TWO_LEVEL="0").items():
        mp.setenv(k, v)
    ts = None
    try:
        c.ts = ts = DOTTimeStepper(P.sc, P.ep, P.nparts)
        assert ts.backsolveForm() == 0
        c.Xs, c.l2gs = [], []
        for p in range(P.nparts):
            X, l2g = ts.partMatrix(p, inverse=True)
            assert np.isfinite(X).all(), (c.case, p)
            assert np.array_equal(l2g, P.verts[p])
            c.Xs.append(X)
            c.l2gs.append(l2g)
        c.nV = P.sc.V_rest.shape[0]
        c.fixed = np.asarray(P.sc.fixed, dtype=bool)
        yield c
    finally:
        if ts is not None:
            ts.close()
        mp.undo()


def worst_component(c, z, z_ref, tol, source=None):
    """(ratio, message): the component with the largest |z - z_ref| / tol (an error where tol = 0 counts as infinite), named by the
    part, tile index, form and row the job table gives it"""
    err = np.abs(z.astype(BR.LD) - z_ref).astype(np.float64).ravel()
    t = tol.ravel()
    ratio = np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err > 0, np.inf, 0.0))
    g = int(np.argmax(ratio))
    # (the component is COLUMN `row` of every tile of the part that reaches it; the tile named is the one that holds it as a row)
    where = "; ".join(f"part {p} tile {i} {form} row {row}" for p, i, form, row in c.plan.locate(g))
    msg = (f"{c.case}: vertex {g // 3} component {g % 3} ({where}): device {float(z.ravel()[g])!r}, reference {float(z_ref.ravel()[g])!r}, "
           f"|difference| {err[g]:.3e} > tol {t[g]:.3e}")
    if source is not None:
        dof, p, tl, row, why = source
        msg += f"; right-hand side e_j of part {p} tile {int(c.plan.tiles[tl, 4])} {c.plan.form[tl]} row {row} ({why})"
    return float(ratio[g]), msg


def dense_right_hand_sides(c):
    rng = np.random.default_rng(20)
    nV = c.nV
    normal = rng.standard_normal((nV, 3))
    scaled = rng.choice([-1.0, 1.0], (nV, 3)) * 10.0 ** rng.uniform(-8, 8, (nV, 1))
    sep = np.zeros(nV, dtype=bool)
    sep[c.plan.root_separator_vertices()] = True
    v = rng.standard_normal((nV, 3))
    out = {"standard normal": normal, "signs times 10^U(-8,8) per vertex": scaled, "root separator only": v * sep[:, None],
           "all but the root separator": v * ~sep[:, None]}
    for r in out.values():
        r[c.fixed] = 0.0
    return out


def test_dense_right_hand_sides_stay_inside_the_bound_in_every_component(solved):
    c = solved
    rhs = dense_right_hand_sides(c)
    z_ref, tol = BR.reference_apply(c.Xs, c.l2gs, c.nV, np.stack(list(rhs.values())))
    failures = []
    for k, (name, r) in enumerate(rhs.items()):
        z = c.ts.applyPrecond(r)
        ratio, msg = worst_component(c, z, z_ref[k], tol[k])
        zmax = float(np.abs(z_ref[k]).max())
        print(f"{c.case}, {name}: max_k |z - z_ref| / tol_k = {ratio:.3g}, max_k tol_k / max|z_ref| = "
              f"{tol[k].max() / zmax if zmax > 0 else 0.0:.3g}")
        if name == "standard normal":
            # a condition on the inputs: the bound is nowhere looser than a tenth of the 1e-9 max|p| of the whole-application tests
            assert tol[k].max() <= 1e-10 * zmax
        if name == "root separator only" and not r.any():
            assert not z.any()                              # (a subdomain too small to be split: no separator, nothing to solve)
        assert (z[tol[k] == 0.0] == 0.0).all(), f"{name}: {msg}"
        if not ratio <= 1.0:
            failures.append(f"{name}: {msg}")
    assert not failures, "\n".join(failures)


def test_unit_vectors_of_tile_edges_stay_inside_the_bound_in_every_component(solved):
    c = solved
    rows, wanted = c.plan.sweep_rows()
    assert 0 < len(rows) <= BC.MAX_APPLIES
    Z_ref, tol = BR.reference_unit_columns(c.Xs, c.l2gs, c.nV, [x[0] for x in rows])
    worst, worst_tol, failures = 0.0, 0.0, []
    r = np.zeros((c.nV, 3))
    for k, src in enumerate(rows):
        r.ravel()[src[0]] = 1.0
        z = c.ts.applyPrecond(r)                           # one dotmi_apply_precond per unit vector
        r.ravel()[src[0]] = 0.0
        ratio, msg = worst_component(c, z, Z_ref[k], tol[k], src)
        worst = max(worst, ratio)
        worst_tol = max(worst_tol, float(tol[k].max() / np.abs(Z_ref[k]).max()))
        if not ratio <= 1.0 or (z[tol[k] == 0.0] != 0.0).any():
            failures.append(msg)
    forms = sorted({str(c.plan.form[x[2]]) for x in rows})
    print(f"{c.case}, {len(rows)} unit vectors ({wanted - len(rows)} rows of fixed vertices or shared dofs left out) in {forms}: "
          f"max_k |z - z_ref| / tol_k = {worst:.3g}, max_k tol_k / max|z_ref| = {worst_tol:.3g}")
    assert not failures, f"{len(failures)} of {len(rows)} unit vectors; the first:\n" + "\n".join(failures[:5])
