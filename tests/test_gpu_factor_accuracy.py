"""The tile factorisation (dot_amd/csrc/k_tilefactor.hip, scheduled by tile_factor.hpp) against H, component by component, in every
arithmetically distinct form: one launch per level (tile_task_kernel), the dataflow launch (tile_flow_kernel with its coherent
stores), the split levels (tile_gemm_kernel on half tiles beside the diagonal tasks), each with the diagonal tiles by
wave_chol_inv16_lds / lane_chol_inv<4> / sqrt_rsqrt (DOTMI_FAST_DIAG=1) and by the one-row-per-lane wave_chol_inv<16> (0), and on
the levels form the eager groupings (DOTMI_TILE_EAGER_MIN 1 / 1000, DOTMI_TILE_EAGER_MIN_RMUL=0) and the cleared-and-filled H tiles
(DOTMI_TILE_HFILL=0).

One handle per (mesh, switch set) of tests/factor_cases.py, DOTMI_TWO_LEVEL=0; the matrices of the mesh are reached on that one handle
through updatePrecondMtrAndFactorize, setLame and setTime.  Per matrix and subdomain H_s and X_s are read back once, and:
  * H_s agrees with the oracle's to 1e-12 relative -- so that a failure below is the factorisation's;
  * every component of F = X_s H_s X_s^T - I, from the doubles read back, lies inside the a-priori bound B that
    tests/factor_reference.py derives (no constant from a run; tests/test_factor_reference.py shows on the CPU that a float64
    restatement keeps it more than a thousand times over and that a dropped product, a lost sign, a pivot root off by 2^-30 and a zeroed padding
    diagonal all leave it);
  * X_s in dissection order is Q^T: exact zeros above the diagonal and in every tile outside the symbolic pattern of Q (the identity
    padding itself is not returned by the ABI: the padding inside live 4 x 4, 16 x 16 and 64 x 64 blocks is held only through F on
    the live rows);
  * no call reported a subdomain that is not positive definite.
Scaling: rho, mu and lambda times 4^k, k = +-20, scale the free block of H_s by exactly 4^k (the identity rows of fixed vertices
stay) and must scale the free block of X_s by exactly 2^-k, bit for bit, in both diagonal forms -- sqrt_rsqrt and the rcp / sqrt of
the other base across the exponent range.
Out of scope: the two-level form (no explicit X_s; tests/test_gpu_two_level.py)."""
import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.lib import DotmiError
from dot_amd.timestepper import DOTTimeStepper
from tests import factor_cases as FC
from tests import factor_reference as FR

pytestmark = pytest.mark.gpu


class Factored:
    pass


def reach(ts, m, matrix, state):
    """bring the handle to `matrix`; state = the (mu, lambda, dt) it is in"""
    x, mu, lam, dt = m.config[matrix]
    same_lame = np.array_equal(mu, state[0]) and np.array_equal(lam, state[1])
    if same_lame and dt == state[2]:
        ts.updatePrecondMtrAndFactorize(x)
        return state
    # (the two setters refresh at the handle's own positions: the rest state, which every such matrix is built at)
    assert np.array_equal(x, m.config["rest"][0])
    if not same_lame:
        ts.setLame(mu, lam)
    if dt != state[2]:
        ts.setTime(m.sc.cfg.duration, dt)
    return mu, lam, dt


@pytest.fixture(scope="module", params=[(mesh, sw) for mesh in FC.MESHES for sw in FC.SWITCHES], ids=lambda p: f"{p[0]}-{p[1]}")
def factored(request):
    """the handle of a (mesh, switch set) taken through the mesh's matrices; H_s and X_s of every subdomain read back once each"""
    c = Factored()
    c.mesh_name, c.switches = request.param
    c.m = m = FC.mesh(c.mesh_name)
    env, c.kind = FC.SWITCHES[c.switches]
    mp = pytest.MonkeyPatch()
    for k, v in dict(env, DOTMI_TWO_LEVEL="0").items():
        mp.setenv(k, v)
    ts = None
    c.error, c.H, c.X = None, {}, {}
    try:
        ts = DOTTimeStepper(m.sc, m.ep, m.nparts)
        assert ts.backsolveForm() == 0
        c.got_kind = dl.load().dotmi_factor_kind(ts._h)
        state = (*m.base, m.sc.cfg.dt)
        try:
            for matrix in m.matrices:
                if matrix != "rest":
                    state = reach(ts, m, matrix, state)
                c.H[matrix], c.X[matrix] = [], []
                for p in range(m.nparts):
                    H, l2g = ts.partMatrix(p, inverse=False)
                    X, _ = ts.partMatrix(p, inverse=True)
                    assert np.array_equal(l2g, m.verts[p])
                    c.H[matrix].append(H)
                    c.X[matrix].append(X)
        except DotmiError as e:                  # DOTMI_E_NOTSPD of a refresh, or anything else the library refuses
            c.error = f"{matrix}: {e}"
        c.refs = FC.references(c.mesh_name, list(c.H), {k: v for k, v in c.H.items()}) if c.error is None else {}
        yield c
    finally:
        if ts is not None:
            ts.close()
        mp.undo()


def test_the_handle_is_in_the_form_the_switches_name_and_reports_no_indefinite_subdomain(factored):
    c = factored
    assert c.got_kind == c.kind
    assert c.error is None, c.error
    assert list(c.H) == list(c.m.matrices)


def test_assembled_subdomain_matrices_agree_with_the_oracle(factored):
    c = factored
    assert c.error is None, c.error
    for matrix in c.H:
        for p, (H, Ho) in enumerate(zip(c.H[matrix], c.m.oracle_H(matrix))):
            assert np.array_equal(H, H.T)
            err = np.abs(H - Ho).max() / np.abs(Ho).max()
            assert err < 1e-12, (c.mesh_name, matrix, p, err)


def eager_of(switches):
    return {"levels-eager1": "eager1", "levels-eager1000": "eager1000"}.get(switches, "default")


def test_every_component_of_the_factor_residual_lies_inside_the_a_priori_bound(factored):
    c = factored
    assert c.error is None, c.error
    failures = []
    for matrix in c.H:
        worst, bmax = 0.0, 0.0
        for p, (X, r, lay) in enumerate(zip(c.X[matrix], c.refs[matrix], c.m.layouts)):
            assert np.isfinite(X).all(), (c.mesh_name, c.switches, matrix, p)
            res = r.residual(lay.to_dissection(X))
            ratio, i, j = FR.worst(res, r.B)
            worst, bmax = max(worst, ratio), max(bmax, float(r.B.max()))
            if not ratio <= 1.0:
                ti, tj = sorted((int(lay.tile[i]), int(lay.tile[j])))
                w = FR.tile_writers(c.m.plan(p, eager_of(c.switches)), lay.nt)
                failures.append(f"{matrix}: part {p}, rows {int(lay.live_rows[i])} and {int(lay.live_rows[j])} (tile row {ti}, tile column {tj}; "
                                f"in the host-side restatement's task list the Q tile is written by {w.get(('Q', ti, tj))}, the R tile by {w.get(('R', ti, tj))}, the diagonal tiles by "
                                f"{w.get(('Q', ti, ti))} and {w.get(('Q', tj, tj))}): |F| = {res[i, j]:.3e} > B = {r.B[i, j]:.3e}")
        print(f"{c.mesh_name} {c.switches} {matrix}: max |F| / B over the subdomains = {worst:.3g}, max B = {bmax:.3g}")
    assert not failures, "\n".join(failures)


def test_the_stored_factor_is_lower_triangular_in_dissection_order_with_exact_zeros_outside_the_pattern_of_q(factored):
    c = factored
    assert c.error is None, c.error
    for matrix in c.X:
        for p, (X, lay) in enumerate(zip(c.X[matrix], c.m.layouts)):
            Xd = lay.to_dissection(X)
            bad = FR.shape_violations(Xd, lay)
            assert bad.size == 0, (c.mesh_name, c.switches, matrix, p, bad[:5].tolist(), Xd[tuple(bad[0])])
            assert (np.diag(Xd) > 0).all()
            # (the symbolic pattern holds what H_s really has: every non-zero of H_s lies in a tile of the planner's pattern)
            Hd = np.triu(lay.to_dissection(c.H[matrix][p]))
            ti, tj = lay.tile[:, None], lay.tile[None, :]
            assert not (Hd != 0)[~lay.hpat[ti, tj].astype(bool)].any()


# ---- exact scaling -------------------------------------------------------------------------------------------------------------------
def scaled_factors(k, fast_diag):
    """[(H_s, X_s, fixed scalars of the part)] of synbar:8x3x3:4 at rest with rho, mu and lambda multiplied by 4^k (exact powers of
    two; nothing under- or overflows)"""
    from dot_amd.scene import lame
    from dot_amd.workloads import load_workload
    sc, ep, n = load_workload("synbar:8x3x3:4")
    s = 4.0 ** k
    mu0, lam0 = lame(sc.cfg.YM, sc.cfg.PR)
    sc.cfg.rho = sc.cfg.rho * s
    nT = sc.T.shape[0]
    mp = pytest.MonkeyPatch()
    mp.setenv("DOTMI_TWO_LEVEL", "0")
    mp.setenv("DOTMI_FAST_DIAG", fast_diag)
    ts = None
    try:
        ts = DOTTimeStepper(sc, ep, n, mu=np.full(nT, mu0 * s), lam=np.full(nT, lam0 * s))
        out = []
        for p in range(n):
            H, l2g = ts.partMatrix(p, False)
            out.append((H, ts.partMatrix(p, True)[0], np.repeat(np.asarray(sc.fixed, dtype=bool)[l2g], 3)))
        return out
    finally:
        if ts is not None:
            ts.close()
        mp.undo()


@pytest.mark.parametrize("fast_diag", ["1", "0"])
def test_scaling_the_materials_by_powers_of_four_scales_the_factor_by_powers_of_two_bit_for_bit(fast_diag):
    """H_s as a whole is NOT homogeneous in (rho, mu, lambda): the rows of fixed vertices are rows of the identity whatever the
    materials (the stage that breaks it is the Dirichlet elimination of the assembly, by design).  Exact scaling is a true precondition
    on the free scalars, which the identity rows are decoupled from by exact zeros: there H_s must be 4^k times the unscaled block and
    X_s 2^-k times, bit for bit; the fixed rows must stay what they were."""
    base = scaled_factors(0, fast_diag)
    for k in (20, -20):
        for p, ((H0, X0, fx), (H, X, _)) in enumerate(zip(base, scaled_factors(k, fast_diag))):
            fr = ~fx
            FF, XF = np.ix_(fr, fr), np.ix_(fx, fx)
            assert np.isfinite(X).all() and np.abs(X0[FF]).max() > 0
            dH = H[FF] != H0[FF] * 4.0 ** k
            dX = X[FF] != X0[FF] * 2.0 ** -k
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = lambda A, A0: float(np.nanmax(np.where(A0 != 0, np.abs(A / A0 - 1.0), 0.0))) if A.size else 0.0
                print(f"DOTMI_FAST_DIAG={fast_diag}, k = {k}, part {p}: {int(fx.sum())} fixed scalars; free block: {int(dH.sum())} entries of H_s "
                      f"and {int(dX.sum())} of X_s off the exact scaling (largest relative deviation {rel(H[FF], H0[FF] * 4.0 ** k):.3g}, "
                      f"{rel(X[FF], X0[FF] * 2.0 ** -k):.3g})")
            assert np.array_equal(H[fx], H0[fx]) and np.array_equal(H[:, fx], H0[:, fx])
            assert np.array_equal(H[XF], np.eye(int(fx.sum())))
            assert not dH.any(), (k, p, "the free block of H_s is not exactly homogeneous in (rho, mu, lambda)")
            assert not dX.any(), (k, p)
            assert np.array_equal(X[fx], X0[fx]) and np.array_equal(X[:, fx], X0[:, fx])
