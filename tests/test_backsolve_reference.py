"""CPU checks of the reference the back-solve forms are held to on the GPU (tests/backsolve_reference.py,
tests/test_gpu_backsolve_forms.py), and of which kernel forms that GPU test reaches.

  (a) reference_apply against a 60-digit mpmath evaluation;
  (b) the tolerance is a theorem: plain float64 evaluations in four summation orders stay inside it;
  (c) it is sharp enough: one zeroed entry of a real inverse Cholesky factor violates it, 50 of 50;
  (d) it hides nothing the max-norm tests see: on synbar:24x8x8:1, max tol <= 1e-10 max|z_ref| for a standard-normal right-hand side;
  (e) the coverage table: the forms every case of the GPU test reaches, from the host-only planner (tests/backsolve_cases.py), and that
      their union is every instantiation the all-parts launch can reach.  backsolve_tile<512,1,32> and <512,2,16> take tiles only in
      GSDD's per-part launch (launch_gemv_part with maxTileLen > 3072), which no entry applies alone: out of scope here.
Every tolerance is the a-priori bound derived in tests/backsolve_reference.py; none was read off a run."""
import mpmath
import numpy as np
import pytest

from tests import backsolve_cases as BC
from tests import backsolve_reference as BR


def block_sparse_lower(n, rng, block=8):
    """random lower-triangular matrix whose rows start at the first column of a random earlier block (the shape of a stored factor)"""
    X = np.tril(rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-3, 3, (n, n)))
    for i in range(n):
        X[i, :block * rng.integers(0, i // block + 1)] = 0.0
    return X


def test_reference_apply_agrees_with_mpmath_at_60_digits():
    rng = np.random.default_rng(5)
    nV, n = 27, 60
    l2gs = [np.sort(rng.choice(nV, n // 3, replace=False)) for _ in range(3)]
    Xs = [block_sparse_lower(n, rng) for _ in l2gs]
    r = rng.standard_normal((nV, 3)) * 10.0 ** rng.uniform(-8, 8, (nV, 1))
    z, tol = BR.reference_apply(Xs, l2gs, nV, r)
    mpmath.mp.dps = 60
    zm = [mpmath.mpf(0)] * (3 * nV)
    sm = [mpmath.mpf(0)] * (3 * nV)
    dup = BR.multiplicity(l2gs, nV)
    for X, l2g in zip(Xs, l2gs):
        d = BR._dofs(l2g)
        Xm = mpmath.matrix(X.tolist())
        rs = mpmath.matrix([float(r.ravel()[k]) for k in d])
        p = Xm.T * (Xm * rs)
        Xa = Xm.apply(abs)
        s = Xa.T * (Xa * rs.apply(abs))
        for k, g in enumerate(d):
            zm[g] += p[k]
            sm[g] += s[k]
    worst = 0.0
    for g in range(3 * nV):
        if dup[g // 3] == 0:
            assert z.ravel()[g] == 0.0 and tol.ravel()[g] == 0.0
            continue
        zg, sg = zm[g] / int(dup[g // 3]), sm[g] / int(dup[g // 3])
        hi = float(z.ravel()[g])                          # the longdouble as an exact sum of two doubles
        err = abs(mpmath.mpf(hi) + mpmath.mpf(float(z.ravel()[g] - BR.LD(hi))) - zg) / sg
        worst = max(worst, float(err))
        # tol / S is the stated expression of n and dup
        c = float(BR.c_apply(n, dup[g // 3]) + BR.c_apply(n, dup[g // 3], BR.U_LD))
        assert abs(tol.ravel()[g] / float(sg) - c) <= 1e-6 * c
    print(f"reference_apply against mpmath: max |z - z_mp| / S = {worst:.2e}")
    assert worst <= 1e-17


def _float64_orders(X, r):
    """p = X^T (X r) in plain float64, four summation orders"""
    n = X.shape[0]
    out = {}
    t = np.zeros(n)
    for k in range(n):                                    # forward: column after column, then row after row
        t += X[:, k] * r[k]
    p = np.zeros(n)
    for i in range(n):
        p += t[i] * X[i]
    out["forward"] = p
    t = np.zeros(n)
    for k in range(n - 1, -1, -1):
        t += X[:, k] * r[k]
    p = np.zeros(n)
    for i in range(n - 1, -1, -1):
        p += t[i] * X[i]
    out["reversed"] = p
    p = np.zeros(n)
    for b in range(0, n, 64):                             # blocked by 64 rows: a tile's partial, then the partials' sum
        Xb = X[b:b + 64]
        p += Xb.T @ (Xb @ r)
    out["blocked by 64 rows"] = p

    def pairwise(v):                                      # (terms, n) -> pairwise sum over the terms
        while v.shape[0] > 1:
            if v.shape[0] % 2:
                v = np.vstack([v, np.zeros((1, v.shape[1]))])
            v = v[0::2] + v[1::2]
        return v[0]
    chunks = range(0, n, 128)
    t = pairwise(np.stack([pairwise((X[:, c:c + 128] * r[c:c + 128]).T) for c in chunks]))   # pairwise by column chunk
    out["pairwise by column chunk"] = pairwise(t[:, None] * X)
    return out


def test_float64_evaluations_in_four_orders_stay_inside_the_bound():
    rng = np.random.default_rng(6)
    n = 2000
    nV = n // 3 + 1
    X = block_sparse_lower(n + 1, rng, block=64)[: 3 * (n // 3), : 3 * (n // 3)]
    l2g = np.arange(X.shape[0] // 3)
    r = np.zeros((nV, 3))
    r[l2g] = rng.standard_normal((l2g.size, 3)) * 10.0 ** rng.uniform(-8, 8, (l2g.size, 1))
    z, tol = BR.reference_apply([X], [l2g], nV, r)
    d = BR._dofs(l2g)
    for name, p in _float64_orders(X, r.ravel()[d]).items():
        ratio = np.abs(p - z.ravel()[d]) / tol.ravel()[d]
        print(f"{name}: max |p - z_ref| / tol = {ratio.max():.3f}")
        assert (np.abs(p - z.ravel()[d]) <= tol.ravel()[d]).all(), name
    # two subdomains that share every vertex: the merge's division and its term of the bound
    X2 = block_sparse_lower(X.shape[0], rng, block=64)
    z, tol = BR.reference_apply([X, X2], [l2g, l2g], nV, r)
    p = (X.T @ (X @ r.ravel()[d]) + X2.T @ (X2 @ r.ravel()[d])) / 2
    assert (np.abs(p - z.ravel()[d]) <= tol.ravel()[d]).all()


@pytest.fixture(scope="module")
def bar_factor(oracle):
    """X = inv(chol(H_s)) of synbar:24x8x8:1 at rest in the subdomain's nested-dissection order, returned in ascending vertex order
    as dotmi_part_matrix returns it; H_s from the CPU oracle"""
    P = BC.Plan("24x8x8")
    sc, cfg = P.sc, P.sc.cfg
    orc = oracle.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, P.ep, 1, cfg.with_gravity)
    H = orc.part_dense(0)
    l2g = orc.part_verts(0)
    orc.close()
    assert np.array_equal(l2g, P.verts[0])
    rows = (P.pos[0][:, None] + np.arange(3)[None, :]).ravel()       # layout row of every dof
    perm = np.argsort(rows)
    Lc = np.linalg.cholesky(H[np.ix_(perm, perm)])
    Xnd = np.linalg.inv(Lc)
    # what is stored of a row: from the first column of its tree node (a separator's: of its sub-tree) to the diagonal; the rest is
    # structurally zero and comes out of the inversion as rounding noise
    first = np.zeros(P.nmax, dtype=np.int64)
    for off, size, a, c, offS, sizeS in P.nodes:
        first[(off, offS)[int(a >= 0)]:][:(size, sizeS)[int(a >= 0)]] = off
    col = np.sort(rows)
    Xnd = np.where((col[None, :] >= first[col][:, None]) & (col[None, :] <= col[:, None]), Xnd, 0.0)
    X = np.empty_like(Xnd)
    X[np.ix_(perm, perm)] = Xnd
    return P, X, l2g, rows


def test_one_zeroed_entry_of_a_real_factor_violates_the_bound(bar_factor):
    """Mutation sensitivity: zero the stored entry X[j, k] -- the first, a middle or the last entry of layout row j --, apply the
    MUTATED factor to e_j in plain float64 as the device would, and compare with the reference of the true factor: component k must
    leave the tolerance (the dropped term X_jk X_jj is the leading term of S_k)."""
    P, X, l2g, rows = bar_factor
    nV = P.sc.V_rest.shape[0]
    rng = np.random.default_rng(7)
    fixed = np.asarray(P.sc.fixed, dtype=bool)
    free = np.flatnonzero(~np.repeat(fixed[l2g], 3))
    js = rng.choice(free, 51, replace=False)
    Z, tol = BR.reference_unit_columns([X], [l2g], nV, 3 * l2g[js // 3] + js % 3)
    caught, ratios = 0, []
    for n_, j in enumerate(js):
        # the stored entries of row j, in layout order (start, middle, end of the row)
        ks = np.flatnonzero(X[j] != 0.0)
        ks = ks[np.argsort(rows[ks])]
        assert rows[ks[-1]] == rows[j]                    # lower triangular in the layout: the row ends on its diagonal
        k = (ks[0], ks[ks.size // 2], ks[-1])[n_ % 3]
        Xm = X[:, [j, k]].copy()                          # p_k = column k . column j; only X[j, k] changes
        Xm[j, 1] = 0.0
        dev = Xm[:, 1] @ (Xm[:, 0] if k != j else Xm[:, 1])
        g = 3 * l2g[k // 3] + k % 3
        err, t = abs(dev - Z[n_].ravel()[g]), tol[n_].ravel()[g]
        ratios.append(err / t)
        caught += err > t
    print(f"zeroed entries caught: {caught} of {len(js)} ({100.0 * caught / len(js):.0f} %), smallest |error| / tol = {min(ratios):.3g}")
    assert caught == len(js) >= 50


def test_the_bound_is_nowhere_looser_than_a_tenth_of_the_max_norm_tests(bar_factor):
    """A condition on the inputs of the GPU test, not a measurement of the kernels: for the standard-normal right-hand side
    max_k tol_k <= 1e-10 max|z_ref|, a tenth of the 1e-9 max|p| the whole-application tests allow."""
    P, X, l2g, rows = bar_factor
    nV = P.sc.V_rest.shape[0]
    r = np.random.default_rng(11).standard_normal((nV, 3))
    r[np.asarray(P.sc.fixed, dtype=bool)] = 0.0
    z, tol = BR.reference_apply([X], [l2g], nV, r)
    print(f"synbar:24x8x8:1, inv(chol(H_s)) from the oracle: max tol / max|z_ref| = {tol.max() / np.abs(z).max():.2e}")
    assert tol.max() <= 1e-10 * np.abs(z).max()


@pytest.fixture(scope="module")
def plans():
    return {case: BC.Plan(case) for case in BC.CASES}


@pytest.mark.parametrize("case", list(BC.CASES))
def test_forms_the_gpu_case_reaches(plans, case):
    """The coverage table, recomputed from dotmi_plan_backsolve_tiles: the set of non-empty forms and the chunk counts of the two-phase
    tiles per case (not the tile counts).  A threshold change that empties a form fails here."""
    P = plans[case]
    _, _, forms, chunks = BC.CASES[case]
    got = {str(f): int((P.form == f).sum()) for f in sorted(set(P.form))}
    print(case, got, "chunks", sorted(set(P.chunks[P.chunks > 0].tolist())), "rows per tile", sorted(set(P.tiles[:, 2].tolist())))
    assert set(got) == forms
    assert set(P.chunks[P.chunks > 0].tolist()) == chunks
    # the sweep stays under its cap without dropping a row, touches every form, and never names a fixed vertex
    rows, wanted = P.sweep_rows()
    assert len(rows) <= BC.MAX_APPLIES and len({x[0] for x in rows}) == len(rows)
    assert wanted <= BC.MAX_APPLIES                         # (the cap cuts nothing in any of today's cases)
    for f in forms:                                         # four tiles of every form, or all it has
        assert len({t for _, _, t, _, _ in rows if P.form[t] == f}) >= min(BC.TILES_PER_FORM, int((P.form == f).sum())), f
    assert not np.asarray(P.sc.fixed, dtype=bool)[[x[0] // 3 for x in rows]].any()
    for dof, p, t, row, why in rows:
        assert P.global_dof(p, row) == dof and P.tiles[t, 1] <= row < P.tiles[t, 1] + P.tiles[t, 2]
        assert (p, int(P.tiles[t, 4]), str(P.form[t]), row) in P.locate(dof)


def test_the_cases_together_reach_every_form_of_the_all_parts_launch(plans):
    reached = set().union(*(set(P.form.tolist()) for P in plans.values()))
    assert reached == BC.ALL_FORMS
    assert {2, 3} <= set().union(*(set(P.chunks[P.chunks > 0].tolist()) for P in plans.values()))
    assert any(P.nparts > 1 and np.max(BR.multiplicity(P.verts, P.sc.V_rest.shape[0])) >= 3 for P in plans.values())   # the merge
    # the switch no other GPU test sets, both ways, and a launch without packs
    assert {"DOTMI_TILE_ROWS", "DOTMI_TILE_ROWS_LONG", "DOTMI_WAVE_PACKS"} <= set().union(*(set(c[1]) for c in BC.CASES.values()))
