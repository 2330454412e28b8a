"""Newton-PCG on sharded handles, host only (DOTMI_FLAG_NEWTON_PCG_DIST): the sharded iteration restated in numpy
(tests/pcg_sharded_reference.py) on the oracle's operators and the library's own ownership plan takes the iterations of the
single-rank restatement (tests/pcg_reference.py), the plan's row slices and subdomain ranges cover everything exactly once, and the
flag is declared."""
import os

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd.workloads import load_workload
from tests import oracle_py as O
from tests import pcg_reference as R
from tests import pcg_sharded_reference as S

CASES = [("synbar:16x5x5:4", 2), ("bunny5K_LTSS", 3)]


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def case(request):
    """the oracle two DOT steps into the script, the handles moved for the third, refactored there; b = -g; the plan of `world` ranks;
    the subdomain matrices factorised once"""
    name, world = request.param
    sc, ep, n = load_workload(name)
    cfg = sc.cfg
    orc = O.OracleSim(sc.V_rest, sc.T, cfg.YM, cfg.PR, cfg.rho, cfg.energy_id, cfg.dt, sc.fixed, sc.x0, ep, n, cfg.with_gravity)
    for _ in range(2):
        idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
        orc.move(idx, pos)
        assert orc.step().status == 0
    idx, pos = sc.scripter.step(orc.state()[0], cfg.dt)
    orc.move(idx, pos)
    x = orc.state()[0]
    orc.refactor(x)
    yield sc, ep, n, orc, orc.dup(), -orc.gradient(x), S.rank_plan(sc, ep, n, world), S.subdomain_solves(orc, n)
    orc.close()


def test_row_slices_and_subdomain_ranges_cover_everything_exactly_once(case):
    sc, ep, n, orc, dup, b, plan, solves = case
    nV = sc.V_rest.shape[0]
    rows, parts = np.zeros(nV, dtype=int), np.zeros(n, dtype=int)
    for p0, p1, v0, v1 in plan:
        assert 0 <= p0 <= p1 <= n and 0 <= v0 <= v1 <= nV
        rows[v0:v1] += 1
        parts[p0:p1] += 1
    assert (rows == 1).all() and (parts == 1).all()
    assert sum(p1 > p0 for p0, p1, _, _ in plan) >= 2               # real partial ownership
    # ... and subdomains of different ranks share vertices: the shares of S q overlap, the sum is a real one
    held = [np.unique(np.concatenate([solves[p][0] for p in range(p0, p1)])) for p0, p1, _, _ in plan if p1 > p0]
    assert np.intersect1d(held[0], held[1]).size > 0


@pytest.mark.parametrize("rel_tol", [1e-3, 1e-8])
def test_sharded_restatement_takes_the_single_rank_restatements_iterations(case, rel_tol):
    """within 1 iteration at both tolerances; at 1e-8 the true residual |b - H u| / |b| <= 2e-8 (the project's standing bounds)"""
    sc, ep, n, orc, dup, b, plan, solves = case
    _, it_ref, res_ref, state_ref = R.pcg(orc.spmv, R.m_sym(orc.apply_precond, dup), b, rel_tol, 500)
    u, it, res, state, payloads = S.pcg_sharded(orc.spmv, solves, plan, dup, b, rel_tol, 500)
    true = np.linalg.norm(b - orc.spmv(u)) / np.linalg.norm(b)
    print(f"{len(plan)} ranks, rel_tol {rel_tol:g}: {it} iterations (single-rank restatement {it_ref}), recursive {res[-1]:.3e}, true {true:.3e}")
    assert state == 1 and state_ref == 1
    assert abs(it - it_ref) <= 1
    assert res[-1] <= rel_tol
    if rel_tol == 1e-8:
        assert true <= 2e-8
    assert payloads == [(b.size, b.size + 2)] * it                  # one collective of n and one of n + 2 doubles per iteration


def test_flag_is_declared_and_collides_with_no_other():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dotmi.h")).read()
    assert dl.DOTMI_FLAG_NEWTON_PCG_DIST == 8192 and "#define DOTMI_FLAG_NEWTON_PCG_DIST 8192" in header
    flags = {k: v for k, v in vars(dl).items() if k.startswith(("FLAG_", "DOTMI_FLAG_"))}
    assert len(flags) >= 13
    assert len(set(flags.values())) == len(flags)
    for k, v in flags.items():
        assert v > 0 and v & (v - 1) == 0, k                        # one bit each
