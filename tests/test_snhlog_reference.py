"""The log-regularised Stable Neo-Hookean material (id 2) on the CPU: the 60-digit reference of tests/snhlog_reference.py against
the definition (StableNHEnergy.cpp, the SNH_WITHLOG branches), the spectral coefficients the refresh uses against the
finite-difference dP/dF, the derivation of the bound constants, and the host layers' new constant and option.  All in mpmath
or float64 numpy; nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest

from dot_amd import lib as dl
from dot_amd import scene
from tests import designed_states as D
from tests import elem_reference as R
from tests import snhlog_reference as S

mpf = R.mpf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, LAM = mpf(D.MU), mpf(D.LAM)
IDENT = [[mpf(int(i == j)) for j in range(3)] for i in range(3)]


def some_states():
    rng = np.random.default_rng(5)
    return [R.m3(np.eye(3) + 0.4 * rng.standard_normal((3, 3))) for _ in range(4)] + [R.m3(D.mesh("inverted")[2][1:4] * 0.7)]


def test_alpha_and_the_rest_state():
    """alpha = 1 + 3 mu / (4 lam); P(I) = 0 (rest-stable WITH the regulariser); Psi(I) = (lam (alpha - 1)^2 - mu log 4) / 2"""
    a = S.alpha(MU, LAM)
    assert abs(a - (1 + 3 * MU / (4 * LAM))) < mpf(10) ** -55
    psi, P = S.energy_density(IDENT, MU, LAM)
    assert max(abs(v) for row in P for v in row) < mpf(10) ** -55 * MU
    assert abs(psi - (LAM * (a - 1) ** 2 - MU * R.M.log(4)) / 2) < mpf(10) ** -55 * MU
    # and it is not the plain form's value: the two materials differ at rest already
    assert abs(psi - R.energy_density(R.SNH, IDENT, MU, LAM)[0]) > mpf("0.1") * MU


def test_stress_is_the_derivative_of_the_energy():
    """P = dPsi/dF by central differences at 60 digits (h = 1e-20: truncation and cancellation both ~1e-40)"""
    for F in some_states():
        P = S.energy_density(F, MU, LAM)[1]
        for k in range(3):
            for l in range(3):
                Fp, Fm = [r[:] for r in F], [r[:] for r in F]
                Fp[k][l] += R.FD_H
                Fm[k][l] -= R.FD_H
                fd = (S.energy_density(Fp, MU, LAM)[0] - S.energy_density(Fm, MU, LAM)[0]) / (2 * R.FD_H)
                assert abs(fd - P[k][l]) < mpf(10) ** -30 * (MU + LAM)


def test_spectral_derivatives_against_the_definition():
    """dPsi/dsigma and d2Psi/dsigma2 of the issue's lines from Psi(sigma) by central differences, in mpmath"""
    def psi(s):
        S2, J = s[0] ** 2 + s[1] ** 2 + s[2] ** 2, s[0] * s[1] * s[2]
        return (MU * (S2 - 3 - R.M.log(S2 + 1)) + LAM * (J - S.alpha(MU, LAM)) ** 2) / 2
    h = mpf(10) ** -15
    for s in ([mpf("1.3"), mpf("0.9"), mpf("0.4")], [mpf(2), mpf(2), mpf("-0.5")], [mpf(1), mpf(1), mpf(1)]):
        d, A, _ = S.spectral_coefficients(s, MU, LAM)
        for i in range(3):
            e = [h if k == i else 0 for k in range(3)]
            sp, sm = [a + b for a, b in zip(s, e)], [a - b for a, b in zip(s, e)]
            assert abs((psi(sp) - psi(sm)) / (2 * h) - d[i]) < mpf(10) ** -25 * LAM
            dp, dm = S.spectral_coefficients(sp, MU, LAM)[0], S.spectral_coefficients(sm, MU, LAM)[0]
            for j in range(3):
                assert abs((dp[j] - dm[j]) / (2 * h) - A[i][j]) < mpf(10) ** -25 * LAM


@pytest.mark.parametrize("name", D.PD_CANDIDATES)
def test_spectral_blocks_against_the_finite_difference_dPdF(name):
    """the 21 spectral entries (second derivatives, B-left, the right coefficient) on LAPACK's SVD reproduce the 60-digit
    finite-difference dP/dF of the pd_* families: float64 accuracy of a well-conditioned state (1e-12 |dP/dF|)"""
    ref = S.reference(name)
    for e in range(0, D.N_TETS, 5):
        want = S.dPdF_fd(ref["Fmp"][e], MU, LAM)
        have = S.spectral_dPdF(*D.lapack_svd(ref["F"][e]))
        assert np.abs(have - want).max() <= 1e-12 * np.abs(want).max()


def test_pd_families_qualify():
    """at least six pd_* families keep lambda_min(dP/dF) >= 0.1 mu (all twelve do; the smallest is 0.134 mu on pd_e / pd_f)"""
    low = {n: float(S.pd_min_eig(n).min()) for n in D.PD_CANDIDATES}
    print(low)
    assert sum(S.pd_mask(n).any() for n in D.PD_CANDIDATES) >= 6
    assert all(v >= 0.1 for v in low.values()) and abs(min(low.values()) - 0.134) < 1e-3


def test_mesh_reference_is_this_material():
    """the subclassed MeshRef sums this material's density (a fall-through to plain Stable Neo-Hookean would show here)"""
    name = "generic"
    V, T, x = D.mesh(name)
    ref, plain = S.reference(name), D.reference(name, R.SNH)
    for e in (0, 7, 23):
        t = S.Tet(V[T[e]], D.MU, D.LAM, D.RHO, D.DT)
        assert ref["psi_w"][e] == t.w * S.energy_density(ref["Fmp"][e], MU, LAM)[0]
        assert abs(ref["psi_w"][e] - plain["psi_w"][e]) > 1e-3 * abs(plain["psi_w"][e])
    assert np.array_equal(ref["kDm"], plain["kDm"]) and np.array_equal(ref["F"], plain["F"])


def test_constants_are_reproduced_by_the_derivation(capsys):
    """K_PSI, K_P, K_H of tests/snhlog_reference.py are 4 x the float64 / LAPACK evaluation's largest normalised error, and the
    families named there are the ones that set them"""
    k, fam = S.lapack_constants()
    with capsys.disabled():
        print(f"\nid 2 lapack constants K_PSI {k[0]:.4g} ({fam[0]}) K_P {k[1]:.4g} ({fam[1]}) K_H {k[2]:.4g} ({fam[2]})")
    for have, want in zip((S.K_PSI, S.K_P, S.K_H), k):
        assert abs(have - want) <= 0.01 * want, (have, want)
    assert fam == ("wide_10", "scale_1e3", "pd_c")


def test_abi_constant_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "dotmi.h")) as f:
        hdr = f.read()
    ids = dict(re.findall(r"#define (DOTMI_ENERGY_\w+) (\d+)", hdr))
    assert ids == {"DOTMI_ENERGY_FCR": "0", "DOTMI_ENERGY_SNH": "1", "DOTMI_ENERGY_SNH_LOG": "2"}
    assert dl.ENERGY_SNH_LOG == 2 and scene.ENERGY_SNH_LOG == 2 and S.SNH_LOG == 2


def test_config_option_stands_beside_the_script(tmp_path):
    """`snh_log` turns a script's SNH into id 2 and is an error with FCR; the parser knows no new token"""
    assert scene.Config(energy="SNH", snh_log=True).energy_id == 2
    assert scene.Config(energy="SNH").energy_id == 1 and scene.Config(energy="FCR").energy_id == 0
    with pytest.raises(ValueError):
        scene.Config(energy="FCR", snh_log=True).energy_id
    assert scene.ENERGY_NAMES == ("FCR", "SNH")
    p = tmp_path / "s.txt"
    p.write_text("energy SNH_LOG\n")
    cfg = scene.parse_script(str(p))
    assert cfg.energy == "SNH" and not cfg.snh_log      # an unknown name is the default type, as before


def test_create_refuses_energy_3():
    """dotmi_create checks for a device before its arguments, so without a GPU every create is refused with DOTMI_E_NOGPU (-4);
    with one, energy = 3 is DOTMI_E_INVALID (-1; asserted on the GPU as well, tests/test_gpu_snhlog.py)"""
    from dot_amd.timestepper import DOTTimeStepper, DotmiError
    from tests.workloads import load_workload
    sc, ep, n = load_workload("synbar:8x3x3:4")
    with pytest.raises(DotmiError) as ei:
        DOTTimeStepper(sc, ep, n, energy=3)
    assert re.search(r"failed \((-1|-4)\)", str(ei.value))
