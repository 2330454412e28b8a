"""The 60-digit element reference (tests/elem_reference.py) checked against itself, the constants of the bounds checked
against their definition, and dot_amd/csrc/elem_math.hpp -- which compiles for the host -- held to those bounds on every
designed family (tests/designed_states.py) without a GPU.  The kernels themselves: tests/test_gpu_designed_states.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import designed_states as D
from tests import elem_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
mpf = R.mpf
MATS = [(R.FCR, "FCR"), (R.SNH, "SNH")]


# ---- the reference against itself ----------------------------------------------------------------------------------------
def _states():
    rng = np.random.default_rng(5)
    shapes = D.REST_SHAPES
    return [(shapes[k % 3], shapes[k % 3] @ (np.eye(3) + a * rng.standard_normal((3, 3))).T + rng.standard_normal(3))
            for k, a in enumerate((1e-3, 0.3, 0.6, 1.2))]


def _digits(a, b, scale):
    err = max(abs(u - v) for u, v in zip(a, b))
    return 99.0 if err == 0 else float(-R.M.log10(err / scale))


def _central(f, x, h):
    """central differences of f (a list of mpf) over the 12 coordinates of x: -> cols[j][r] = d f_r / d x_j"""
    cols = []
    for k in range(4):
        for c in range(3):
            xp = [r[:] for r in x]; xm = [r[:] for r in x]
            xp[k][c] += h; xm[k][c] -= h
            cols.append([(a - b) / (2 * h) for a, b in zip(f(xp), f(xm))])
    return cols


@pytest.mark.parametrize("mat,_", MATS, ids=[m[1] for m in MATS])
def test_gradient_is_the_derivative_of_the_energy_and_hessian_of_the_gradient(mat, _):
    """to >= 25 digits: the gradient against central differences of the energy (h = 1e-20), and the Hessian -- itself a central
    difference with h = 1e-20 -- along a direction against a difference of the gradient with another step (h = 1e-15)"""
    d = [[mpf(int(v)) for v in row] for row in np.random.default_rng(1).integers(-3, 4, (4, 3))]
    for X4, x4 in _states():
        t = R.Tet(X4, D.MU, D.LAM, D.RHO, D.DT)
        x = R.MeshRef._mp(x4)
        g = t.elastic(mat, x)[1]
        fd = [c[0] for c in _central(lambda y: [t.elastic(mat, y)[0]], x, R.FD_H)]
        assert _digits(fd, g, max(abs(v) for v in g)) >= 25
        cols = _central(lambda y: t.elastic(mat, y)[1], x, R.FD_H)
        Hd = [sum(cols[j][r] * d[j // 3][j % 3] for j in range(12)) for r in range(12)]
        h2 = mpf(10) ** -15
        gp = t.elastic(mat, [[x[k][c] + h2 * d[k][c] for c in range(3)] for k in range(4)])[1]
        gm = t.elastic(mat, [[x[k][c] - h2 * d[k][c] for c in range(3)] for k in range(4)])[1]
        assert _digits(Hd, [(a - b) / (2 * h2) for a, b in zip(gp, gm)], max(abs(v) for v in Hd)) >= 25
        H = t.hessian_fd(mat, x)            # what the tests use: the same differences, rounded to double
        assert np.array_equal(H, np.array([[float(cols[j][r]) for j in range(12)] for r in range(12)]))
        assert np.abs(H - H.T).max() <= 1e-15 * np.abs(H).max()


@pytest.mark.parametrize("mat,_", MATS, ids=[m[1] for m in MATS])
def test_objectivity(mat, _):
    """Psi(QF) = Psi(F), P(QF) = Q P(F) for a rotation Q, to >= 40 digits"""
    c, s = R.M.cos(mpf("0.7")), R.M.sin(mpf("0.7"))
    c2, s2 = R.M.cos(mpf("-1.9")), R.M.sin(mpf("-1.9"))
    Q = R.mul([[c, -s, 0], [s, c, 0], [0, 0, 1]], [[1, 0, 0], [0, c2, -s2], [0, s2, c2]])
    mu, lam = mpf(D.MU), mpf(D.LAM)
    for X4, x4 in _states():
        F = R.Tet(X4, D.MU, D.LAM, D.RHO, D.DT).F(R.MeshRef._mp(x4))
        psi, P, _ = R.energy_density(mat, F, mu, lam)
        psiQ, PQ, _ = R.energy_density(mat, R.mul(Q, F), mu, lam)
        QP = R.mul(Q, P)
        scale = max(abs(v) for row in P for v in row)
        assert _digits([psiQ], [psi], max(abs(psi), mpf(1))) >= 40
        assert _digits([v for row in PQ for v in row], [v for row in QP for v in row], scale) >= 40


def test_longdouble_snh_helpers_agree_with_the_reference():
    """snh_energy_extended / snh_gradient_extended of tests/test_gpu_parity.py (numpy longdouble) against the 60-digit
    reference, to 1e-17 of the scale, on a designed family with inverted and skewed tets"""
    from types import SimpleNamespace
    from tests.test_gpu_parity import snh_energy_extended, snh_gradient_extended
    V, T, x = D.mesh("noise_0.5")
    ref = D.reference("noise_0.5", R.SNH)
    # the helpers read A, vol, mass and x~ from a handle and YM, PR, dt from the scene: hand them the reference's, in longdouble
    LD = np.longdouble
    tets = R.MeshRef(V, T, D.MU, D.LAM, D.RHO, D.DT, R.SNH)

    def ld(v):          # mpf -> longdouble in two pieces (hi + lo)
        hi = float(v)
        return LD(hi) + LD(float(v - mpf(hi)))
    Ald = np.array([[[ld(v) for v in row] for row in t.DmInv] for t in tets.tets]).reshape(len(T), 9)
    vol = np.array([ld(t.vol) for t in tets.tets])
    mass = np.array([ld(m) for m in tets.mass])
    ts = SimpleNamespace(features=lambda: (Ald, vol, mass), getState=lambda: (None, None, V))
    sc = SimpleNamespace(cfg=SimpleNamespace(YM=D.YM, PR=D.PR, dt=D.DT), T=T, fixed=np.zeros(len(V), dtype=np.uint8))
    mu, lam = np.full(len(T), D.MU), np.full(len(T), D.LAM)
    g = snh_gradient_extended(sc, ts, x, mu, lam)
    gref = R.g_to_np(ref["g"])
    assert np.abs(g - gref).max() <= 1e-17 * np.abs(gref).max() + np.abs(np.spacing(gref)).max()   # + the final rounding to double
    E = snh_energy_extended(sc, ts, x, mu, lam)
    assert abs(E - float(ref["E"])) <= 1e-17 * abs(E) + np.spacing(E)


# ---- the constants ---------------------------------------------------------------------------------------------------------
def test_constants_are_four_times_the_lapack_errors(capsys):
    """K_PSI, K_P, K_H written at the top of tests/designed_states.py are 4 x the largest normalised error of the float64
    evaluation on numpy.linalg.svd against the 60-digit reference over all asserted families (+- 1 %)"""
    k = D.lapack_constants()
    with capsys.disabled():
        print(f"\nlapack constants K_PSI {k[0]:.4g} K_P {k[1]:.4g} K_H {k[2]:.4g}")
    for have, want in zip((D.K_PSI, D.K_P, D.K_H), k):
        assert abs(have - want) <= 0.01 * want, (have, want)
    for mat, _ in MATS:
        assert sum(D.pd_mask(n, mat).any() for n in D.PD_CANDIDATES) >= 6
    assert len(D.UNDEFINED_R) <= 2 and min(len(D.mesh(n)[1]) for n in D.FAMILIES) >= 24


# ---- elem_math.hpp on the host -----------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "elem_math.hpp"
using namespace dotmi;
template <int MAT>
static void run(const Mat3 &F, double mu, double lam)
{
    Mat3 U, V, A;
    double S[3], d[3], B[3][4];
    svd3(F, U, S, V);
    dpsi<MAT>(S, mu, lam, d);
    spectral_blocks<MAT>(S, mu, lam, 1.0, false, A, B);
    for (int i = 0; i < 9; ++i) printf("%a ", U.m[i / 3][i % 3]);
    for (int i = 0; i < 3; ++i) printf("%a ", S[i]);
    for (int i = 0; i < 9; ++i) printf("%a ", V.m[i / 3][i % 3]);
    printf("%a ", psi<MAT>(S, mu, lam));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            printf("%a ", U.m[r][0] * d[0] * V.m[c][0] + U.m[r][1] * d[1] * V.m[c][1] + U.m[r][2] * d[2] * V.m[c][2]);
    for (int i = 0; i < 9; ++i) printf("%a ", A.m[i / 3][i % 3]);
    for (int i = 0; i < 12; ++i) printf("%a ", B[i / 4][i % 4]);
    printf("\n");
}
int main()
{
    int mat;
    double mu, lam;
    Mat3 F;
    while (scanf("%d %la %la", &mat, &mu, &lam) == 3) {
        for (int i = 0; i < 9; ++i)
            if (scanf("%la", &F.m[i / 3][i % 3]) != 1) return 1;
        if (mat == 0) run<0>(F, mu, lam);
        else run<1>(F, mu, lam);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    """svd3 / psi / dpsi / spectral_blocks of elem_math.hpp compiled for the host with the flags of dot_amd/csrc/Makefile;
    -> f(mat, F (n,3,3)) -> dict of arrays"""
    if HIPCC is None:
        pytest.skip("hipcc is not installed")
    d = tmp_path_factory.mktemp("host_twin")
    (d / "driver.hip").write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-unused-result",
                           "-I", os.path.join(ROOT, "dot_amd", "csrc"), str(d / "driver.hip"), "-o", str(exe)])

    def run(mat, F):
        text = "".join(" ".join([str(mat), float(D.MU).hex(), float(D.LAM).hex()] + [float(v).hex() for v in f.reshape(9)]) + "\n"
                       for f in F)
        out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode()
        a = np.array([[float.fromhex(t) for t in line.split()] for line in out.splitlines()])
        assert a.shape == (len(F), 52)
        return dict(U=a[:, 0:9].reshape(-1, 3, 3), S=a[:, 9:12], V=a[:, 12:21].reshape(-1, 3, 3), psi=a[:, 21],
                    P=a[:, 22:31].reshape(-1, 3, 3), A=a[:, 31:40].reshape(-1, 3, 3), B=a[:, 40:52].reshape(-1, 3, 4))
    return run


def host_twin_errors(run, name, mat):
    """normalised errors of the host twin on the rounded-to-double F of every tet of the family, against the reference
    re-evaluated on exactly those F: sigma / (eps s0), Psi / (eps S_Psi), P / (eps kappa_R S_P), and -- where the projection
    is idle -- dP/dF assembled from spectral_blocks / (eps kappa_R max|dP/dF|)"""
    F = D.reference(name, mat)["F"]
    got = run(mat, F)
    mu, lam = mpf(D.MU), mpf(D.LAM)
    probe = R.Tet(D.UNIT, D.MU, D.LAM, D.RHO, D.DT)
    pd = D.pd_mask(name, mat) if name in D.PD_CANDIDATES else np.zeros(len(F), dtype=bool)
    out = {k: np.zeros(len(F)) for k in ("sigma", "psi", "P", "dPdF", "frame")}
    for e in range(len(F)):
        Fm = R.m3(F[e])
        _, s, _, _ = R.svd_rot(Fm)
        psi, P, _ = R.energy_density(mat, Fm, mu, lam)
        sig, kR, SP, SPsi = probe.scales(Fm, s)
        U, S, V = got["U"][e], got["S"][e], got["V"][e]
        s0 = max(sig[0], 1e-300)
        out["sigma"][e] = max(float(abs(mpf(float(S[i])) - s[i])) for i in range(3)) / (D.EPS * s0)
        out["frame"][e] = max(np.abs(U.T @ U - np.eye(3)).max(), np.abs(V.T @ V - np.eye(3)).max(), abs(np.linalg.det(U) - 1),
                              abs(np.linalg.det(V) - 1), np.abs(U @ np.diag(S) @ V.T - F[e]).max() / s0) / D.EPS
        out["psi"][e] = float(abs(mpf(float(got["psi"][e])) - psi)) / (D.EPS * SPsi)
        out["P"][e] = max(float(abs(mpf(float(got["P"][e][i][j])) - P[i][j])) for i in range(3) for j in range(3)) / (D.EPS * kR * SP)
        if pd[e]:
            Mref = R.dPdF_fd(mat, Fm, mu, lam)
            Mdev = D.spectral_dPdF(mat, U, S, V, blocks=(got["A"][e], got["B"][e]))
            out["dPdF"][e] = np.abs(Mdev - Mref).max() / (D.EPS * kR * np.abs(Mref).max())
        tol = D.K_P * D.EPS * s0           # descending up to rounding (equal sigma); the sign of S[2] is part of the sigma bound
        assert S[0] >= S[1] - tol and S[1] >= abs(S[2]) - tol, (name, e, S)
    return out


@pytest.mark.parametrize("mat,mname", MATS, ids=[m[1] for m in MATS])
@pytest.mark.parametrize("name", list(D.FAMILIES))
def test_host_twin_of_elem_math_meets_the_bounds(host_twin, name, mat, mname, capsys):
    err = host_twin_errors(host_twin, name, mat)
    with capsys.disabled():
        print(f"\n  host twin {mname} {name}: " + " ".join(f"{k} {v.max():.3g}" for k, v in err.items()), end="")
    assert np.isfinite(err["psi"]).all() and np.isfinite(err["sigma"]).all()
    # conventions (U, V in SO(3), F = U S V^T) and singular values accurate to K eps sigma_0 -- the rank <= 1 branch included
    assert err["frame"].max() <= D.K_P and err["sigma"].max() <= D.K_P
    assert err["psi"].max() <= D.K_PSI
    if name not in D.UNDEFINED_R:          # the polar factor is not defined on these two: energy and finiteness only
        assert err["P"].max() <= D.K_P
        assert err["dPdF"].max() <= D.K_H


def test_oracle_errors_per_family(capsys):
    """Printed, not asserted (DESIGN.md records them): the CPU oracle's own normalised gradient error per family against
    the 60-digit reference, so that a reader knows which side of a device-vs-oracle comparison is the accurate one."""
    from tests import oracle_py as O
    lines = []
    for mat, mname in MATS:
        for name in D.ASSERTED:
            V, T, x = D.mesh(name)
            orc = O.OracleSim(V, T, D.YM, D.PR, D.RHO, mat, D.DT, np.zeros(len(V), dtype=np.uint8), V.copy(),
                              (np.arange(len(T)) * 4 // len(T)).astype(np.int32), 4, False)
            g = orc.gradient(x)
            orc.close()
            assert np.isfinite(g).all()
            lines.append(f"  oracle {mname} {name}: g {D.normalised_errors(name, mat, None, g.reshape(-1, 12))['g'].max():.3g}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
