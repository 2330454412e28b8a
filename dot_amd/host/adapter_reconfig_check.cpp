// Compile/link check of the C++ adapter's setters on a built stepper (tests/test_reconfigure_host.py builds it with g++, no HIP
// headers, and runs it): setRelGL2Tol and setTime forward to dotmi_set_rel_tol / dotmi_set_time_step once the handle exists,
// setLameParam to dotmi_set_lame.  Without a GPU precompute() must throw the ABI's "no CPU fallback" error (exit 3); with one the
// tiny mesh of adapter_check.cpp steps through all three.
#include <cstdio>
#include <cstring>
#include "DotHipTimeStepper.hpp"

int main()
{
    const double V[] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1};
    const int32_t F[] = {0, 1, 2, 3, 1, 2, 3, 4};
    const double u[] = {35714.2857, 35714.2857}, lam[] = {142857.1428, 142857.1428};
    const uint8_t fixed[] = {1, 0, 0, 0, 0};
    const int32_t epart[] = {0, 1};
    dot_amd::MeshView m;
    m.nV = 5; m.nT = 2; m.V_rest = V; m.F = F; m.u = u; m.lambda = lam; m.density = 1000.0; m.isFixedVert = fixed;
    dot_amd::Options o;
    o.energyType = DOTMI_ENERGY_SNH; o.partitionAmt = 2; o.epart = epart;
    dot_amd::DotHipTimeStepper ts(m, o, V);
    ts.setTime(1.0, 0.025);
    ts.setRelGL2Tol();
    try {
        ts.setLameParam(u, lam);   // the handle does not exist yet
        return 4;
    } catch (const std::logic_error &) {
    }
    try {
        ts.precompute();
    } catch (const std::exception &e) {
        std::printf("precompute failed: %s\n", e.what());
        return std::strstr(e.what(), "no CPU fallback") ? 3 : 1;
    }
    int rc = ts.solve(1);
    const double tol0 = ts.getTargetGRes();
    ts.setRelGL2Tol(1.0e-3);   // targetGRes goes with relTol^2
    const double tol1 = ts.getTargetGRes();
    if (!(tol1 > 9.9e3 * tol0 && tol1 < 1.01e4 * tol0)) return 5;
    rc |= ts.solve(1);
    ts.setTime(1.0, 0.0125);   // ... and with dt^4
    const double tol2 = ts.getTargetGRes();
    if (!(tol2 > tol1 / 16.01 && tol2 < tol1 / 15.99)) return 6;
    rc |= ts.solve(1);
    const double u2[] = {2 * u[0], u[1]}, lam2[] = {2 * lam[0], lam[1]};
    ts.setLameParam(u2, lam2);
    if (!(ts.getTargetGRes() > tol2)) return 7;
    rc |= ts.solve(1);
    try {
        ts.setRelGL2Tol(0.0);
        return 8;
    } catch (const std::runtime_error &) {
    }
    std::printf("solve -> %d, iter %d, inner %d, tol %.6e\n", rc, ts.getIterNum(), ts.getInnerIterAmt(), ts.getTargetGRes());
    return (rc == 0 && ts.getIterNum() == 4) ? 0 : 2;
}
