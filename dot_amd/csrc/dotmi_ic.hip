// dotmi_ic.hip -- LBFGS-HI (DOTMI_FLAG_LBFGS_HI; `timeStepper LBFGSHI`, LBFGSTimeStepper with D0T_HI, LBFGSTimeStepper.cpp:214-233,
// :308-316, :376-378): L-BFGS whose initial inverse Hessian is an INCOMPLETE Cholesky factor of the projected Hessian, rebuilt at the
// end of every step.  This is a GPU form of the method, not of Eigen::IncompleteCholesky: a block (3 x 3) IC(0) on H's own block
// pattern in the multicolour ordering of ic_plan.hpp (Eigen: scalar, AMD ordering, diagonal scaling, sequential substitutions), one
// launch per colour (k_ic.hip), with a diagonal-shift restart on breakdown.  Create, step and refix follow LBFGS-PD's conventions
// (dotmi_pd.hip): no subdomain block solve, host-driven loop, unit first step, single GPU.
#include "dotmi_handle.hpp"
#include "ic_plan.hpp"

namespace dotmi {

constexpr int IC_MAX_ATTEMPTS = 40;
constexpr double IC_FIRST_SHIFT = 1e-3;

// the plan and the factor storage (once per create)
int build_ic(dotmi_handle *h, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx)
{
    IcPlan P;
    ic_plan(h->nV, adj_ptr, adj_idx, P);
    DevIC &D = h->IC;
    D.nV = h->nV;
    D.nL = (int)P.lidx.size();
    h->icStart = P.cstart;
    if (int rc = upload(h, &D.vert, P.vert)) return rc;
    if (int rc = upload(h, &D.lptr, P.lptr)) return rc;
    if (int rc = upload(h, &D.lidx, P.lidx)) return rc;
    if (int rc = upload(h, &D.lsrc, P.lsrc)) return rc;
    if (int rc = upload(h, &D.dsrc, P.dsrc)) return rc;
    if (int rc = upload(h, &D.pptr, P.pptr)) return rc;
    if (int rc = upload(h, &D.pa, P.pa)) return rc;
    if (int rc = upload(h, &D.pb, P.pb)) return rc;
    if (int rc = upload(h, &D.uptr, P.uptr)) return rc;
    if (int rc = upload(h, &D.ublk, P.ublk)) return rc;
    if (int rc = upload(h, &D.uvert, P.uvert)) return rc;
    const size_t nF = 9 * ((size_t)D.nL + D.nV);
    if (int rc = dalloc(h, &D.F, nF)) return rc;
    if (int rc = dalloc(h, &D.yw, (size_t)3 * D.nV)) return rc;
    if (int rc = dalloc(h, &D.flag, 1)) return rc;
    HIPCHECK(h, hipHostMalloc((void **)&h->h_info, sizeof(int)));
    h->h_info[0] = 0;
    h->wTotal = nF;
    // one application streams every stored block twice: forward and backward sweep
    h->precond_bytes = 72 * ((int64_t)D.nL + D.nV) * 2;
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: LBFGS-HI: %d colours, %d lower blocks, %zu products, %.1f MB of factor storage\n", P.nColours, D.nL,
                P.pa.size(), 8e-6 * nF);
    return 0;
}

// The refresh of an LBFGS-HI handle: H(x) by the element-Hessian and assembly kernels of every refresh, then the incomplete
// factor -- no dense fill, no tile factorisation.  Shift policy, once per factorisation: the first attempt takes sigma = 0 if the
// last successful shift was 0, else half of it; a breakdown doubles it (from 1e-3), refills and refactors, one flag read-back
// per attempt.
int ic_refresh(dotmi_handle *h, const double *x, double *ms_hess, double *ms_fact)
{
    const DevIC &D = h->IC;
    HIPCHECK(h, hipEventRecord(h->ev0, h->st));
    launch_elem_hessians(h->M, h->mat, h->dtSq, x, h->He, h->st);
    launch_assemble(h->M, h->He, h->Hval, h->st);
    HIPCHECK(h, hipEventRecord(h->ev1, h->st));
    double sigma = h->icShift == 0.0 ? 0.0 : 0.5 * h->icShift;
    const int nc = (int)h->icStart.size() - 1;
    int attempts = 0;
    bool ok = false;
    while (!ok && attempts < IC_MAX_ATTEMPTS) {
        ++attempts;
        launch_ic_fill(D, h->Hval, sigma, h->st);
        HIPCHECK(h, hipMemsetAsync(D.flag, 0, sizeof(int), h->st));
        for (int c = 0; c < nc; ++c) launch_ic_factor_colour(D, h->icStart[c], h->icStart[c + 1], h->st);
        HIPCHECK(h, hipMemcpyAsync(h->h_info, D.flag, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHECK(h, hipStreamSynchronize(h->st));
        HIPCHECK(h, hipGetLastError());
        ok = h->h_info[0] == 0;
        if (!ok && attempts < IC_MAX_ATTEMPTS) sigma = std::max(IC_FIRST_SHIFT, 2.0 * sigma);
    }
    HIPCHECK(h, hipEventRecord(h->ev2, h->st));
    HIPCHECK(h, hipEventSynchronize(h->ev2));
    h->icAttempts = attempts;
    float a = 0, b = 0;
    hipEventElapsedTime(&a, h->ev0, h->ev1);
    hipEventElapsedTime(&b, h->ev1, h->ev2);
    if (ms_hess) *ms_hess += a;
    if (ms_fact) *ms_fact += b;
    h->phaseMs[DOTMI_T_MATRIX_COMPUTATION] += a;
    h->phaseMs[DOTMI_T_NUMERICAL_FACTORIZATION] += b;
    if (!ok) {
        h->err = "LBFGS-HI: the incomplete Cholesky factorisation broke down with every shift up to " + std::to_string(sigma) + " (" +
                 std::to_string(attempts) + " attempts)";
        h->poisoned = true;
        return DOTMI_E_NOTSPD;
    }
    h->icShift = sigma;
    h->poisoned = false;
    return 0;
}

// z = (L L^T)^-1 q: forward sweep through the colours, backward sweep back (2 x colours launches on the handle's stream, a linear
// chain); leaves the y_i . z partials of the stored pairs in partC
int ic_apply(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L)
{
    const Bracket br = backsolve_bracket(h);
    if (br.ev0) HIPCHECK(h, hipEventRecord(br.ev0, h->st));
    const int nc = (int)h->icStart.size() - 1;
    for (int c = 0; c < nc; ++c) launch_ic_forward_colour(h->IC, h->icStart[c], h->icStart[c + 1], q, h->st);
    for (int c = nc - 1; c >= 0; --c) launch_ic_backward_colour(h->IC, h->icStart[c], h->icStart[c + 1], z, h->st);
    if (br.ev1) HIPCHECK(h, hipEventRecord(br.ev1, h->st));
    launch_multidot(h->n, z, L.y, L.m, h->partC, h->st);
    return 0;
}

}  // namespace dotmi

extern "C" {

int dotmi_ic_info(dotmi_handle *h, int32_t *colours, double *shift, int32_t *attempts)
{
    if (!h) return DOTMI_E_INVALID;
    if (!h->hi) {
        h->err = "dotmi_ic_info: not an LBFGS-HI handle";
        return DOTMI_E_INVALID;
    }
    if (colours) *colours = (int32_t)h->icStart.size() - 1;
    if (shift) *shift = h->icShift;
    if (attempts) *attempts = h->icAttempts;
    return 0;
}

int dotmi_ic_factor(dotmi_handle *h, int32_t cap, double *blocks)
{
    if (!h) return DOTMI_E_INVALID;
    if (!h->hi) {
        h->err = "dotmi_ic_factor: not an LBFGS-HI handle";
        return DOTMI_E_INVALID;
    }
    const int nb = h->IC.nL + h->IC.nV;
    if (!blocks) return nb;
    if (cap < nb) {
        h->err = "dotmi_ic_factor: room for " + std::to_string(nb) + " blocks is needed";
        return DOTMI_E_INVALID;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = enter_with_factors(h)) return rc;
    HIPCHECK(h, hipMemcpyAsync(blocks, h->IC.F, sizeof(double) * 9 * (size_t)nb, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    return nb;
}

}  // extern "C"
