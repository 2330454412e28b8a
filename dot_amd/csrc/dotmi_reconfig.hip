// dotmi_reconfig.hip -- tolerance, time step and materials changed on a live handle (dotmi_set_rel_tol, dotmi_set_time_step,
// dotmi_set_lame): each does only what the new value invalidates.  The rule behind every detail: afterwards the handle is the one
// dotmi_create would have built from the new value, brought to this state with dotmi_set_state and dotmi_refactor(h, NULL).
//
// Where the three values live, and who re-reads them:
//   relTol      only in targetGRes; the loop drivers read h->targetGRes per step (run_device_loop copies it into DevLoop)
//   dt          dt, dtSq, gdtsq are launch arguments everywhere (element passes, refresh, pd_factor, initX, BE update, DevLoop::dtSq per
//               step) -- what was BUILT with them is x~, the Hessian with its subdomain factors, and LBFGS-PD's L with its factor
//   mu, lambda  host copies (tolerance), the global per-element arrays M.mu / M.lam (refresh, PD Laplacian; Mown shares the pointers),
//               and per patch family either two kernel arguments (one material) or per-slot arrays
// The captured factorisation graph (run_factor) holds tile tasks on fixed buffers and none of these values: it is replayed as it is.
// The forecasts a step leaves for the next one (pairing, held back-solves, vertex patches) choose among forms with identical
// iterates; they stay, as they do across dotmi_set_state.
#include "dotmi_handle.hpp"

namespace dotmi {

// every entry: the refresh a step left running is judged first; its verdict, if any, is the call's and nothing is changed
static int enter(dotmi_handle *h)
{
    HIPCHECK(h, hipSetDevice(h->device));
    return resolve_refresh(h);
}

// the refresh of everything built with dt or the materials, at the current positions (the path of dotmi_refix)
static int refresh_factors(dotmi_handle *h)
{
    if (h->pd) return pd_factor(h);
    return refactor(h, h->x, nullptr, nullptr);
}

// one family: the kernel-argument form for one material, else the slot arrays (allocated on first need) filled on the device
static int set_family(dotmi_handle *h, dotmi_handle::SlotMap &SM, bool uniform, double **mu_s, double **lam_s)
{
    *mu_s = *lam_s = nullptr;
    if (uniform || !SM.elem) return 0;
    if (!SM.mu) {
        if (int rc = dalloc(h, &SM.mu, SM.nSlots)) return rc;
        if (int rc = dalloc(h, &SM.lam, SM.nSlots)) return rc;
    }
    launch_gather_lame(SM.elem, SM.nSlots, h->M.mu, h->M.lam, SM.mu, SM.lam, h->st);
    *mu_s = SM.mu;
    *lam_s = SM.lam;
    return 0;
}

template <class Patches>
static void point_family(Patches &D, double *mu_s, double *lam_s, double mu0, double lam0)
{
    D.mu = mu_s;
    D.lam = lam_s;
    D.mu0 = mu_s ? 0.0 : mu0;   // (as create leaves them)
    D.lam0 = mu_s ? 0.0 : lam0;
}

}  // namespace dotmi

extern "C" {

int dotmi_set_rel_tol(dotmi_handle *h, double relTol)
{
    if (!h) return DOTMI_E_INVALID;
    if (!(relTol > 0) || !std::isfinite(relTol)) {
        h->err = "dotmi_set_rel_tol: relTol must be positive and finite";
        return DOTMI_E_INVALID;
    }
    if (int rc = enter(h)) return rc;
    h->relTol = relTol;
    h->targetGRes = host_target_gres(h);
    return 0;
}

int dotmi_set_time_step(dotmi_handle *h, double dt)
{
    if (!h) return DOTMI_E_INVALID;
    if (!(dt > 0) || !std::isfinite(dt)) {
        h->err = "dotmi_set_time_step: dt must be positive and finite";
        return DOTMI_E_INVALID;
    }
    if (int rc = enter(h)) return rc;
    h->dt = dt;
    h->dtSq = dt * dt;
    for (int d = 0; d < 3; ++d) h->gdtsq[d] = h->dtSq * h->grav[d];
    h->targetGRes = host_target_gres(h);
    launch_x_tilde(h->nV, h->M.fixed, h->xn, h->v, h->dt, h->gdtsq, h->xt, h->st);
    return refresh_factors(h);
}

int dotmi_set_lame(dotmi_handle *h, const double *mu, const double *lambda)
{
    if (!h) return DOTMI_E_INVALID;
    if (!mu || !lambda) {
        h->err = "dotmi_set_lame: mu and lambda must be given";
        return DOTMI_E_INVALID;
    }
    bool uniform = true;
    for (int e = 0; e < h->nT; ++e) {
        if (!(mu[e] > 0) || !(lambda[e] > 0) || !std::isfinite(mu[e]) || !std::isfinite(lambda[e])) {
            h->err = "dotmi_set_lame: mu and lambda must be positive and finite (element " + std::to_string(e) + ")";
            return DOTMI_E_INVALID;
        }
        uniform = uniform && mu[e] == mu[0] && lambda[e] == lambda[0];
    }
    if (int rc = enter(h)) return rc;
    h->mu.assign(mu, mu + h->nT);
    h->lam.assign(lambda, lambda + h->nT);
    h->targetGRes = host_target_gres(h);
    const size_t bytes = sizeof(double) * (size_t)h->nT;
    HIPCHECK(h, hipMemcpyAsync(h->M.mu, h->mu.data(), bytes, hipMemcpyHostToDevice, h->st));
    HIPCHECK(h, hipMemcpyAsync(h->M.lam, h->lam.data(), bytes, hipMemcpyHostToDevice, h->st));
    // the families of create (build_element_side, choose_loop_form): all elements; this rank's own where the element pass is
    // sharded; the 512-element set of a speculating step where it is a set of its own; the vertex patches
    const double mu0 = mu[0], lam0 = lambda[0];
    double *ms = nullptr, *ls = nullptr;
    if (int rc = set_family(h, h->smAll, uniform, &ms, &ls)) return rc;
    point_family(h->PTall, ms, ls, mu0, lam0);
    if (h->smOwn.elem) {
        if (int rc = set_family(h, h->smOwn, uniform, &ms, &ls)) return rc;
    }
    point_family(h->PT, ms, ls, mu0, lam0);   // (not sharded: PT is PTall's tables)
    if (h->smSpec.elem) {
        if (int rc = set_family(h, h->smSpec, uniform, &ms, &ls)) return rc;
        point_family(h->PTspec, ms, ls, mu0, lam0);
    } else if (h->specFits) {
        point_family(h->PTspec, ms, ls, mu0, lam0);   // (PTspec is PT's tables)
    }
    if (h->smVP.elem) {
        if (int rc = set_family(h, h->smVP, uniform, &ms, &ls)) return rc;
        point_family(h->VP, ms, ls, mu0, lam0);
    }
    return refresh_factors(h);
}

}  // extern "C"
