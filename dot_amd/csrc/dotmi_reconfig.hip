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
//
// The time integration rule (dotmi_set_time_integration, dotmi_set_history; time_integration.hpp) is a fourth such value: under BDF2 the
// launches take the EFFECTIVE step dt_e = gamma dt of the next step, so whatever changes it between two steps -- the caller's dt, the
// integrator, the stored level n-1 (dotmi_set_state drops it, dotmi_set_history gives it) -- redoes what dotmi_set_time_step redoes: x^ and
// x~ from the stored levels and, where dt_e did change, the refresh (tit_replan).
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

// the effective step of the next step into what the launches take; true when it changed
bool tit_apply(dotmi_handle *h, const TitPlan &p)
{
    const bool changed = p.dt_eff != h->dt;
    h->dt = p.dt_eff;
    h->dtSq = h->dt * h->dt;
    for (int d = 0; d < 3; ++d) h->gdtsq[d] = h->dtSq * h->grav[d];
    h->targetGRes = host_target_gres(h);
    return changed;
}

// between two steps: the next step's rule from (tit, dtUser, dtPrev, levels), x~ (BDF2: and x^) from the stored levels, and the refresh
// where the effective step changed (always: whenever the caller's entry refreshes anyway)
int tit_replan(dotmi_handle *h, bool always)
{
    const TitPlan p = tit_plan(h->tit, h->dtUser, h->dtPrev, h->levels);
    const bool changed = tit_apply(h, p);
    if (h->tit == TIT_BDF2)
        launch_bdf2_predict(h->nV, h->M.fixed, h->xn, h->v, h->xnm1, h->vnm1, h->xhat, h->xt, p, h->gdtsq, h->st);
    else
        launch_x_tilde(h->nV, h->M.fixed, h->xn, h->v, h->dt, h->gdtsq, h->xt, h->st);
    return (changed || always) ? refresh_factors(h) : 0;
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
    h->dtUser = dt;
    // BDF2: the variable-step rule, w = dt / dt_prev -- not a restart (Optimizer::setTime leaves the velocity alone, too)
    if (h->tit == TIT_BDF2) return tit_replan(h, true);
    h->dt = dt;
    h->dtSq = dt * dt;
    for (int d = 0; d < 3; ++d) h->gdtsq[d] = h->dtSq * h->grav[d];
    h->targetGRes = host_target_gres(h);
    launch_x_tilde(h->nV, h->M.fixed, h->xn, h->v, h->dt, h->gdtsq, h->xt, h->st);
    return refresh_factors(h);
}

// The reference switches on Config::timeIntegrationType at the velocity update (Optimizer.cpp:354-361), the predictor (:588-610), the
// energy (:1188) and the gradient (:1225); its enum has the one entry TIT_BE.  Here the switch is at the first two only: BDF2's energy and
// gradient are backward Euler's at the effective step.
int dotmi_set_time_integration(dotmi_handle *h, int32_t kind)
{
    if (!h) return DOTMI_E_INVALID;
    if (kind != DOTMI_TIT_BE && kind != DOTMI_TIT_BDF2) {
        h->err = "dotmi_set_time_integration: unknown time integration id " + std::to_string(kind);
        return DOTMI_E_INVALID;
    }
    if (int rc = enter(h)) return rc;
    if (kind == h->tit) return 0;
    if (kind == DOTMI_TIT_BDF2 && !h->xnm1) {
        // zeroed: the start step forms x^ = 1 x_n - 0 x_{n-1}
        for (double **vec : {&h->xnm1, &h->vnm1, &h->xhat}) {
            if (int rc = dalloc(h, vec, (size_t)h->n)) return rc;
            HIPCHECK(h, hipMemsetAsync(*vec, 0, sizeof(double) * h->n, h->st));
        }
    }
    h->tit = kind;
    h->levels = 0;   // a backward-Euler handle keeps no level n-1: the first BDF2 step is a start step
    h->dtPrev = 0.0;
    return tit_replan(h, false);
}

int32_t dotmi_time_integration(const dotmi_handle *h) { return h ? h->tit : DOTMI_E_INVALID; }

int dotmi_time_integration_info(const dotmi_handle *h, int32_t *kind, int32_t *levels, double *dt_eff, double *dt_prev)
{
    if (!h) return DOTMI_E_INVALID;
    if (kind) *kind = h->tit;
    if (levels) *levels = h->levels;
    if (dt_eff) *dt_eff = h->dt;
    if (dt_prev) *dt_prev = h->levels ? h->dtPrev : 0.0;
    return 0;
}

int dotmi_get_history(dotmi_handle *h, double *x_prev, double *v_prev, double *dt_prev)
{
    if (!h) return DOTMI_E_INVALID;
    if (int rc = enter(h); rc == DOTMI_E_DEVICE) return rc;
    if (dt_prev) *dt_prev = h->levels ? h->dtPrev : 0.0;
    if (!h->levels) return 0;
    const size_t bytes = sizeof(double) * h->n;
    HIPCHECK(h, hipStreamSynchronize(h->st));
    if (x_prev) HIPCHECK(h, hipMemcpy(x_prev, h->xnm1, bytes, hipMemcpyDeviceToHost));
    if (v_prev) HIPCHECK(h, hipMemcpy(v_prev, h->vnm1, bytes, hipMemcpyDeviceToHost));
    return 1;
}

int dotmi_set_history(dotmi_handle *h, const double *x_prev, const double *v_prev, double dt_prev)
{
    if (!h) return DOTMI_E_INVALID;
    if (!x_prev || !v_prev) {
        h->err = "dotmi_set_history: x_prev and v_prev must be given";
        return DOTMI_E_INVALID;
    }
    if (!(dt_prev > 0) || !std::isfinite(dt_prev)) {
        h->err = "dotmi_set_history: dt_prev must be positive and finite";
        return DOTMI_E_INVALID;
    }
    if (h->tit != TIT_BDF2) {
        h->err = "dotmi_set_history: backward Euler keeps no level n-1 (dotmi_set_time_integration(h, DOTMI_TIT_BDF2) first)";
        return DOTMI_E_INVALID;
    }
    if (int rc = enter(h)) return rc;
    const size_t bytes = sizeof(double) * h->n;
    HIPCHECK(h, hipMemcpyAsync(h->xnm1, x_prev, bytes, hipMemcpyHostToDevice, h->st));
    HIPCHECK(h, hipMemcpyAsync(h->vnm1, v_prev, bytes, hipMemcpyHostToDevice, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));   // (the caller's arrays are free again)
    h->levels = 1;
    h->dtPrev = dt_prev;
    return tit_replan(h, false);
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
