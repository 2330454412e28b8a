// time_integration.hpp -- the time integration rule of a step, stated once for the update / predictor kernels (k_timeint.hip), the host
// sequencing (dotmi_step, dotmi_reconfig.hip), dotmi_plan_time_integration and tit_check.cpp.  Extends the reference's one-entry switch
// on TimeIntegrationType (Optimizer.cpp:354-361 velocity update, :588-610 predictor, :1188 energy, :1225 gradient) by BDF2.
// Needs neither the HIP runtime nor the handle.
//
// A variable-step BDF2 step from (x_n, v_n) and (x_{n-1}, v_{n-1}), w = dt / dt_prev:
//     gamma = (1 + w) / (1 + 2 w),   c0 = (1 + w)^2 / (1 + 2 w),   c1 = w^2 / (1 + 2 w)        (c0 - c1 = 1; w = 1: 2/3, 4/3, 1/3)
//     x^ = c0 x_n - c1 x_{n-1},      v^ = c0 v_n - c1 v_{n-1},      dt_e = gamma dt
// is the backward-Euler step of size dt_e from (x^, v^): the predictor x~ = x^ + (dt_e v^ + dt_e^2 g) on free vertices, the minimisation
// of the same incremental potential with dt_e for dt, and v+ = (x+ - x^) / dt_e.  Energy, gradient, Hessian, factors and tolerance see
// dt_e only.  Without level n-1 (the first step of a run, or of a state that was set) the step is backward Euler at dt: (1, 0, 1).
//
// The per-component expressions have the operation shape of be_update_kernel, x_tilde_kernel and dotmi_set_state -- xn + (v * dt +
// gdtsq), no contraction (-ffp-contract=off everywhere they are compiled) -- so that a BDF2 step agrees to the bit with a
// backward-Euler handle at dt_e that was given (x^, v^).
#pragma once

#if defined(__HIPCC__)
#define TIT_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define TIT_HD inline
#endif

namespace dotmi {

constexpr int TIT_BE = 0;     // DOTMI_TIT_BE (TimeIntegrationType::TIT_BE, Types.hpp)
constexpr int TIT_BDF2 = 1;   // DOTMI_TIT_BDF2

struct TitPlan {
    double c0, c1;    // x^ = c0 x_n - c1 x_{n-1}, likewise v^
    double gamma;     // dt_e = gamma dt
    double dt_eff;
};

// kind: TIT_BE / TIT_BDF2; levels: 1 when (x_{n-1}, v_{n-1}) exist and dt_prev is the size of the step that led from them to level n
TIT_HD TitPlan tit_plan(int kind, double dt, double dt_prev, int levels)
{
    if (kind != TIT_BDF2 || levels < 1) return TitPlan{1.0, 0.0, 1.0, dt};
    const double w = dt / dt_prev;
    const double den = 1.0 + 2.0 * w;
    // c0 = 1 + w^2 / (1 + 2 w) ( = (1 + w)^2 / (1 + 2 w) ) and c1 = c0 - 1, which is exact for c0 >= 1: c0 - c1 == 1 in floating
    // point too, so a vertex at rest keeps x^ = x to rounding and a constant is a fixed point of the coefficients
    const double c0 = 1.0 + (w * w) / den;
    const double gamma = (1.0 + w) / den;
    return TitPlan{c0, c0 - 1.0, gamma, gamma * dt};
}

// x^ (and v^) of one component
TIT_HD double tit_hat(double c0, double c1, double an, double anm1) { return c0 * an - c1 * anm1; }

// x~ of one component: the predictor on a free vertex, the current position on a fixed one
TIT_HD double tit_x_tilde(bool fixed, double x, double xhat, double vhat, double dt_eff, double gdtsq)
{
    return fixed ? x : xhat + (vhat * dt_eff + gdtsq);
}

// v+ of one component
TIT_HD double tit_velocity(double x, double xhat, double dt_eff) { return (x - xhat) / dt_eff; }

}  // namespace dotmi
