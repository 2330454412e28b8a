// tit_check.cpp -- the time integration rule (time_integration.hpp) on the CPU under the address / UB sanitizers (make tit_check; links
// nothing of HIP).  Four checks:
//   1. backward Euler, and BDF2 without level n-1, plan (c0, c1, gamma) = (1, 0, 1) and dt_e = dt, and their x^, x~, v+ are the
//      expressions of be_update_kernel / x_tilde_kernel bit for bit;
//   2. for w = dt / dt_prev in {1, 0.5, 3}: c0 - c1 == 1 exactly, gamma, c0, c1 within a few roundings of their closed forms, and at
//      w = 1 the textbook 2/3, 4/3, 1/3;
//   3. the header's per-component functions, applied vertex by vertex as the kernels of k_timeint.hip apply them, against a plain indexed
//      statement of the update and the predictor over whole arrays, bit for bit, on random states with fixed vertices;
//   4. exactness: on x(t) = a + b t + c t^2 per component, with levels taken from the polynomial, the velocity formula returns x'(t_{n+1})
//      and agrees with the classical variable-step difference formula, and the predictor with the constant acceleration 2c for gravity
//      reproduces x(t_{n+1}) -- the rule integrates quadratics exactly (to rounding), whatever the step ratio.
#include "time_integration.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace dotmi;

namespace {

int g_fail = 0;
void expect(bool ok, const char *what, double a = 0, double b = 0)
{
    if (ok) return;
    fprintf(stderr, "tit_check: %s (%.17g vs %.17g)\n", what, a, b);
    ++g_fail;
}
bool same_bits(double a, double b) { return !memcmp(&a, &b, sizeof(double)); }
bool close_rel(double a, double b, double rel) { return std::abs(a - b) <= rel * std::max(std::abs(a), std::abs(b)); }

struct State {
    std::vector<double> x, xn, v, xnm1, vnm1, xhat, xt;
    explicit State(int n) : x(n), xn(n), v(n), xnm1(n), vnm1(n), xhat(n), xt(n) {}
};

// ---- the plain statement: variable-step BDF2 over whole arrays, written out from the formulas ----
void plain_update(int nV, const std::vector<unsigned char> &fixed, State &s, double dt_done, double dt, double dt_prev,
                  const double *grav)
{
    const double w = dt / dt_prev;
    const double c0 = 1.0 + w * w / (1.0 + 2.0 * w), c1 = c0 - 1.0, dte = (1.0 + w) / (1.0 + 2.0 * w) * dt;
    for (int i = 0; i < nV; ++i)
        for (int d = 0; d < 3; ++d) {
            const int k = 3 * i + d;
            const double vel = (s.x[k] - s.xhat[k]) / dt_done;
            s.xnm1[k] = s.xn[k];
            s.vnm1[k] = s.v[k];
            s.xn[k] = s.x[k];
            s.v[k] = vel;
            s.xhat[k] = c0 * s.xn[k] - c1 * s.xnm1[k];
            const double vh = c0 * s.v[k] - c1 * s.vnm1[k];
            s.xt[k] = fixed[i] ? s.x[k] : s.xhat[k] + (vh * dte + dte * dte * grav[d]);
        }
}

// ---- the header's functions, vertex by vertex, in the order of bdf2_update_kernel ----
void header_update(int nV, const std::vector<unsigned char> &fixed, State &s, double dt_done, const TitPlan &next, const double *gdtsq)
{
    for (int i = 0; i < nV; ++i)
        for (int d = 0; d < 3; ++d) {
            const int k = 3 * i + d;
            const double xv = s.x[k], xo = s.xn[k], vo = s.v[k];
            const double vel = tit_velocity(xv, s.xhat[k], dt_done);
            s.xnm1[k] = xo;
            s.vnm1[k] = vo;
            s.xn[k] = xv;
            s.v[k] = vel;
            const double xh = tit_hat(next.c0, next.c1, xv, xo), vh = tit_hat(next.c0, next.c1, vel, vo);
            s.xhat[k] = xh;
            s.xt[k] = tit_x_tilde(fixed[i] != 0, xv, xh, vh, next.dt_eff, gdtsq[d]);
        }
}

bool same_state(const State &a, const State &b)
{
    auto eq = [](const std::vector<double> &u, const std::vector<double> &w) { return !memcmp(u.data(), w.data(), sizeof(double) * u.size()); };
    return eq(a.xn, b.xn) && eq(a.v, b.v) && eq(a.xnm1, b.xnm1) && eq(a.vnm1, b.vnm1) && eq(a.xhat, b.xhat) && eq(a.xt, b.xt);
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240911);
    std::uniform_real_distribution<double> val(-1.0, 1.0);
    const double ratios[3] = {1.0, 0.5, 3.0};

    // ---- 1. backward Euler is (1, 0, 1) and its expressions are the backward-Euler kernels' ----
    for (int kind : {TIT_BE, TIT_BDF2})
        for (int levels : {0, 1}) {
            if (kind == TIT_BDF2 && levels == 1) continue;
            const double dt = 0.01 * (1.0 + std::abs(val(rng)));
            const TitPlan p = tit_plan(kind, dt, 0.37 * dt, levels);
            expect(p.c0 == 1.0 && p.c1 == 0.0 && p.gamma == 1.0 && same_bits(p.dt_eff, dt), "backward Euler is not (1, 0, 1) at dt", p.c0, p.c1);
            for (int t = 0; t < 1000; ++t) {
                const double xn = 10 * val(rng), xo = 10 * val(rng), v = val(rng), vo = val(rng), x = xn + 0.01 * val(rng), g = -9.8 * dt * dt;
                const double xh = tit_hat(p.c0, p.c1, xn, xo), vh = tit_hat(p.c0, p.c1, v, vo);
                expect(xh == xn && vh == v, "x^ != x_n under backward Euler", xh, xn);
                expect(same_bits(tit_x_tilde(false, xn, xh, vh, p.dt_eff, g), xn + (v * dt + g)), "x~ is not x_tilde_kernel's");
                expect(same_bits(tit_x_tilde(true, xn, xh, vh, p.dt_eff, g), xn), "x~ of a fixed vertex is not its position");
                expect(same_bits(tit_velocity(x, xh, p.dt_eff), (x - xn) / dt), "v+ is not be_update_kernel's");
            }
        }

    // ---- 2. the coefficients ----
    for (double w : ratios)
        for (int t = 0; t < 200; ++t) {
            const double dtp = 0.001 + 0.05 * std::abs(val(rng)), dt = w * dtp;
            const TitPlan p = tit_plan(TIT_BDF2, dt, dtp, 1);
            const double wr = dt / dtp;   // (w itself up to one rounding)
            expect(p.c0 - p.c1 == 1.0, "c0 - c1 != 1", p.c0, p.c1);
            expect(close_rel(p.gamma, (1 + wr) / (1 + 2 * wr), 4e-16), "gamma", p.gamma, (1 + wr) / (1 + 2 * wr));
            // (c0 in [1, 4) carries one rounding of its own and one of the quotient; c1 = c0 - 1 inherits them as an absolute error)
            expect(std::abs(p.c0 - (1 + wr) * (1 + wr) / (1 + 2 * wr)) <= 9e-16, "c0", p.c0, (1 + wr) * (1 + wr) / (1 + 2 * wr));
            expect(std::abs(p.c1 - wr * wr / (1 + 2 * wr)) <= 9e-16, "c1", p.c1, wr * wr / (1 + 2 * wr));
            expect(same_bits(p.dt_eff, p.gamma * dt), "dt_e != gamma dt", p.dt_eff, p.gamma * dt);
        }
    {
        const TitPlan p = tit_plan(TIT_BDF2, 0.01, 0.01, 1);
        expect(close_rel(p.gamma, 2.0 / 3.0, 2.3e-16) && close_rel(p.c0, 4.0 / 3.0, 2.3e-16) && std::abs(p.c1 - 1.0 / 3.0) <= 2.3e-16,
               "w = 1 is not (2/3, 4/3, 1/3)", p.gamma, p.c0);
    }

    // ---- 3. the header against the plain statement over arrays, several steps with changing step sizes ----
    long long compared = 0;
    for (int seq = 0; seq < 50; ++seq) {
        const int nV = 1 + (int)(rng() % 97), n = 3 * nV;
        std::vector<unsigned char> fixed(nV);
        for (auto &f : fixed) f = rng() % 4 == 0;
        State a(n), b(n);
        for (int k = 0; k < n; ++k) {
            a.xn[k] = 10 * val(rng);
            a.v[k] = val(rng);
            a.xnm1[k] = a.xn[k] - 0.01 * val(rng);
            a.vnm1[k] = val(rng);
            a.xhat[k] = a.xn[k] + 0.01 * val(rng);
        }
        b = a;
        const double grav[3] = {0.0, -9.80665, 0.3};
        double dt_done = 0.004 + 0.004 * std::abs(val(rng)), dt_prev_user = dt_done;
        for (int step = 0; step < 12; ++step) {
            for (int k = 0; k < n; ++k) a.x[k] = b.x[k] = a.xn[k] + 0.01 * val(rng);
            const double dt = dt_prev_user * ratios[rng() % 3];
            const TitPlan next = tit_plan(TIT_BDF2, dt, dt_prev_user, 1);
            const double gdtsq[3] = {next.dt_eff * next.dt_eff * grav[0], next.dt_eff * next.dt_eff * grav[1],
                                     next.dt_eff * next.dt_eff * grav[2]};
            plain_update(nV, fixed, a, dt_done, dt, dt_prev_user, grav);
            header_update(nV, fixed, b, dt_done, next, gdtsq);
            ++compared;
            if (!same_state(a, b)) {
                expect(false, "the header's update differs from the plain statement", seq, step);
                return 1;
            }
            dt_done = next.dt_eff;
            dt_prev_user = dt;
        }
    }

    // ---- 4. exactness on quadratics in t ----
    for (double w : ratios)
        for (int t = 0; t < 500; ++t) {
            const double a = val(rng), b = val(rng), c = val(rng);
            const double dtp = 0.01 + 0.05 * std::abs(val(rng)), dt = w * dtp, tn = val(rng), tp = tn - dtp, t1 = tn + dt;
            auto X = [&](double s) { return a + b * s + c * s * s; };
            auto V = [&](double s) { return b + 2 * c * s; };
            const TitPlan p = tit_plan(TIT_BDF2, dt, dtp, 1);
            const double xh = tit_hat(p.c0, p.c1, X(tn), X(tp)), vh = tit_hat(p.c0, p.c1, V(tn), V(tp));
            // v+ of the exact position is the exact velocity, and the classical variable-step formula
            const double vel = tit_velocity(X(t1), xh, p.dt_eff);
            expect(std::abs(vel - V(t1)) <= 1e-11, "v+ is not exact on a quadratic", vel, V(t1));
            const double wr = dt / dtp;
            const double classic = ((1 + 2 * wr) / (1 + wr) * X(t1) - (1 + wr) * X(tn) + wr * wr / (1 + wr) * X(tp)) / dt;
            expect(std::abs(vel - classic) <= 1e-11, "v+ is not the variable-step BDF2 difference", vel, classic);
            // the step itself, M a = f with the constant acceleration 2c:  x+ = x^ + dt_e v^ + dt_e^2 (2c) = x~ with gdtsq = dt_e^2 2c
            const double xt = tit_x_tilde(false, X(tn), xh, vh, p.dt_eff, p.dt_eff * p.dt_eff * 2 * c);
            expect(std::abs(xt - X(t1)) <= 1e-13, "the step is not exact on a quadratic", xt, X(t1));
        }

    if (g_fail) {
        fprintf(stderr, "tit_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("tit_check: backward Euler is (1, 0, 1); c0 - c1 == 1; %lld updates equal to the plain statement; quadratics exact at w = 1, 0.5, 3\n",
           compared);
    return 0;
}
