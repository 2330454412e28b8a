// k_timeint.hip -- the BDF2 side of the time integration switch (time_integration.hpp; the reference's switch has one entry, TIT_BE:
// Optimizer.cpp:354-361 the update, :588-610 the predictor): the end-of-step update with the shift of the two levels, the predictor from
// the stored levels, and the start iterate.  One thread per vertex, three components, every value written once by its own thread.  The
// backward-Euler kernels (init_x_kernel, be_update_kernel, x_tilde_kernel) are not touched and a backward-Euler handle launches none of these.
#include <hip/hip_runtime.h>

#include "dotmi_internal.hpp"
#include "time_integration.hpp"

namespace dotmi {

struct Vec3Arg {
    double v[3];
};

// v+ = (x - x^) / dt_e of the step that ends; x_{n-1} <- x_n, v_{n-1} <- v_n, x_n <- x, v_n <- v+; then the next step's x^, x~ with its
// own coefficients and effective step (v^ lives only here: nothing reads it after x~)
__global__ void __launch_bounds__(256) bdf2_update_kernel(int nV, const uint8_t *__restrict__ fixed, const double *__restrict__ x,
                                                          double *__restrict__ xhat, double *__restrict__ xn, double *__restrict__ v,
                                                          double *__restrict__ xnm1, double *__restrict__ vnm1, double *__restrict__ xt,
                                                          double dt_eff_done, TitPlan next, Vec3Arg gdtsq_next)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nV) return;
    const bool fx = fixed[i] != 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int k = 3 * i + d;
        const double xv = x[k], xo = xn[k], vo = v[k];
        const double vel = tit_velocity(xv, xhat[k], dt_eff_done);
        xnm1[k] = xo;
        vnm1[k] = vo;
        xn[k] = xv;
        v[k] = vel;
        const double xh = tit_hat(next.c0, next.c1, xv, xo);
        const double vh = tit_hat(next.c0, next.c1, vel, vo);
        xhat[k] = xh;
        xt[k] = tit_x_tilde(fx, xv, xh, vh, next.dt_eff, gdtsq_next.v[d]);
    }
}

void launch_bdf2_update(int nV, const uint8_t *fixed, const double *x, double *xhat, double *xn, double *v, double *xnm1, double *vnm1,
                        double *xt, double dt_eff_done, const TitPlan &next, const double *gdtsq_next, hipStream_t st)
{
    Vec3Arg g = {{gdtsq_next[0], gdtsq_next[1], gdtsq_next[2]}};
    hipLaunchKernelGGL(bdf2_update_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, fixed, x, xhat, xn, v, xnm1, vnm1, xt,
                       dt_eff_done, next, g);
}

// x^, x~ again from the stored levels: dt, the integrator or the levels changed between two steps (a fixed vertex: x_n, as in
// x_tilde_kernel)
__global__ void __launch_bounds__(256) bdf2_predict_kernel(int nV, const uint8_t *__restrict__ fixed,
                                                           const double *__restrict__ xn, const double *__restrict__ v,
                                                           const double *__restrict__ xnm1, const double *__restrict__ vnm1,
                                                           double *__restrict__ xhat, double *__restrict__ xt, TitPlan p, Vec3Arg gdtsq)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nV) return;
    const bool fx = fixed[i] != 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int k = 3 * i + d;
        const double xv = xn[k];
        const double xh = tit_hat(p.c0, p.c1, xv, xnm1[k]);
        const double vh = tit_hat(p.c0, p.c1, v[k], vnm1[k]);
        xhat[k] = xh;
        xt[k] = tit_x_tilde(fx, xv, xh, vh, p.dt_eff, gdtsq.v[d]);
    }
}

void launch_bdf2_predict(int nV, const uint8_t *fixed, const double *xn, const double *v, const double *xnm1,
                         const double *vnm1, double *xhat, double *xt, const TitPlan &p, const double *gdtsq, hipStream_t st)
{
    Vec3Arg g = {{gdtsq[0], gdtsq[1], gdtsq[2]}};
    hipLaunchKernelGGL(bdf2_predict_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, fixed, xn, v, xnm1, vnm1, xhat, xt, p, g);
}

// the start iterate: x~ on free vertices; a fixed vertex keeps what dotmi_set_dirichlet wrote
__global__ void __launch_bounds__(256) bdf2_init_x_kernel(int nV, const uint8_t *__restrict__ fixed, const double *__restrict__ xt,
                                                          double *__restrict__ x)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nV || fixed[i]) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) x[3 * i + d] = xt[3 * i + d];
}

void launch_bdf2_init_x(int nV, const uint8_t *fixed, const double *xt, double *x, hipStream_t st)
{
    hipLaunchKernelGGL(bdf2_init_x_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, fixed, xt, x);
}

}  // namespace dotmi
