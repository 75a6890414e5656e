// macper.hpp -- what the periodic staggered (MAC) tier's two translation units share
// (macper.hip: stencils, FFT solves, the explicit / IMEX loop; macper_sl.hip: grid-wrap cubic
// splines, the semi-Lagrangian predictor and its loop): the face arithmetic of the central
// predictor, the context's workspace layout and the launch helpers around the FFT pair.
#pragma once
#include "rmt_internal.hpp"

namespace rmt {

struct MacpCoef { double nu, dx2, dy2, twodx, twody, dt; };

// mac.py:639-644 (imex 0: u + dt * ru) and :530-532, 538 (imex 1: u - dt * adv_u) at one
// u-face; v00 .. vNW: _v_at_u_per's four terms in its order (v, west, north, north-west)
__device__ __forceinline__ double macp_ustar(double uc, double uE, double uW, double uN,
                                             double uS, double v00, double vW, double vN,
                                             double vNW, const MacpCoef &k, int imex) {
    const double dudx = (uE - uW) / k.twodx;
    const double dudy = (uN - uS) / k.twody;
    const double vau = 0.25 * (((v00 + vW) + vN) + vNW);
    const double adv = uc * dudx + vau * dudy;
    if (imex) return uc - k.dt * adv;
    const double lap = ((uE - 2.0 * uc) + uW) / k.dx2 + ((uN - 2.0 * uc) + uS) / k.dy2;
    const double ru = -adv + k.nu * lap;
    return uc + k.dt * ru;
}

// mac.py:645-650 / :534-536, 539 at one v-face; u00 .. uSE: _u_at_v_per's four terms in its
// order (u, east, south, south-east)
__device__ __forceinline__ double macp_vstar(double vc, double vE, double vW, double vN,
                                             double vS, double u00, double uE, double uS,
                                             double uSE, const MacpCoef &k, int imex) {
    const double dvdx = (vE - vW) / k.twodx;
    const double dvdy = (vN - vS) / k.twody;
    const double uav = 0.25 * (((u00 + uE) + uS) + uSE);
    const double adv = uav * dvdx + vc * dvdy;
    if (imex) return vc - k.dt * adv;
    const double lap = ((vE - 2.0 * vc) + vW) / k.dx2 + ((vN - 2.0 * vc) + vS) / k.dy2;
    const double rv = -adv + k.nu * lap;
    return vc + k.dt * rv;
}

__device__ __forceinline__ int macp_wrap(int i, int n) {
    i %= n;
    return i < 0 ? i + n : i;
}

// Workspace of the context, in doubles: the half-spectrum first (16-byte aligned), then
// `planes` real planes of ny * nx rounded up to an even count, then `tail` doubles.
inline size_t macp_spec(const rmt_ctx *ctx) { return 2 * (size_t)ctx->ny * (ctx->nx / 2 + 1); }
inline size_t macp_plane(const rmt_ctx *ctx) {
    return ((size_t)ctx->ny * ctx->nx + 1) & ~(size_t)1;
}
int macp_workspace(rmt_ctx *ctx, int planes, size_t tail = 0);
// the context's plan for its (ny, nx) (made once), with the call's symbol uploaded
int macp_plan(rmt_ctx *ctx, const double *lx, const double *ly);
// in -> out (may be the same plane) through the half-spectrum; mode 0 Poisson, 1 Helmholtz
int macp_solve(rmt_ctx *ctx, const double *in, int mode, double coef, double *out);
int macp_div(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy, double s,
             double *out);
// mac.py:476-480 from the scaled divergence in phi: solve in place, correct
int macp_project_rhs(rmt_ctx *ctx, const double *us, const double *vs, double dx, double dy,
                     double dt_rho, double *u, double *v, double *phi);

}  // namespace rmt
