// mac_soft.hip -- the soft disc in the lid cavity under the integrator ladder
// (benchmarks/mac_soft_disc_lid.py:79-150): the pieces of that loop no other operator of
// librmt covers.
//   rmt_mac_solid_force             :103-110 in one launch: solid_cauchy_stress (w_cut = 0), the
//                                   (1 - H) blend, the central divergence, the face average;
//                                   the blended stress lives in LDS only
//   rmt_mac_midpoint_centres        :133-134 (and :82-83 with u0 == u1): the mean of two face
//                                   fields averaged to the cell centres
//   rmt_mac_soft_diag               :139-150: everything the stop test and the record read
//   rmt_mac_advect_xi_conservative  mac.py:698-721: SSP-RK3 of -H div(u xi) on the face velocity
// Every expression keeps the reference's operand order and IEEE division (-ffp-contract=off):
// the outputs are the reference's bits but for H's sine and the order of the two sums.
#include "rmt_internal.hpp"

namespace rmt {

// ------------------------------------------------------------ fused face forces ----
// The face-force tile of rmt_internal.hpp.  The map and phi are read from global memory through
// solid_stress_cell, the operator's own cell function: outside phi <= 0 it returns after one
// load.  LDS: 3 x 67 x 19 doubles = 29.8 KiB.
__global__ void __launch_bounds__(FF_T) k_mac_solid_force(const double *__restrict__ X1,
                                                          const double *__restrict__ X2,
                                                          const double *__restrict__ phi, int ny,
                                                          int nx, double dx, double dy, double w_t,
                                                          double mu_s, double kappa, double clamp,
                                                          int iso, double *__restrict__ fu,
                                                          double *__restrict__ fv,
                                                          double *__restrict__ J) {
    __shared__ double sxx[FF_SH * FF_SW], sxy[FF_SH * FF_SW], syy[FF_SH * FF_SW];
    const int i0 = blockIdx.x * FF_TX, j0 = blockIdx.y * FF_TY;
    const double h2x = 2 * dx, h2y = 2 * dy;
    ff_stress_region(i0, j0, nx, ny, [&](int i, int j, long g, int l, bool owned) {
        Stress s{0.0, 0.0, 0.0, 1.0};
        if (j >= 1 && j < ny - 1 && i >= 1 && i < nx - 1)
            solid_stress_cell(X1, X2, phi, g, nx, dx, dy, mu_s, kappa, 0.0, clamp, iso != 0, s);
        const double b = 1 - heaviside(phi[g], w_t);
        sxx[l] = b * s.sxx; sxy[l] = b * s.sxy; syy[l] = b * s.syy;
        if (owned) J[g] = s.J;
    });
    __syncthreads();
    ff_faces(sxx, sxy, syy, i0, j0, nx, ny, h2x, h2y, fu, fv);                     // :107-110
}

// ------------------------------------------------------------- midpoint centres ----
__global__ void __launch_bounds__(256) k_mac_midpoint_centres(const double *__restrict__ u0,
                                                              const double *__restrict__ v0,
                                                              const double *__restrict__ u1,
                                                              const double *__restrict__ v1,
                                                              int ny, int nx,
                                                              double *__restrict__ uc,
                                                              double *__restrict__ vc) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const long f = (long)j * (nx + 1) + i;
    const double ul = 0.5 * (u0[f] + u1[f]), ur = 0.5 * (u0[f + 1] + u1[f + 1]);
    const double vd = 0.5 * (v0[c] + v1[c]), vu = 0.5 * (v0[c + nx] + v1[c + nx]);
    uc[c] = 0.5 * (ul + ur);
    vc[c] = 0.5 * (vd + vu);
}

// ------------------------------------------------------------------ diagnostics ----
// out8: the count of phi <= 0, the sums of Xc and Yc over them (Xc = (i + 0.5) dx as the
// driver's meshgrid), min J, max J (NaN propagates, as ndarray.min / max), max|u|, max|v| (the
// same) and 1.0 if u or v holds a non-finite value.  MS_RB workgroups of MS_T threads leave
// partials in ctx->red, one workgroup folds them: a fixed order, so the sums repeat bit for bit.
constexpr int MS_RB = 128, MS_T = 256, MS_NQ = 8;
static_assert(MS_NQ * MS_RB <= RED_BLOCKS + 64, "ctx->red holds the partials");
struct SoftAcc { double q[MS_NQ]; };
__device__ __forceinline__ SoftAcc soft_identity() {
    return {{0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0, 0.0, 0.0}};
}
__device__ __forceinline__ void soft_merge(SoftAcc &a, const SoftAcc &b) {
    a.q[0] = a.q[0] + b.q[0]; a.q[1] = a.q[1] + b.q[1]; a.q[2] = a.q[2] + b.q[2];
    a.q[3] = nanmin(a.q[3], b.q[3]); a.q[4] = nanmax(a.q[4], b.q[4]);
    a.q[5] = nanmax(a.q[5], b.q[5]); a.q[6] = nanmax(a.q[6], b.q[6]);
    a.q[7] = nanmax(a.q[7], b.q[7]);
}
__device__ __forceinline__ void soft_fold(SoftAcc *sh, SoftAcc &a) {
    sh[threadIdx.x] = a;
    __syncthreads();
    tree_fold<MS_T>([&](int t, int u) { soft_merge(sh[t], sh[u]); });
    a = sh[0];
}
__global__ void __launch_bounds__(MS_T) k_mac_soft_diag_p1(const double *__restrict__ phi,
                                                           const double *__restrict__ J,
                                                           const double *__restrict__ u,
                                                           const double *__restrict__ v, int ny,
                                                           int nx, double dx, double dy,
                                                           double *__restrict__ part) {
    __shared__ SoftAcc sh[MS_T];
    SoftAcc a = soft_identity();
    const long stride = (long)MS_RB * MS_T, first = blockIdx.x * (long)MS_T + threadIdx.x;
    const long n = (long)ny * nx, nu = (long)ny * (nx + 1), nv = (long)(ny + 1) * nx;
    for (long k = first; k < n; k += stride) {
        a.q[3] = nanmin(a.q[3], J[k]); a.q[4] = nanmax(a.q[4], J[k]);
        if (phi[k] <= 0.0) {
            const int j = (int)(k / nx), i = (int)(k % nx);
            a.q[0] += 1.0; a.q[1] += (i + 0.5) * dx; a.q[2] += (j + 0.5) * dy;
        }
    }
    for (long k = first; k < nu; k += stride) {
        a.q[5] = nanmax(a.q[5], fabs(u[k]));
        if (!isfinite(u[k])) a.q[7] = 1.0;
    }
    for (long k = first; k < nv; k += stride) {
        a.q[6] = nanmax(a.q[6], fabs(v[k]));
        if (!isfinite(v[k])) a.q[7] = 1.0;
    }
    soft_fold(sh, a);
    if (threadIdx.x == 0)
        for (int m = 0; m < MS_NQ; ++m) part[m * MS_RB + blockIdx.x] = a.q[m];
}
__global__ void __launch_bounds__(MS_T) k_mac_soft_diag_p2(const double *__restrict__ part,
                                                           double *__restrict__ out8) {
    __shared__ SoftAcc sh[MS_T];
    SoftAcc a = soft_identity();
    if (threadIdx.x < MS_RB)
        for (int m = 0; m < MS_NQ; ++m) a.q[m] = part[m * MS_RB + threadIdx.x];
    soft_fold(sh, a);
    if (threadIdx.x == 0)
        for (int m = 0; m < MS_NQ; ++m) out8[m] = a.q[m];
}

// ------------------------------------------------------- conservative advection ----
// One SSP-RK3 stage of mac.py:713-721 at a cell: r = -H * div(u q) with q at the faces the
// two-cell average (the edge value at the walls), then
//   STAGE 1: q + dt r                        (q is xi)
//   STAGE 2: 0.75 xi + 0.25 (q + dt r)
//   STAGE 3: (1/3) xi + (2/3) (q + dt r)
template <int STAGE>
__global__ void __launch_bounds__(256) k_mac_xi_cons_stage(const double *__restrict__ xi,
                                                           const double *__restrict__ q,
                                                           const double *__restrict__ u,
                                                           const double *__restrict__ v,
                                                           const double *__restrict__ phi, int ny,
                                                           int nx, double dx, double dy, double dt,
                                                           double w_cut, double *__restrict__ out) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const long f = (long)j * (nx + 1) + i;
    const double qc = q[c];
    const double ql = i > 0 ? 0.5 * (q[c - 1] + qc) : qc;
    const double qr = i < nx - 1 ? 0.5 * (qc + q[c + 1]) : qc;
    const double qd = j > 0 ? 0.5 * (q[c - nx] + qc) : qc;
    const double qu = j < ny - 1 ? 0.5 * (qc + q[c + nx]) : qc;
    const double div = (u[f + 1] * qr - u[f] * ql) / dx + (v[c + nx] * qu - v[c] * qd) / dy;
    const double H = phi[c] <= w_cut ? 1.0 : 0.0;
    const double e = qc + dt * (-H * div);
    if (STAGE == 1) out[c] = e;
    else if (STAGE == 2) out[c] = 0.75 * xi[c] + 0.25 * e;
    else out[c] = (1.0 / 3.0) * xi[c] + (2.0 / 3.0) * e;
}

}  // namespace rmt
using namespace rmt;

int rmt_mac_solid_force(rmt_ctx *ctx, const double *X1, const double *X2, const double *phi,
                        double dx, double dy, double w_t, double mu_s, double kappa,
                        double detg_clamp, int isochoric, double *fu, double *fv, double *J) {
    RMT_CHECK(ctx && X1 && X2 && phi && fu && fv && J, RMT_EINVAL, "null argument");
    const dim3 grid((ctx->nx + FF_TX - 1) / FF_TX, (ctx->ny + FF_TY - 1) / FF_TY);
    k_mac_solid_force<<<grid, FF_T, 0, ctx->stream>>>(X1, X2, phi, ctx->ny, ctx->nx, dx, dy, w_t,
                                                      mu_s, kappa, detg_clamp, isochoric, fu, fv,
                                                      J);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_midpoint_centres(rmt_ctx *ctx, const double *u0, const double *v0, const double *u1,
                             const double *v1, double *uc, double *vc) {
    RMT_CHECK(ctx && u0 && v0 && u1 && v1 && uc && vc, RMT_EINVAL, "null argument");
    k_mac_midpoint_centres<<<grid1d(N_CELLS, 256), 256, 0, ctx->stream>>>(u0, v0, u1, v1, ctx->ny,
                                                                          ctx->nx, uc, vc);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_soft_diag(rmt_ctx *ctx, const double *phi, const double *J, const double *u,
                      const double *v, double dx, double dy, double *out8) {
    RMT_CHECK(ctx && phi && J && u && v && out8, RMT_EINVAL, "null argument");
    k_mac_soft_diag_p1<<<MS_RB, MS_T, 0, ctx->stream>>>(phi, J, u, v, ctx->ny, ctx->nx, dx, dy,
                                                        ctx->red);
    k_mac_soft_diag_p2<<<1, MS_T, 0, ctx->stream>>>(ctx->red, out8);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_advect_xi_conservative(rmt_ctx *ctx, const double *xi, const double *u,
                                   const double *v, double dx, double dy, double dt,
                                   const double *phi, double w_cut, double *out) {
    RMT_CHECK(ctx && xi && u && v && phi && out, RMT_EINVAL, "null argument");
    RMT_CHECK(out != xi, RMT_EINVAL, "rmt_mac_advect_xi_conservative: out is xi");
    const long n = N_CELLS;
    RMT_TRY(ensure_scratch(ctx, 2 * n * sizeof(double)));
    double *q1 = ctx->scratch, *q2 = ctx->scratch + n;
    const int ny = ctx->ny, nx = ctx->nx;
    const unsigned g = grid1d(n, 256);
    k_mac_xi_cons_stage<1><<<g, 256, 0, ctx->stream>>>(xi, xi, u, v, phi, ny, nx, dx, dy, dt,
                                                       w_cut, q1);
    k_mac_xi_cons_stage<2><<<g, 256, 0, ctx->stream>>>(xi, q1, u, v, phi, ny, nx, dx, dy, dt,
                                                       w_cut, q2);
    k_mac_xi_cons_stage<3><<<g, 256, 0, ctx->stream>>>(xi, q2, u, v, phi, ny, nx, dx, dy, dt,
                                                       w_cut, out);
    RMT_LAUNCHED();
    return RMT_OK;
}
