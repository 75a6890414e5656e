// mac_reinit.hip -- reference-map reinitialisation with stored deformation on the MAC lid tier
// (benchmarks/mac_reinit_test.py:23-113, Rycroft 2018): the pieces of that loop no other
// operator of librmt covers.
//   rmt_advect_sl_rk4_multi    functions.py:194-227 for up to 8 planes on one backtrace, the
//                              solid mask (phi <= 0) folded in
//   rmt_mac_total_stress       :23-33, :74-81: F_current from the map, F_total = F_current . Fs,
//                              S = (1 - H) mu_s b
//   rmt_mac_total_force        :74-85 in one launch: the same stress, its central divergence
//                              averaged to the faces; xi and S live in LDS only
//   rmt_mac_epoch_distortion   :91-94: max J, min J and the count over phi <= 0
// Every expression keeps the reference's operand order and IEEE division (-ffp-contract=off):
// the outputs are the reference's bits but for H's sine.
#include "rmt_internal.hpp"

namespace rmt {

// --------------------------------------------------------- multi-plane advection ----
struct MrPlanes { const double *q[8]; double *out[8]; };

// k_sl_rk4 once a cell, then the foot's bilinear weights once (bilinear_t's expressions: each
// product (1 - fx) * (1 - fy) * u is ((1 - fx) * (1 - fy)) * u, so forming the weight first
// changes no bit) and NP gathers.  phi non-null: times (phi <= 0 ? 1 : 0), k_mask_solid's
// product (q * 0.0 keeps -0.0 and NaN).
template <int NP>
__global__ void __launch_bounds__(256) k_sl_rk4_multi(MrPlanes P, const double *__restrict__ a,
                                                      const double *__restrict__ b,
                                                      const double *__restrict__ X,
                                                      const double *__restrict__ Y,
                                                      const double *__restrict__ phi, int ny,
                                                      int nx, double dt, DivK Kx, DivK Ky) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    double xb, yb;
    sl_backtrace_t<false>(a, b, X[c], Y[c], dt, Kx, Ky, nx, ny, 0, ny, nullptr, xb, yb);
    const double mk = phi ? (phi[c] <= 0.0 ? 1.0 : 0.0) : 0.0;
    double x = divk(xb, Kx), y = divk(yb, Ky);
    const bool bad = !(isfinite(x) && isfinite(y));
    if (bad) x = y = 0.0;
    if (x < 0.0) x = 0.0; else if (x > nx - 1.0) x = nx - 1.0;
    if (y < 0.0) y = 0.0; else if (y > ny - 1.0) y = ny - 1.0;
    int ix = (int)floor(x), iy = (int)floor(y);
    if (ix >= nx - 1) ix = nx - 2;
    if (iy >= ny - 1) iy = ny - 2;
    const double fx = x - ix, fy = y - iy;
    const double w00 = (1 - fx) * (1 - fy), w10 = fx * (1 - fy), w01 = (1 - fx) * fy,
                 w11 = fx * fy;
    const long o = (long)iy * nx + ix;
    double r[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const double *__restrict__ q = P.q[k] + o;
        r[k] = w00 * q[0] + w10 * q[1] + w01 * q[nx] + w11 * q[nx + 1];
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        double v = bad ? __builtin_nan("") : r[k];
        if (phi) v = v * mk;
        P.out[k][c] = v;
    }
}

// ------------------------------------------------------------- total stress ----
struct TotCell { double J, F[4], S[3]; };

// One cell of :23-33 and :76-81.  x1, x2 point at the cell in a plane of row stride sy (the
// global plane or an LDS tile); (i, j), (nx, ny) are the cell and the grid (grad2's one-sided
// rows and columns); h2x = 2 dx, h2y = 2 dy.
__device__ __forceinline__ void total_stress_cell(const double *x1, const double *x2, long sy,
                                                  int i, int j, int nx, int ny, double h2x,
                                                  double h2y, double f0, double f1, double f2,
                                                  double f3, double phi, double w_t, double mu_s,
                                                  TotCell &o) {
    const double g11 = grad2(x1, 1, i, nx, h2x), g12 = grad2(x1, sy, j, ny, h2y);
    const double g21 = grad2(x2, 1, i, nx, h2x), g22 = grad2(x2, sy, j, ny, h2y);
    double detG = g11 * g22 - g12 * g21;
    if (fabs(detG) < 1e-9) detG = 1e-9;
    const double c0 = g22 / detG, c1 = -g12 / detG, c2 = -g21 / detG, c3 = g11 / detG;
    o.J = 1.0 / detG;
    const double t0 = c0 * f0 + c1 * f2, t1 = c0 * f1 + c1 * f3;
    const double t2 = c2 * f0 + c3 * f2, t3 = c2 * f1 + c3 * f3;
    o.F[0] = t0; o.F[1] = t1; o.F[2] = t2; o.F[3] = t3;
    const double b11 = t0 * t0 + t1 * t1, b12 = t0 * t2 + t1 * t3, b22 = t2 * t2 + t3 * t3;
    const double s = (1 - heaviside(phi, w_t)) * mu_s;
    o.S[0] = s * b11; o.S[1] = s * b12; o.S[2] = s * b22;
}

struct MrFs { const double *p[4]; };
struct MrFt { double *p[4]; };

__global__ void __launch_bounds__(256) k_mac_total_stress(const double *__restrict__ X1,
                                                          const double *__restrict__ X2, MrFs Fs,
                                                          const double *__restrict__ phi, int ny,
                                                          int nx, double h2x, double h2y,
                                                          double w_t, double mu_s,
                                                          double *__restrict__ Sxx,
                                                          double *__restrict__ Sxy,
                                                          double *__restrict__ Syy,
                                                          double *__restrict__ Jep, MrFt Ft) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    TotCell o;
    total_stress_cell(X1 + c, X2 + c, nx, i, j, nx, ny, h2x, h2y, Fs.p[0][c], Fs.p[1][c],
                      Fs.p[2][c], Fs.p[3][c], phi[c], w_t, mu_s, o);
    Sxx[c] = o.S[0]; Sxy[c] = o.S[1]; Syy[c] = o.S[2]; Jep[c] = o.J;
    if (Ft.p[0]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) Ft.p[k][c] = o.F[k];
    }
}

// ---------------------------------------------------------- fused face forces ----
// The face-force tile of rmt_internal.hpp with the map staged in LDS: S reaches xi one cell
// further, so xi lies on the tile + 3 left / below and + 2 right / above, clipped to the grid.
// LDS: 2 x 69 x 21 + 3 x 67 x 19 doubles = 52.5 KiB, three workgroups a CU.
constexpr int MR_XW = FF_TX + 5, MR_XH = FF_TY + 5;

__global__ void __launch_bounds__(FF_T) k_mac_total_force(const double *__restrict__ X1,
                                                          const double *__restrict__ X2, MrFs Fs,
                                                          const double *__restrict__ phi, int ny,
                                                          int nx, double h2x, double h2y,
                                                          double w_t, double mu_s,
                                                          double *__restrict__ fu,
                                                          double *__restrict__ fv,
                                                          double *__restrict__ Jep) {
    __shared__ double sx1[MR_XH * MR_XW], sx2[MR_XH * MR_XW];
    __shared__ double sxx[FF_SH * FF_SW], sxy[FF_SH * FF_SW], syy[FF_SH * FF_SW];
    const int i0 = blockIdx.x * FF_TX, j0 = blockIdx.y * FF_TY, tid = threadIdx.x;
    // xi: columns [xa, xb], rows [ya, yb]
    const int xa = max(0, i0 - 3), xb = min(nx - 1, i0 + FF_TX + 1);
    const int ya = max(0, j0 - 3), yb = min(ny - 1, j0 + FF_TY + 1);
    const int xw = xb - xa + 1, xn = xw * (yb - ya + 1);
    for (int q = tid; q < xn; q += FF_T) {
        const int r = q / xw, cc = q - r * xw;
        const long g = (long)(ya + r) * nx + xa + cc;
        sx1[r * MR_XW + cc] = X1[g];
        sx2[r * MR_XW + cc] = X2[g];
    }
    __syncthreads();
    ff_stress_region(i0, j0, nx, ny, [&](int i, int j, long g, int s, bool owned) {
        const int l = (j - ya) * MR_XW + (i - xa);
        TotCell o;
        total_stress_cell(sx1 + l, sx2 + l, MR_XW, i, j, nx, ny, h2x, h2y, Fs.p[0][g], Fs.p[1][g],
                          Fs.p[2][g], Fs.p[3][g], phi[g], w_t, mu_s, o);
        sxx[s] = o.S[0]; sxy[s] = o.S[1]; syy[s] = o.S[2];
        if (owned) Jep[g] = o.J;
    });
    __syncthreads();
    ff_faces(sxx, sxy, syy, i0, j0, nx, ny, h2x, h2y, fu, fv);                     // :82-85
}

// -------------------------------------------------------------- epoch distortion ----
// max J, min J (NaN propagates, as ndarray.max / min) and the count over phi <= 0: order-free,
// so exact.  MR_RB workgroups of MR_T threads leave partials in ctx->red, one workgroup folds
// them.
constexpr int MR_RB = 256, MR_T = 256;
__device__ __forceinline__ void mr_fold(double *smx, double *smn, double *sct, double &mx,
                                        double &mn, double &ct) {
    const int t = threadIdx.x;
    smx[t] = mx; smn[t] = mn; sct[t] = ct;
    __syncthreads();
    tree_fold<MR_T>([&](int t, int u) {
        smx[t] = nanmax(smx[t], smx[u]);
        smn[t] = nanmin(smn[t], smn[u]);
        sct[t] = sct[t] + sct[u];
    });
    mx = smx[0]; mn = smn[0]; ct = sct[0];
}
__global__ void __launch_bounds__(MR_T) k_mac_epoch_p1(const double *__restrict__ J,
                                                       const double *__restrict__ phi, long n,
                                                       double *__restrict__ part) {
    __shared__ double smx[MR_T], smn[MR_T], sct[MR_T];
    double mx = -INFINITY, mn = INFINITY, ct = 0.0;
    for (long k = blockIdx.x * (long)MR_T + threadIdx.x; k < n; k += (long)MR_RB * MR_T)
        if (phi[k] <= 0.0) {
            mx = nanmax(mx, J[k]); mn = nanmin(mn, J[k]); ct += 1.0;
        }
    mr_fold(smx, smn, sct, mx, mn, ct);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mx; part[MR_RB + blockIdx.x] = mn; part[2 * MR_RB + blockIdx.x] = ct;
    }
}
__global__ void __launch_bounds__(MR_T) k_mac_epoch_p2(const double *__restrict__ part,
                                                       double *__restrict__ out3) {
    __shared__ double smx[MR_T], smn[MR_T], sct[MR_T];
    static_assert(MR_RB == MR_T, "one partial a thread");
    double mx = part[threadIdx.x], mn = part[MR_RB + threadIdx.x], ct = part[2 * MR_RB + threadIdx.x];
    mr_fold(smx, smn, sct, mx, mn, ct);
    if (threadIdx.x == 0) { out3[0] = mx; out3[1] = mn; out3[2] = ct; }
}
static_assert(3 * MR_RB <= RED_BLOCKS + 64, "ctx->red holds the partials");

}  // namespace rmt
using namespace rmt;

template <int NP>
static void launch_multi(rmt_ctx *ctx, const MrPlanes &P, const double *a, const double *b,
                         const double *X, const double *Y, const double *phi, double dt,
                         double dx, double dy) {
    k_sl_rk4_multi<NP><<<grid1d(N_CELLS, 256), 256, 0, ctx->stream>>>(
        P, a, b, X, Y, phi, ctx->ny, ctx->nx, dt, divk_make(dx), divk_make(dy));
}

int rmt_advect_sl_rk4_multi(rmt_ctx *ctx, int np, const double *const *q, const double *a,
                            const double *b, const double *X, const double *Y, double dt,
                            double dx, double dy, const double *phi, double *const *out) {
    RMT_CHECK(ctx && q && a && b && X && Y && out, RMT_EINVAL, "null argument");
    RMT_CHECK(np >= 1 && np <= 8, RMT_EINVAL, "rmt_advect_sl_rk4_multi: 1..8 planes");
    MrPlanes P = {};
    for (int k = 0; k < np; ++k) {
        RMT_CHECK(q[k] && out[k], RMT_EINVAL, "rmt_advect_sl_rk4_multi: null plane");
        for (int m = 0; m < np; ++m)
            RMT_CHECK(out[k] != q[m], RMT_EINVAL,
                      "rmt_advect_sl_rk4_multi: an output plane is an input plane");
        P.q[k] = q[k]; P.out[k] = out[k];
    }
    switch (np) {
#define MR_CASE(n) case n: launch_multi<n>(ctx, P, a, b, X, Y, phi, dt, dx, dy); break;
        MR_CASE(1) MR_CASE(2) MR_CASE(3) MR_CASE(4) MR_CASE(5) MR_CASE(6) MR_CASE(7) MR_CASE(8)
#undef MR_CASE
    }
    RMT_LAUNCHED();
    return RMT_OK;
}

static int mr_fs(const double *const *Fs, MrFs &o) {
    RMT_CHECK(Fs, RMT_EINVAL, "null argument");
    for (int k = 0; k < 4; ++k) {
        RMT_CHECK(Fs[k], RMT_EINVAL, "null Fs plane");
        o.p[k] = Fs[k];
    }
    return RMT_OK;
}

int rmt_mac_total_stress(rmt_ctx *ctx, const double *X1, const double *X2,
                         const double *const *Fs, const double *phi, double dx, double dy,
                         double w_t, double mu_s, double *Sxx, double *Sxy, double *Syy,
                         double *J_ep, double *const *Ftot) {
    RMT_CHECK(ctx && X1 && X2 && phi && Sxx && Sxy && Syy && J_ep, RMT_EINVAL, "null argument");
    MrFs F; MrFt T = {};
    RMT_TRY(mr_fs(Fs, F));
    if (Ftot)
        for (int k = 0; k < 4; ++k) {
            RMT_CHECK(Ftot[k], RMT_EINVAL, "null Ftot plane");
            T.p[k] = Ftot[k];
        }
    k_mac_total_stress<<<grid1d(N_CELLS, 256), 256, 0, ctx->stream>>>(
        X1, X2, F, phi, ctx->ny, ctx->nx, 2 * dx, 2 * dy, w_t, mu_s, Sxx, Sxy, Syy, J_ep, T);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_total_force(rmt_ctx *ctx, const double *X1, const double *X2,
                        const double *const *Fs, const double *phi, double dx, double dy,
                        double w_t, double mu_s, double *fu, double *fv, double *J_ep) {
    RMT_CHECK(ctx && X1 && X2 && phi && fu && fv && J_ep, RMT_EINVAL, "null argument");
    MrFs F;
    RMT_TRY(mr_fs(Fs, F));
    const dim3 grid((ctx->nx + FF_TX - 1) / FF_TX, (ctx->ny + FF_TY - 1) / FF_TY);
    k_mac_total_force<<<grid, FF_T, 0, ctx->stream>>>(X1, X2, F, phi, ctx->ny, ctx->nx, 2 * dx,
                                                      2 * dy, w_t, mu_s, fu, fv, J_ep);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_epoch_distortion(rmt_ctx *ctx, const double *J_ep, const double *phi, double *out3) {
    RMT_CHECK(ctx && J_ep && phi && out3, RMT_EINVAL, "null argument");
    k_mac_epoch_p1<<<MR_RB, MR_T, 0, ctx->stream>>>(J_ep, phi, N_CELLS, ctx->red);
    k_mac_epoch_p2<<<1, MR_T, 0, ctx->stream>>>(ctx->red, out3);
    RMT_LAUNCHED();
    return RMT_OK;
}
