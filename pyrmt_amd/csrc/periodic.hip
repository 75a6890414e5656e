// periodic.hip -- functions.py:1177-1290, the doubly-periodic projection branch (A25).
//
// The collocated grid carries an overlap row / column (x[-1] == x[0] physically); the
// periodic field lives on the reduced (ny-1) x (nx-1) sub-grid.  Operators: wide central
// divergence / gradient with wrap-around on the reduced grid, tiled back onto the overlap
// grid (_tile_overlap :1205-1213); the Poisson solve is a 2D real FFT of the reduced rhs
// (rocFFT D2Z / Z2D, the reference uses numpy.fft), divided by the separable symbol
// -sin^2(2 pi k / m) / h^2 per axis (m = nx - 1, ny - 1) with the null modes (|eig| < 1e-12:
// constant and Nyquist) zeroed; means by the row-tree reduction.
#include "rocfft_util.hpp"
#include <algorithm>
#include <vector>

namespace rmt {

struct PerPlan {
    int mx = 0, my = 0;
    RocfftPlans fft;   // [0] D2Z, [1] Z2D
    double *red = nullptr, *C = nullptr, *lamx = nullptr, *lamy = nullptr, *g = nullptr;
};

void per_destroy(PerPlan *P) {
    if (!P) return;
    (void)hipFree(P->red); (void)hipFree(P->C); (void)hipFree(P->lamx); (void)hipFree(P->lamy);
    (void)hipFree(P->g);
    delete P;
}

static int per_plan(rmt_ctx *ctx, const double *lamx, const double *lamy) {
    const int mx = ctx->nx - 1, my = ctx->ny - 1;
    RMT_CHECK(mx >= 2 && my >= 2, RMT_EINVAL, "periodic solve: ny, nx >= 3");
    PerPlan *P = ctx->per;
    if (!P || P->mx != mx || P->my != my) {
        if (P) per_destroy(P);
        P = ctx->per = new PerPlan;
        P->mx = mx; P->my = my;
        RMT_TRY(rocfft_ready());
        const size_t len[2] = {(size_t)mx, (size_t)my};   // fastest axis first
        RMT_TRY(rocfft_ok(rocfft_plan_create(&P->fft.plan[0], rocfft_placement_notinplace,
                                             rocfft_transform_type_real_forward,
                                             rocfft_precision_double, 2, len, 1, nullptr),
                          "periodic plan fwd"));
        RMT_TRY(rocfft_ok(rocfft_plan_create(&P->fft.plan[1], rocfft_placement_notinplace,
                                             rocfft_transform_type_real_inverse,
                                             rocfft_precision_double, 2, len, 1, nullptr),
                          "periodic plan inv"));
        RMT_TRY(P->fft.finish());
        RMT_HIP(hipMalloc(&P->red, (size_t)my * mx * sizeof(double)));
        RMT_HIP(hipMalloc(&P->C, (size_t)my * (mx / 2 + 1) * 2 * sizeof(double)));
        RMT_HIP(hipMalloc(&P->lamx, mx * sizeof(double)));
        RMT_HIP(hipMalloc(&P->lamy, my * sizeof(double)));
        RMT_HIP(hipMalloc(&P->g, 2 * (size_t)ctx->ny * ctx->nx * sizeof(double)));
    }
    RMT_HIP(hipMemcpyAsync(P->lamx, lamx, mx * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipMemcpyAsync(P->lamy, lamy, my * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    return RMT_OK;
}

// functions.py:1236-1252: (roll(f, -1) - roll(f, 1)) / 2h on the reduced grid, tiled
__global__ void k_per_grad(const double *__restrict__ a, const double *__restrict__ b, int ny,
                           int nx, double dx, double dy, int mode, double *__restrict__ o1,
                           double *__restrict__ o2) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int mx = nx - 1, my = ny - 1;
    const int j = (int)(c / nx) % my, i = (int)(c % nx) % mx;   // tile overlap
    const int ip = (i + 1) % mx, im = (i + mx - 1) % mx, jp = (j + 1) % my, jm = (j + my - 1) % my;
    const double ddx = (a[(long)j * nx + ip] - a[(long)j * nx + im]) / (2.0 * dx);
    const double *f = mode ? a : b;   // mode 0: divergence of (a, b); 1: gradient of a
    const double ddy = (f[(long)jp * nx + i] - f[(long)jm * nx + i]) / (2.0 * dy);
    if (mode == 0) o1[c] = ddx + ddy;
    else { o1[c] = ddx; o2[c] = ddy; }
}

__global__ void k_per_extract(const double *__restrict__ full, int ny, int nx, double s,
                              double dt, double *__restrict__ red) {
    const int mx = nx - 1, my = ny - 1;
    const long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (q >= (long)my * mx) return;
    const int j = (int)(q / mx), i = (int)(q % mx);
    // rhs_2d = rho_bar * divU / dt (functions.py:1282), then r = rhs[:-1, :-1]
    red[q] = dt > 0 ? (s * full[(long)j * nx + i]) / dt : full[(long)j * nx + i];
}

// phat = rhat / eig, null modes (|eig| < 1e-12) -> 0 (functions.py:1196-1201, 1228-1229)
__global__ void k_per_divide(double2 *__restrict__ C, int my, int mx,
                             const double *__restrict__ lamx, const double *__restrict__ lamy) {
    const int h = mx / 2 + 1;
    const long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (q >= (long)my * h) return;
    const int ky = (int)(q / h), kx = (int)(q % h);
    const double e = lamx[kx] + lamy[ky];
    const double2 z = C[q];
    C[q] = fabs(e) < 1e-12 ? make_double2(0.0, 0.0) : make_double2(z.x / e, z.y / e);
}

__global__ void k_per_tile(const double *__restrict__ red, int ny, int nx, double scale,
                           double *__restrict__ out) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int mx = nx - 1, my = ny - 1;
    out[c] = red[(long)((int)(c / nx) % my) * mx + (int)(c % nx) % mx] * scale;
}

// correction with the local or scalar density, BC by source cell, p accumulation
__global__ void k_per_correct(const double *__restrict__ as, const double *__restrict__ bs,
                              const double *__restrict__ gx, const double *__restrict__ gy,
                              const double *__restrict__ rho, double rho_s, double dt, int ny,
                              int nx, int bc, double lid, const double *__restrict__ pc,
                              const double *__restrict__ p_prev, double *__restrict__ a,
                              double *__restrict__ b, double *__restrict__ p) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const BCSrc s = bc_source(bc, lid, (int)(c / nx), (int)(c % nx), ny, nx);
    auto cu = [&](long k) { return as[k] - (dt / (rho ? rho[k] : rho_s)) * gx[k]; };
    auto cv = [&](long k) { return bs[k] - (dt / (rho ? rho[k] : rho_s)) * gy[k]; };
    a[c] = s.u_const ? s.u_val : cu(s.u_src);
    b[c] = s.v_const ? s.v_val : cv(s.v_src);
    p[c] = p_prev ? p_prev[c] + pc[c] : pc[c];
}

// functions.py:1216-1233 on device buffers: rhs_full (ny x nx) -> p (ny x nx); rhs scaled by
// s / dt first when dt > 0
static int per_solve(rmt_ctx *ctx, const double *rhs, double s, double dt, double *p) {
    PerPlan *P = ctx->per;
    const int ny = ctx->ny, nx = ctx->nx, mx = P->mx, my = P->my;
    const long nr = (long)my * mx, nn = (long)ny * nx;
    hipStream_t st = ctx->stream;
    k_per_extract<<<grid1d(nr, 256), 256, 0, st>>>(rhs, ny, nx, s, dt, P->red);
    RMT_LAUNCHED();
    RMT_TRY(sub_mean_rows(ctx, P->red, my, mx));                     // r -= mean(r)
    RMT_TRY(P->fft.on(st));
    void *in[1] = {P->red}, *out[1] = {P->C};
    RMT_TRY(rocfft_ok(rocfft_execute(P->fft.plan[0], in, out, P->fft.info), "periodic execute fwd"));
    k_per_divide<<<grid1d((long)my * (mx / 2 + 1), 256), 256, 0, st>>>((double2 *)P->C, my, mx,
                                                                         P->lamx, P->lamy);
    RMT_LAUNCHED();
    void *in2[1] = {P->C}, *out2[1] = {P->red};
    RMT_TRY(rocfft_ok(rocfft_execute(P->fft.plan[1], in2, out2, P->fft.info), "periodic execute inv"));
    k_per_tile<<<grid1d(nn, 256), 256, 0, st>>>(P->red, ny, nx, 1.0 / ((double)my * mx), p);
    RMT_LAUNCHED();
    return sub_mean_rows(ctx, p, ny, nx);                            // p -= mean(p)
}

}  // namespace rmt

using namespace rmt;

extern "C" {

int rmt_divergence_periodic(rmt_ctx *ctx, const double *a, const double *b, double dx, double dy,
                            double *divU) {
    RMT_CHECK(ctx && a && b && divU && ctx->ny >= 3 && ctx->nx >= 3, RMT_EINVAL,
              "bad argument");
    const long n = (long)ctx->ny * ctx->nx;
    k_per_grad<<<grid1d(n, 256), 256, 0, ctx->stream>>>(a, b, ctx->ny, ctx->nx, dx, dy, 0, divU,
                                                        nullptr);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_pressure_gradient_periodic(rmt_ctx *ctx, const double *p, double dx, double dy,
                                   double *gx, double *gy) {
    RMT_CHECK(ctx && p && gx && gy && ctx->ny >= 3 && ctx->nx >= 3, RMT_EINVAL,
              "bad argument");
    const long n = (long)ctx->ny * ctx->nx;
    k_per_grad<<<grid1d(n, 256), 256, 0, ctx->stream>>>(p, p, ctx->ny, ctx->nx, dx, dy, 1, gx, gy);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_solve_poisson_fft(rmt_ctx *ctx, const double *rhs, const double *lamx, const double *lamy,
                          double *p) {
    RMT_CHECK(ctx && rhs && lamx && lamy && p, RMT_EINVAL, "bad argument");
    RMT_TRY(per_plan(ctx, lamx, lamy));
    return per_solve(ctx, rhs, 1.0, 0.0, p);
}

int rmt_pressure_projection_periodic(rmt_ctx *ctx, const double *a_star, const double *b_star,
                                     double dx, double dy, double dt, double rho_bar,
                                     const double *rho_cells, int bc_kind, double lid,
                                     const double *lamx, const double *lamy,
                                     const double *p_prev, double *a, double *b, double *p) {
    RMT_CHECK(ctx && a_star && b_star && lamx && lamy && a && b && p, RMT_EINVAL, "bad argument");
    RMT_CHECK(bc_kind >= 0 && bc_kind <= 3, RMT_EINVAL, "unknown velocity bc kind");
    RMT_TRY(per_plan(ctx, lamx, lamy));
    PerPlan *P = ctx->per;
    const int ny = ctx->ny, nx = ctx->nx;
    const long n = (long)ny * nx;
    RMT_TRY(ensure_scratch(ctx, n * sizeof(double)));
    double *div = P->g, *pc = ctx->scratch, *gx = P->g, *gy = P->g + n;
    k_per_grad<<<grid1d(n, 256), 256, 0, ctx->stream>>>(a_star, b_star, ny, nx, dx, dy, 0, div,
                                                        nullptr);
    RMT_LAUNCHED();
    RMT_TRY(per_solve(ctx, div, rho_bar, dt, pc));
    k_per_grad<<<grid1d(n, 256), 256, 0, ctx->stream>>>(pc, pc, ny, nx, dx, dy, 1, gx, gy);
    k_per_correct<<<grid1d(n, 256), 256, 0, ctx->stream>>>(a_star, b_star, gx, gy, rho_cells,
                                                           rho_bar, dt, ny, nx, bc_kind, lid, pc,
                                                           p_prev, a, b, p);
    RMT_LAUNCHED();
    return sub_mean_rows(ctx, p, ny, nx);
}

}  // extern "C"
