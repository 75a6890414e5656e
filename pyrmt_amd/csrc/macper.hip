// macper.hip -- mac.py:445-540, 636-650, the periodic staggered (MAC) tier, and the loop of
// benchmarks/mac_taylor_green_convergence.py:59-66.
//
// u (x-faces), v (y-faces) and p (centres) are all (ny, nx) planes, i fastest, and every
// index wraps (np.roll).  The stencil kernels keep the reference's operation order and are
// bit-exact; the Poisson / Helmholtz solves are a rocFFT 2D D2Z, one symbol kernel on the
// ny x (nx/2+1) half-spectrum and Z2D (the reference: numpy.fft.fft2 / ifft2, pocketfft), equal
// to rounding.  The loop's explicit step is two stencil kernels around the FFT pair:
// k_macp_predict_div (option macp_fused) and k_macp_correct.
#include "macper.hpp"
#include "rocfft_util.hpp"

namespace rmt {

struct MacPerPlan {
    int ny = 0, nx = 0;
    RocfftPlans fft;   // [0] D2Z, [1] Z2D
    double *lx = nullptr, *ly = nullptr;   // the per-axis symbol of the call in flight
};

void macper_destroy(MacPerPlan *P) {
    if (!P) return;
    (void)hipFree(P->lx); (void)hipFree(P->ly);
    delete P;
}

// The context's plan for its (ny, nx) (made once), with the call's symbol uploaded.
int macp_plan(rmt_ctx *ctx, const double *lx, const double *ly) {
    const int ny = ctx->ny, nx = ctx->nx;
    RMT_CHECK(ny >= 2 && nx >= 2, RMT_EINVAL, "periodic MAC solve: ny, nx >= 2");
    MacPerPlan *P = ctx->macper;
    if (!P || P->ny != ny || P->nx != nx) {
        if (P) macper_destroy(P);
        P = ctx->macper = new MacPerPlan;
        P->ny = ny; P->nx = nx;
        RMT_TRY(rocfft_ready());
        const size_t len[2] = {(size_t)nx, (size_t)ny};   // fastest first
        RMT_TRY(rocfft_ok(rocfft_plan_create(&P->fft.plan[0], rocfft_placement_notinplace,
                                             rocfft_transform_type_real_forward,
                                             rocfft_precision_double, 2, len, 1, nullptr),
                          "periodic MAC plan fwd"));
        RMT_TRY(rocfft_ok(rocfft_plan_create(&P->fft.plan[1], rocfft_placement_notinplace,
                                             rocfft_transform_type_real_inverse,
                                             rocfft_precision_double, 2, len, 1, nullptr),
                          "periodic MAC plan inv"));
        RMT_TRY(P->fft.finish());
        RMT_HIP(hipMalloc(&P->lx, nx * sizeof(double)));
        RMT_HIP(hipMalloc(&P->ly, ny * sizeof(double)));
    }
    RMT_HIP(hipMemcpyAsync(P->lx, lx, nx * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipMemcpyAsync(P->ly, ly, ny * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    return RMT_OK;
}

// the workspace laid out in macper.hpp
int macp_workspace(rmt_ctx *ctx, int planes, size_t tail) {
    return ensure_scratch(ctx,
                          (macp_spec(ctx) + planes * macp_plane(ctx) + tail) * sizeof(double));
}

// mac.py:449-450, times s (project_per's rho / dt; 1.0 is exact)
__global__ void k_macp_div(const double *__restrict__ u, const double *__restrict__ v, int ny,
                           int nx, double dx, double dy, double s, double *__restrict__ out) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int ip = i + 1 == nx ? 0 : i + 1, jp = j + 1 == ny ? 0 : j + 1;
    out[c] = s * ((u[(long)j * nx + ip] - u[c]) / dx + (v[(long)jp * nx + i] - v[c]) / dy);
}

// mac.py:453-458 (gu or gv may be null)
__global__ void k_macp_grad(const double *__restrict__ p, int ny, int nx, double dx, double dy,
                            double *__restrict__ gu, double *__restrict__ gv) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int im = i == 0 ? nx - 1 : i - 1, jm = j == 0 ? ny - 1 : j - 1;
    if (gu) gu[c] = (p[c] - p[(long)j * nx + im]) / dx;
    if (gv) gv[c] = (p[c] - p[(long)jm * nx + i]) / dy;
}

// the predictor (explicit or the IMEX right-hand side) at every face
__global__ void k_macp_predict(const double *__restrict__ u, const double *__restrict__ v, int ny,
                               int nx, MacpCoef k, int imex, double *__restrict__ us,
                               double *__restrict__ vs) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int ip = i + 1 == nx ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
    const long r = (long)j * nx, rp = (long)(j + 1 == ny ? 0 : j + 1) * nx,
               rm = (long)(j == 0 ? ny - 1 : j - 1) * nx;
    us[c] = macp_ustar(u[c], u[r + ip], u[r + im], u[rp + i], u[rm + i], v[c], v[r + im],
                       v[rp + i], v[rp + im], k, imex);
    vs[c] = macp_vstar(v[c], v[r + ip], v[r + im], v[rp + i], v[rm + i], u[c], u[r + ip],
                       u[rm + i], u[rm + ip], k, imex);
}

// The explicit predictor and project_per's right-hand side in one pass.  A workgroup owns a
// MACP_TX x MACP_TY tile of cells and holds the periodic window of u and v around it in LDS
// (one cell west / south, two east / north, loaded through wrapped indices, so a partial
// tile and an extent below the tile see the same neighbours as any other cell).  u* is
// computed on the tile plus one column east and v* on the tile plus one row north, by the
// same device functions as k_macp_predict (the same bits), then the tile's u*, v* and
// s * div(u*, v*) are written.
constexpr int MACP_TX = 64, MACP_TY = 16, MACP_WX = MACP_TX + 3, MACP_WY = MACP_TY + 3;
constexpr int MACP_THREADS = 256;

__global__ __launch_bounds__(MACP_THREADS) void k_macp_predict_div(
    const double *__restrict__ u, const double *__restrict__ v, int ny, int nx, MacpCoef k,
    double dx, double dy, double s, double *__restrict__ us, double *__restrict__ vs,
    double *__restrict__ rhs) {
    __shared__ double su[MACP_WY][MACP_WX], sv[MACP_WY][MACP_WX];
    __shared__ double tu[MACP_TY][MACP_TX + 1], tv[MACP_TY + 1][MACP_TX];
    const int i0 = blockIdx.x * MACP_TX, j0 = blockIdx.y * MACP_TY, t = threadIdx.x;
    for (int q = t; q < MACP_WY * MACP_WX; q += MACP_THREADS) {
        const int lj = q / MACP_WX, li = q % MACP_WX;
        const long g = (long)macp_wrap(j0 - 1 + lj, ny) * nx + macp_wrap(i0 - 1 + li, nx);
        su[lj][li] = u[g];
        sv[lj][li] = v[g];
    }
    __syncthreads();
    // tile cell (lj, li) is window cell (lj + 1, li + 1)
    for (int q = t; q < MACP_TY * (MACP_TX + 1); q += MACP_THREADS) {
        const int lj = q / (MACP_TX + 1), li = q % (MACP_TX + 1), a = lj + 1, b = li + 1;
        tu[lj][li] = macp_ustar(su[a][b], su[a][b + 1], su[a][b - 1], su[a + 1][b], su[a - 1][b],
                                sv[a][b], sv[a][b - 1], sv[a + 1][b], sv[a + 1][b - 1], k, 0);
    }
    for (int q = t; q < (MACP_TY + 1) * MACP_TX; q += MACP_THREADS) {
        const int lj = q / MACP_TX, li = q % MACP_TX, a = lj + 1, b = li + 1;
        tv[lj][li] = macp_vstar(sv[a][b], sv[a][b + 1], sv[a][b - 1], sv[a + 1][b], sv[a - 1][b],
                                su[a][b], su[a][b + 1], su[a - 1][b], su[a - 1][b + 1], k, 0);
    }
    __syncthreads();
    for (int q = t; q < MACP_TY * MACP_TX; q += MACP_THREADS) {
        const int lj = q / MACP_TX, li = q % MACP_TX, gj = j0 + lj, gi = i0 + li;
        if (gj >= ny || gi >= nx) continue;
        const long c = (long)gj * nx + gi;
        const double uc = tu[lj][li], vc = tv[lj][li];
        us[c] = uc;
        vs[c] = vc;
        rhs[c] = s * ((tu[lj][li + 1] - uc) / dx + (tv[lj + 1][li] - vc) / dy);
    }
}

// xhat = rhat / symbol, symbol = lx[i] + ly[j] rebuilt per element (one rounded add, as the
// reference's broadcast); mode 0: Poisson, (0,0) zeroed (mac.py:472); mode 1: Helmholtz,
// 1 - coef * symbol (mac.py:517).  scale: the inverse transform's 1 / (ny nx).
__global__ void k_macp_symbol(double2 *__restrict__ C, int ny, int h,
                              const double *__restrict__ lx, const double *__restrict__ ly,
                              int mode, double coef, double scale) {
    const long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (q >= (long)ny * h) return;
    const int j = (int)(q / h), i = (int)(q % h);
    const double e = lx[i] + ly[j];
    const double d = mode ? 1.0 - coef * e : e;
    const double2 z = C[q];
    C[q] = (!mode && q == 0) ? make_double2(0.0, 0.0)
                             : make_double2(z.x / d * scale, z.y / d * scale);
}

// mac.py:479-480: u* - (dt / rho) * grad(phi)
__global__ void k_macp_correct(const double *__restrict__ phi, const double *__restrict__ us,
                               const double *__restrict__ vs, int ny, int nx, double dx,
                               double dy, double dt_rho, double *__restrict__ u,
                               double *__restrict__ v) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int im = i == 0 ? nx - 1 : i - 1, jm = j == 0 ? ny - 1 : j - 1;
    const double pc = phi[c];
    u[c] = us[c] - dt_rho * ((pc - phi[(long)j * nx + im]) / dx);
    v[c] = vs[c] - dt_rho * ((pc - phi[(long)jm * nx + i]) / dy);
}

// in -> out (may be the same plane) through the context's half-spectrum workspace
int macp_solve(rmt_ctx *ctx, const double *in, int mode, double coef, double *out) {
    MacPerPlan *P = ctx->macper;
    const int ny = P->ny, nx = P->nx, h = nx / 2 + 1;
    hipStream_t st = ctx->stream;
    double *C = ctx->scratch;
    RMT_TRY(P->fft.on(st));
    void *i1[1] = {(void *)in}, *o1[1] = {C};
    RMT_TRY(rocfft_ok(rocfft_execute(P->fft.plan[0], i1, o1, P->fft.info),
                      "periodic MAC execute fwd"));
    k_macp_symbol<<<grid1d((long)ny * h, 256), 256, 0, st>>>((double2 *)C, ny, h, P->lx, P->ly,
                                                             mode, coef,
                                                             1.0 / ((double)ny * (double)nx));
    RMT_LAUNCHED();
    void *i2[1] = {C}, *o2[1] = {out};
    return rocfft_ok(rocfft_execute(P->fft.plan[1], i2, o2, P->fft.info),
                     "periodic MAC execute inv");
}

static int macp_predict(rmt_ctx *ctx, const double *u, const double *v, const MacpCoef &k,
                        int imex, double *us, double *vs) {
    const long n = (long)ctx->ny * ctx->nx;
    k_macp_predict<<<grid1d(n, 256), 256, 0, ctx->stream>>>(u, v, ctx->ny, ctx->nx, k, imex, us,
                                                            vs);
    RMT_LAUNCHED();
    return RMT_OK;
}

// mac.py:538-539 after the explicit advection: two Helmholtz solves, in place
static int macp_imex_predict(rmt_ctx *ctx, const double *u, const double *v, const MacpCoef &k,
                             double coef, double *us, double *vs) {
    RMT_TRY(macp_predict(ctx, u, v, k, 1, us, vs));
    RMT_TRY(macp_solve(ctx, us, 1, coef, us));
    return macp_solve(ctx, vs, 1, coef, vs);
}

// mac.py:476-480 from the scaled divergence in phi: solve in place, correct
int macp_project_rhs(rmt_ctx *ctx, const double *us, const double *vs, double dx, double dy,
                     double dt_rho, double *u, double *v, double *phi) {
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(macp_solve(ctx, phi, 0, 0.0, phi));
    k_macp_correct<<<grid1d(n, 256), 256, 0, ctx->stream>>>(phi, us, vs, ctx->ny, ctx->nx, dx, dy,
                                                            dt_rho, u, v);
    RMT_LAUNCHED();
    return RMT_OK;
}

int macp_div(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy, double s,
             double *out) {
    const long n = (long)ctx->ny * ctx->nx;
    k_macp_div<<<grid1d(n, 256), 256, 0, ctx->stream>>>(u, v, ctx->ny, ctx->nx, dx, dy, s, out);
    RMT_LAUNCHED();
    return RMT_OK;
}

}  // namespace rmt

using namespace rmt;

extern "C" {

int rmt_mac_per_divergence(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy,
                           double *out) {
    RMT_CHECK(ctx && u && v && out, RMT_EINVAL, "bad argument");
    return macp_div(ctx, u, v, dx, dy, 1.0, out);
}

int rmt_mac_per_gradient_p(rmt_ctx *ctx, const double *p, double dx, double dy, double *gu,
                           double *gv) {
    RMT_CHECK(ctx && p && (gu || gv), RMT_EINVAL, "bad argument");
    const long n = (long)ctx->ny * ctx->nx;
    k_macp_grad<<<grid1d(n, 256), 256, 0, ctx->stream>>>(p, ctx->ny, ctx->nx, dx, dy, gu, gv);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_per_predictor(rmt_ctx *ctx, const double *u, const double *v, double nu, double dx2,
                          double dy2, double twodx, double twody, double dt, double *u_star,
                          double *v_star) {
    RMT_CHECK(ctx && u && v && u_star && v_star, RMT_EINVAL, "bad argument");
    RMT_CHECK(u_star != u && u_star != v && v_star != u && v_star != v, RMT_EINVAL,
              "periodic MAC predictor: not in place");
    return macp_predict(ctx, u, v, MacpCoef{nu, dx2, dy2, twodx, twody, dt}, 0, u_star, v_star);
}

int rmt_mac_per_predictor_imex(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                               double twody, double dt, double coef, const double *lx,
                               const double *ly, double *u_star, double *v_star) {
    RMT_CHECK(ctx && u && v && lx && ly && u_star && v_star, RMT_EINVAL, "bad argument");
    RMT_CHECK(u_star != u && u_star != v && v_star != u && v_star != v, RMT_EINVAL,
              "periodic MAC predictor: not in place");
    RMT_TRY(macp_workspace(ctx, 0));
    RMT_TRY(macp_plan(ctx, lx, ly));
    return macp_imex_predict(ctx, u, v, MacpCoef{0.0, 1.0, 1.0, twodx, twody, dt}, coef, u_star,
                             v_star);
}

int rmt_mac_per_solve(rmt_ctx *ctx, const double *rhs, int mode, double coef, const double *lx,
                      const double *ly, double *out) {
    RMT_CHECK(ctx && rhs && lx && ly && out && (mode == 0 || mode == 1), RMT_EINVAL,
              "bad argument");
    RMT_TRY(macp_workspace(ctx, 0));
    RMT_TRY(macp_plan(ctx, lx, ly));
    return macp_solve(ctx, rhs, mode, coef, out);
}

int rmt_mac_per_project(rmt_ctx *ctx, const double *u_star, const double *v_star, double dx,
                        double dy, double rho_dt, double dt_rho, const double *lx,
                        const double *ly, double *u, double *v, double *phi) {
    RMT_CHECK(ctx && u_star && v_star && lx && ly && u && v && phi, RMT_EINVAL, "bad argument");
    RMT_TRY(macp_workspace(ctx, 0));
    RMT_TRY(macp_plan(ctx, lx, ly));
    RMT_TRY(macp_div(ctx, u_star, v_star, dx, dy, rho_dt, phi));
    return macp_project_rhs(ctx, u_star, v_star, dx, dy, dt_rho, u, v, phi);
}

int rmt_mac_per_steps(rmt_ctx *ctx, double *u, double *v, double nu, double dx, double dy,
                      double dx2, double dy2, double twodx, double twody, double dt, double coef,
                      double rho_dt, double dt_rho, const double *lx, const double *ly, int imex,
                      int nsteps, double *p) {
    RMT_CHECK(ctx && u && v && u != v && lx && ly && nsteps >= 0, RMT_EINVAL, "bad argument");
    RMT_TRY(macp_workspace(ctx, 3));
    RMT_TRY(macp_plan(ctx, lx, ly));
    const int ny = ctx->ny, nx = ctx->nx;
    const long n = (long)ny * nx;
    double *us = ctx->scratch + macp_spec(ctx), *vs = us + macp_plane(ctx),
           *phi = vs + macp_plane(ctx);
    const MacpCoef k{nu, dx2, dy2, twodx, twody, dt};
    const dim3 tiles((nx + MACP_TX - 1) / MACP_TX, (ny + MACP_TY - 1) / MACP_TY);
    for (int s = 0; s < nsteps; ++s) {
        if (imex) {
            RMT_TRY(macp_imex_predict(ctx, u, v, k, coef, us, vs));
            RMT_TRY(macp_div(ctx, us, vs, dx, dy, rho_dt, phi));
        } else if (ctx->opt.macp_fused) {
            k_macp_predict_div<<<tiles, MACP_THREADS, 0, ctx->stream>>>(u, v, ny, nx, k, dx, dy,
                                                                        rho_dt, us, vs, phi);
            RMT_LAUNCHED();
        } else {
            RMT_TRY(macp_predict(ctx, u, v, k, 0, us, vs));
            RMT_TRY(macp_div(ctx, us, vs, dx, dy, rho_dt, phi));
        }
        RMT_TRY(macp_project_rhs(ctx, us, vs, dx, dy, dt_rho, u, v, phi));
    }
    if (p && nsteps > 0)
        RMT_HIP(hipMemcpyAsync(p, phi, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    return RMT_OK;
}

}  // extern "C"
