// macper_sl.hip -- mac.py:587-633, the semi-Lagrangian predictor of the periodic staggered
// (MAC) tier: _interp_per (scipy.ndimage.map_coordinates, order 3, mode "grid-wrap"),
// _sl_advect_per, momentum_predictor_periodic_semilag, and the "imex-sl" loop of
// benchmarks/mac_taylor_green_convergence.py:59-66 with the CFL switch decided on the device.
//
// The cubic B-spline prefilter of a periodic line s[0 .. n-1] (pole z = sqrt(3) - 2, gain
// (1 - z)(1 - 1/z)) is scipy's causal + anticausal recursion pair; the pair composed is the
// two-sided sum
//     c[i] = sqrt(3) * sum_d z^|d| s[(i + d) mod n]
//          = sqrt(3) * (cp[i] + z * cm[i + 1]),  cp[i] = sum_{k>=0} z^k s[i - k],
//                                                cm[i] = sum_{k>=0} z^k s[i + k]
// (gain * (-z) / (1 - z^2) = (1 - z) / (1 + z) = sqrt(3)).  Both one-sided sums are cut at
// SPL_K = 48 terms, indices wrapping as often as needed: |z|^48 / (1 - |z|) = 4.8e-28 of
// scale is left out.  Any stretch of a line therefore starts both recursions from a
// 47 / 48-sample warm-up, independently of every other stretch, and the result equals the
// serial recursions to rounding (not bit for bit; nothing behind this tier's FFT pair is).
//
// A workgroup takes SPL_W lines x SPL_L samples: it loads the samples and their warm-up
// margins into LDS through wrapped indices (coalesced in both passes: along the lines in the
// axis-0 pass, along the samples in the axis-1 pass), then each thread runs the two
// recursions over SPL_CH samples of one line out of LDS, and the block writes coalesced.
// Extents below the window, below a chunk, odd and rectangular go through the same code.
#include "macper.hpp"

namespace rmt {

constexpr int SPL_K = 48;                    // terms kept of each one-sided sum
constexpr int SPL_CH = 16;                   // samples per thread
constexpr int SPL_G = 8;                     // threads along a line
constexpr int SPL_L = SPL_CH * SPL_G;        // samples of a line per workgroup (128)
constexpr int SPL_W = 32;                    // lines per workgroup
constexpr int SPL_T = SPL_L + 2 * SPL_K - 1; // tile length: 47 before, 48 after (223, odd:
                                             // lanes on consecutive lines hit distinct banks)
constexpr int SPL_THREADS = SPL_W * SPL_G;   // 256
constexpr double SPL_Z = -0.26794919243112270647;   // sqrt(3) - 2
constexpr double SPL_S3 = 1.73205080756887729353;   // sqrt(3)

// the device words of the CFL switch, behind the planes of the workspace (macper.hpp: tail)
constexpr int SLR_BLOCKS = 512;              // partial maxima per field
constexpr size_t SL_TAIL = 2 * SLR_BLOCKS + 2;
struct SlWords { double *part; int *flag, *count; };
static inline SlWords sl_words(double *tail) {
    int *w = (int *)(tail + 2 * SLR_BLOCKS);
    return SlWords{tail, w, w + 1};
}

// AXIS 0: the lines are the columns (length ny, nx of them); AXIS 1: the rows.  flag
// (nullable): the pass runs only where *flag != 0 (the loop's SL branch).  in != out.
template <int AXIS>
__global__ __launch_bounds__(SPL_THREADS) void k_macpsl_prefilter(
    const int *__restrict__ flag, const double *__restrict__ in, int ny, int nx,
    double *__restrict__ out) {
    __shared__ double sh[SPL_W * SPL_T];
    if (flag && !*flag) return;
    const int n = AXIS == 0 ? ny : nx, m = AXIS == 0 ? nx : ny;
    const int l0 = (AXIS == 0 ? blockIdx.x : blockIdx.y) * SPL_W;
    const int p0 = (AXIS == 0 ? blockIdx.y : blockIdx.x) * SPL_L;
    const int t = threadIdx.x;
    const int first = macp_wrap(p0 - (SPL_K - 1), n);
    for (int q = t; q < SPL_W * SPL_T; q += SPL_THREADS) {
        const int line = AXIS == 0 ? q % SPL_W : q / SPL_T;
        const int pos = AXIS == 0 ? q / SPL_W : q % SPL_T;
        int g = first + pos;
        if (g >= n) {
            g -= n;
            if (g >= n) g %= n;
        }
        const int ll = l0 + line;
        double val = 0.0;
        if (ll < m) val = in[AXIS == 0 ? (long)g * nx + ll : (long)ll * nx + g];
        sh[line * SPL_T + pos] = val;
    }
    __syncthreads();
    const int line = t % SPL_W, grp = t / SPL_W;
    const double *ln = sh + line * SPL_T + (SPL_K - 1) + grp * SPL_CH;   // the thread's sample 0
    const bool live = p0 + grp * SPL_CH < n && l0 + line < m;
    double o[SPL_CH];
    if (live) {
        // warm-ups: cp over samples -47 .. -1, cm over samples 63 .. 16 (two independent chains)
        double cp = 0.0, cm = ln[SPL_CH + SPL_K - 1];
#pragma unroll
        for (int w = 0; w < SPL_K - 1; ++w) {
            cp = ln[w - (SPL_K - 1)] + SPL_Z * cp;
            cm = ln[SPL_CH + SPL_K - 2 - w] + SPL_Z * cm;
        }
#pragma unroll
        for (int k = 0; k < SPL_CH; ++k) {
            cp = ln[k] + SPL_Z * cp;
            o[k] = cp;
        }
#pragma unroll
        for (int k = SPL_CH - 1; k >= 0; --k) {
            o[k] = SPL_S3 * (o[k] + SPL_Z * cm);
            cm = ln[k] + SPL_Z * cm;
        }
    }
    if (AXIS == 0) {
        if (!live) return;
#pragma unroll
        for (int k = 0; k < SPL_CH; ++k) {
            const int j = p0 + grp * SPL_CH + k;
            if (j < n) out[(long)j * nx + l0 + line] = o[k];
        }
    } else {
        // through LDS (samples 0 .. SPL_L of each line's tile), so that the rows go out whole
        __syncthreads();
        if (live) {
#pragma unroll
            for (int k = 0; k < SPL_CH; ++k) sh[line * SPL_T + grp * SPL_CH + k] = o[k];
        }
        __syncthreads();
        for (int q = t; q < SPL_W * SPL_L; q += SPL_THREADS) {
            const int r = l0 + q / SPL_L, i = p0 + q % SPL_L;
            if (r < m && i < n) out[(long)r * nx + i] = sh[(q / SPL_L) * SPL_T + q % SPL_L];
        }
    }
}

// The divisors of an evaluation (6, ny, nx) and of a backtrace (dx, dy), made on the host:
// every division below is divk (divk.hpp), the bits of the IEEE quotient in 3 fma-class
// instructions -- an evaluation divides eight times and a face makes ten evaluations.
struct SplK { DivK k6, kny, knx; };
struct SlK { SplK s; DivK kdx, kdy; };
static inline SplK spl_k(const rmt_ctx *ctx) {
    return SplK{divk_make(6.0), divk_make((double)ctx->ny), divk_make((double)ctx->nx)};
}
static inline SlK sl_k(const rmt_ctx *ctx, double dx, double dy) {
    return SlK{spl_k(ctx), divk_make(dx), divk_make(dy)};
}

// one axis of map_coordinates(order=3, mode="grid-wrap") at coordinate q on extent n: the
// four weights and the wrapped taps f-1 .. f+2.  The reduced coordinate can round to n
// itself, so every tap wraps by an integer modulo; the base index is clamped before the
// conversion, so no coordinate (NaN, infinite) indexes outside the plane.
__device__ __forceinline__ void spl_axis(double q, int n, const DivK &Kn, const DivK &K6,
                                         double w[4], int tap[4]) {
    const double r = q - (double)n * floor(divk(q, Kn));
    const double f = floor(r), y = r - f, t = 1.0 - y;
    w[0] = divk(t * t * t, K6);
    w[1] = divk(y * y * (y - 2.0) * 3.0 + 4.0, K6);
    w[2] = divk(t * t * (t - 2.0) * 3.0 + 4.0, K6);
    w[3] = 1.0 - w[0] - w[1] - w[2];
    const int b = (int)fmin(fmax(f, 0.0), (double)n) - 1;   // -1 .. n - 1
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int i = b + a;                                      // -1 .. n + 2, n >= 2
        if (i < 0) i += n;
        if (i >= n) i -= n;
        if (i >= n) i -= n;
        tap[a] = i;
    }
}

// mac.py:593-598 (_interp_per) on the coefficient plane c at (jq, iq): sum_a sum_b
// (c[ja, ib] * wj[a]) * wi[b], a outer, b inner
__device__ __forceinline__ double spl_per(const double *__restrict__ c, int ny, int nx,
                                          const SplK &K, double jq, double iq) {
    double wj[4], wi[4];
    int tj[4], ti[4];
    spl_axis(jq, ny, K.kny, K.k6, wj, tj);
    spl_axis(iq, nx, K.knx, K.k6, wi, ti);
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double *row = c + (long)tj[a] * nx;
#pragma unroll
        for (int b = 0; b < 4; ++b) s += (row[ti[b]] * wj[a]) * wi[b];
    }
    return s;
}

// mac.py:601-614 (_sl_advect_per) at point (j, i) of a field at offset (ox, oy): cf, cu, cv
// are the coefficient planes of the field and of the two face velocities
__device__ __forceinline__ double sl_advect_pt(const double *__restrict__ cf,
                                               const double *__restrict__ cu,
                                               const double *__restrict__ cv, int ny, int nx,
                                               int j, int i, double ox, double oy, double dx,
                                               double dy, double dt, const SlK &K) {
    const double xf = ((double)i + ox) * dx, yf = ((double)j + oy) * dy;
    const double xi = divk(xf, K.kdx), yj = divk(yf, K.kdy);
    const double velx = spl_per(cu, ny, nx, K.s, yj - 0.5, xi);
    const double vely = spl_per(cv, ny, nx, K.s, yj, xi - 0.5);
    const double xm = xf - 0.5 * dt * velx, ym = yf - 0.5 * dt * vely;
    const double xmi = divk(xm, K.kdx), ymj = divk(ym, K.kdy);
    const double vxm = spl_per(cu, ny, nx, K.s, ymj - 0.5, xmi);
    const double vym = spl_per(cv, ny, nx, K.s, ymj, xmi - 0.5);
    const double xd = xf - dt * vxm, yd = yf - dt * vym;
    return spl_per(cf, ny, nx, K.s, divk(yd, K.kdy) - oy, divk(xd, K.kdx) - ox);
}

__global__ void k_macpsl_interp(const double *__restrict__ c, int ny, int nx,
                                const double *__restrict__ iq, const double *__restrict__ jq,
                                long nq, SplK K, double *__restrict__ out) {
    const long k = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (k < nq) out[k] = spl_per(c, ny, nx, K, jq[k], iq[k]);
}

constexpr int SLA_X = 64, SLA_Y = 4;   // cells of a workgroup of the advection kernels

__global__ __launch_bounds__(SLA_X *SLA_Y) void k_macpsl_advect(
    const double *__restrict__ cf, const double *__restrict__ cu, const double *__restrict__ cv,
    int ny, int nx, double ox, double oy, double dx, double dy, double dt, SlK K,
    double *__restrict__ out) {
    const int i = blockIdx.x * SLA_X + threadIdx.x, j = blockIdx.y * SLA_Y + threadIdx.y;
    if (i >= nx || j >= ny) return;
    out[(long)j * nx + i] = sl_advect_pt(cf, cu, cv, ny, nx, j, i, ox, oy, dx, dy, dt, K);
}

// mac.py:628-629 at every face: u (offset (0, 1/2)) and v ((1/2, 0)) advected by (u, v).
// flag (nullable): runs only where *flag != 0
__global__ __launch_bounds__(SLA_X *SLA_Y) void k_macpsl_advect_uv(
    const int *__restrict__ flag, const double *__restrict__ cu, const double *__restrict__ cv,
    int ny, int nx, double dx, double dy, double dt, SlK K, double *__restrict__ us,
    double *__restrict__ vs) {
    if (flag && !*flag) return;
    const int i = blockIdx.x * SLA_X + threadIdx.x, j = blockIdx.y * SLA_Y + threadIdx.y;
    if (i >= nx || j >= ny) return;
    const long c = (long)j * nx + i;
    us[c] = sl_advect_pt(cu, cu, cv, ny, nx, j, i, 0.0, 0.5, dx, dy, dt, K);
    vs[c] = sl_advect_pt(cv, cu, cv, ny, nx, j, i, 0.5, 0.0, dx, dy, dt, K);
}

// k_macp_predict's IMEX right-hand side (the same device functions, the same bits) where
// *flag == 0: the loop's central branch
__global__ void k_macpsl_central(const int *__restrict__ flag, const double *__restrict__ u,
                                 const double *__restrict__ v, int ny, int nx, MacpCoef k,
                                 double *__restrict__ us, double *__restrict__ vs) {
    if (*flag) return;
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int ip = i + 1 == nx ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
    const long r = (long)j * nx, rp = (long)(j + 1 == ny ? 0 : j + 1) * nx,
               rm = (long)(j == 0 ? ny - 1 : j - 1) * nx;
    us[c] = macp_ustar(u[c], u[r + ip], u[r + im], u[rp + i], u[rm + i], v[c], v[r + im],
                       v[rp + i], v[rp + im], k, 1);
    vs[c] = macp_vstar(v[c], v[r + ip], v[r + im], v[rp + i], v[rm + i], u[c], u[r + ip],
                       u[rm + i], u[rm + ip], k, 1);
}

// np.max(np.abs(u)), np.max(np.abs(v)) (a NaN propagates), per workgroup: part[b],
// part[SLR_BLOCKS + b]
__global__ __launch_bounds__(256) void k_macpsl_absmax(const double *__restrict__ u,
                                                       const double *__restrict__ v, long n,
                                                       double *__restrict__ part) {
    __shared__ double su[256], sv[256];
    double mu = 0.0, mv = 0.0;
    for (long c = blockIdx.x * 256L + threadIdx.x; c < n; c += gridDim.x * 256L) {
        mu = nanmax(mu, fabs(u[c]));
        mv = nanmax(mv, fabs(v[c]));
    }
    su[threadIdx.x] = mu; sv[threadIdx.x] = mv;
    __syncthreads();
    tree_fold<256>([&](int t, int w) {
        su[t] = nanmax(su[t], su[w]);
        sv[t] = nanmax(sv[t], sv[w]);
    });
    if (threadIdx.x == 0) {
        part[blockIdx.x] = su[0];
        part[SLR_BLOCKS + blockIdx.x] = sv[0];
    }
}

// mac.py:625-626: cfl = dt * max(max|u| / dx, max|v| / dy) with Python's max (the second
// operand only where it compares greater, so a NaN there is dropped and a NaN in the first
// stays); cfl <= cfl_switch: the central branch (flag 0), else SL (flag 1, one more SL step)
__global__ __launch_bounds__(256) void k_macpsl_decide(const double *__restrict__ part, int nb,
                                                       double dx, double dy, double dt,
                                                       double cfl_switch, int *__restrict__ flag,
                                                       int *__restrict__ count) {
    __shared__ double su[256], sv[256];
    double mu = 0.0, mv = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) {
        mu = nanmax(mu, part[b]);
        mv = nanmax(mv, part[SLR_BLOCKS + b]);
    }
    su[threadIdx.x] = mu; sv[threadIdx.x] = mv;
    __syncthreads();
    tree_fold<256>([&](int t, int w) {
        su[t] = nanmax(su[t], su[w]);
        sv[t] = nanmax(sv[t], sv[w]);
    });
    if (threadIdx.x == 0) {
        const double a = su[0] / dx, b = sv[0] / dy;
        const double cfl = dt * (b > a ? b : a);
        const int sl = cfl <= cfl_switch ? 0 : 1;
        *flag = sl;
        if (sl) *count += 1;
    }
}

// f -> out through tmp (three distinct planes, or out == f), axis 0 then axis 1
static int sl_prefilter(rmt_ctx *ctx, const int *flag, const double *f, double *tmp,
                        double *out) {
    const int ny = ctx->ny, nx = ctx->nx;
    const dim3 g0((nx + SPL_W - 1) / SPL_W, (ny + SPL_L - 1) / SPL_L);
    const dim3 g1((nx + SPL_L - 1) / SPL_L, (ny + SPL_W - 1) / SPL_W);
    k_macpsl_prefilter<0><<<g0, SPL_THREADS, 0, ctx->stream>>>(flag, f, ny, nx, tmp);
    RMT_LAUNCHED();
    k_macpsl_prefilter<1><<<g1, SPL_THREADS, 0, ctx->stream>>>(flag, tmp, ny, nx, out);
    RMT_LAUNCHED();
    return RMT_OK;
}

static inline dim3 sla_grid(const rmt_ctx *ctx) {
    return dim3((ctx->nx + SLA_X - 1) / SLA_X, (ctx->ny + SLA_Y - 1) / SLA_Y);
}

// the switch of one step: the device flag and (SL) the counter
static int sl_decide(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy,
                     double dt, double cfl_switch, const SlWords &W) {
    const long n = (long)ctx->ny * ctx->nx;
    const int nb = (int)std::min<long>(SLR_BLOCKS, grid1d(n, 256));
    k_macpsl_absmax<<<nb, 256, 0, ctx->stream>>>(u, v, n, W.part);
    RMT_LAUNCHED();
    k_macpsl_decide<<<1, 256, 0, ctx->stream>>>(W.part, nb, dx, dy, dt, cfl_switch, W.flag,
                                                W.count);
    RMT_LAUNCHED();
    return RMT_OK;
}

// mac.py:625-633 into us, vs with both branches launched and the one not taken exiting on
// the flag; cu, cv: two more planes (us, vs serve the prefilter's first pass)
static int sl_predict(rmt_ctx *ctx, const double *u, const double *v, const MacpCoef &k,
                      double dx, double dy, double coef, double cfl_switch, const SlWords &W,
                      double *cu, double *cv, double *us, double *vs) {
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(sl_decide(ctx, u, v, dx, dy, k.dt, cfl_switch, W));
    k_macpsl_central<<<grid1d(n, 256), 256, 0, ctx->stream>>>(W.flag, u, v, ctx->ny, ctx->nx, k,
                                                              us, vs);
    RMT_LAUNCHED();
    RMT_TRY(sl_prefilter(ctx, W.flag, u, us, cu));
    RMT_TRY(sl_prefilter(ctx, W.flag, v, vs, cv));
    k_macpsl_advect_uv<<<sla_grid(ctx), dim3(SLA_X, SLA_Y), 0, ctx->stream>>>(
        W.flag, cu, cv, ctx->ny, ctx->nx, dx, dy, k.dt, sl_k(ctx, dx, dy), us, vs);
    RMT_LAUNCHED();
    RMT_TRY(macp_solve(ctx, us, 1, coef, us));
    return macp_solve(ctx, vs, 1, coef, vs);
}

static int sl_read_int(rmt_ctx *ctx, const int *dev, int *host) {
    RMT_HIP(hipMemcpyAsync(host, dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    return RMT_OK;
}

}  // namespace rmt

using namespace rmt;

extern "C" {

int rmt_mac_per_spline_prefilter(rmt_ctx *ctx, const double *f, double *out) {
    RMT_CHECK(ctx && f && out, RMT_EINVAL, "bad argument");
    RMT_CHECK(ctx->ny >= 2 && ctx->nx >= 2, RMT_EINVAL, "periodic spline: ny, nx >= 2");
    RMT_TRY(macp_workspace(ctx, 1));
    return sl_prefilter(ctx, nullptr, f, ctx->scratch + macp_spec(ctx), out);
}

int rmt_mac_per_interp(rmt_ctx *ctx, const double *f, const double *iq, const double *jq,
                       int nq, double *out) {
    RMT_CHECK(ctx && f && nq >= 0 && (nq == 0 || (iq && jq && out)), RMT_EINVAL, "bad argument");
    RMT_CHECK(ctx->ny >= 2 && ctx->nx >= 2, RMT_EINVAL, "periodic spline: ny, nx >= 2");
    if (nq == 0) return RMT_OK;
    RMT_TRY(macp_workspace(ctx, 2));
    double *tmp = ctx->scratch + macp_spec(ctx), *c = tmp + macp_plane(ctx);
    RMT_TRY(sl_prefilter(ctx, nullptr, f, tmp, c));
    k_macpsl_interp<<<grid1d(nq, 256), 256, 0, ctx->stream>>>(c, ctx->ny, ctx->nx, iq, jq, nq,
                                                             spl_k(ctx), out);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_per_sl_advect(rmt_ctx *ctx, const double *f, const double *uf, const double *vf,
                          double ox, double oy, double dx, double dy, double dt, double *out) {
    RMT_CHECK(ctx && f && uf && vf && out, RMT_EINVAL, "bad argument");
    RMT_CHECK(ctx->ny >= 2 && ctx->nx >= 2, RMT_EINVAL, "periodic spline: ny, nx >= 2");
    RMT_TRY(macp_workspace(ctx, 4));
    double *tmp = ctx->scratch + macp_spec(ctx), *cf = tmp + macp_plane(ctx),
           *cu = cf + macp_plane(ctx), *cv = cu + macp_plane(ctx);
    RMT_TRY(sl_prefilter(ctx, nullptr, f, tmp, cf));
    RMT_TRY(sl_prefilter(ctx, nullptr, uf, tmp, cu));
    RMT_TRY(sl_prefilter(ctx, nullptr, vf, tmp, cv));
    k_macpsl_advect<<<sla_grid(ctx), dim3(SLA_X, SLA_Y), 0, ctx->stream>>>(
        cf, cu, cv, ctx->ny, ctx->nx, ox, oy, dx, dy, dt, sl_k(ctx, dx, dy), out);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_per_predictor_semilag(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                                  double twody, double dx, double dy, double dt, double coef,
                                  double cfl_switch, const double *lx, const double *ly,
                                  double *u_star, double *v_star, int *took_sl) {
    RMT_CHECK(ctx && u && v && lx && ly && u_star && v_star, RMT_EINVAL, "bad argument");
    RMT_CHECK(u_star != u && u_star != v && v_star != u && v_star != v && u_star != v_star,
              RMT_EINVAL, "periodic MAC predictor: not in place");
    RMT_TRY(macp_workspace(ctx, 2, SL_TAIL));
    RMT_TRY(macp_plan(ctx, lx, ly));
    double *cu = ctx->scratch + macp_spec(ctx), *cv = cu + macp_plane(ctx);
    const SlWords W = sl_words(cv + macp_plane(ctx));
    RMT_HIP(hipMemsetAsync(W.flag, 0, 2 * sizeof(int), ctx->stream));
    RMT_TRY(sl_predict(ctx, u, v, MacpCoef{0.0, 1.0, 1.0, twodx, twody, dt}, dx, dy, coef,
                       cfl_switch, W, cu, cv, u_star, v_star));
    if (took_sl) RMT_TRY(sl_read_int(ctx, W.flag, took_sl));
    return RMT_OK;
}

int rmt_mac_per_steps_sl(rmt_ctx *ctx, double *u, double *v, double nu, double dx, double dy,
                         double dx2, double dy2, double twodx, double twody, double dt,
                         double coef, double rho_dt, double dt_rho, const double *lx,
                         const double *ly, double cfl_switch, int nsteps, double *p,
                         int *sl_steps) {
    RMT_CHECK(ctx && u && v && u != v && lx && ly && nsteps >= 0, RMT_EINVAL, "bad argument");
    RMT_TRY(macp_workspace(ctx, 5, SL_TAIL));
    RMT_TRY(macp_plan(ctx, lx, ly));
    const long n = (long)ctx->ny * ctx->nx;
    const size_t pl = macp_plane(ctx);
    double *us = ctx->scratch + macp_spec(ctx), *vs = us + pl, *phi = vs + pl, *cu = phi + pl,
           *cv = cu + pl;
    const SlWords W = sl_words(cv + pl);
    const MacpCoef k{nu, dx2, dy2, twodx, twody, dt};
    RMT_HIP(hipMemsetAsync(W.flag, 0, 2 * sizeof(int), ctx->stream));
    for (int s = 0; s < nsteps; ++s) {
        RMT_TRY(sl_predict(ctx, u, v, k, dx, dy, coef, cfl_switch, W, cu, cv, us, vs));
        RMT_TRY(macp_div(ctx, us, vs, dx, dy, rho_dt, phi));
        RMT_TRY(macp_project_rhs(ctx, us, vs, dx, dy, dt_rho, u, v, phi));
    }
    if (p && nsteps > 0)
        RMT_HIP(hipMemcpyAsync(p, phi, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (sl_steps) RMT_TRY(sl_read_int(ctx, W.count, sl_steps));
    return RMT_OK;
}

}  // extern "C"
