// momentum2.hip -- the collocated momentum path beyond one solid at gamma = 0:
//   compute_curvature            functions.py:837-861
//   compute_contact_force        functions.py:864-895
//   momentum_step_rk4, gamma > 0 functions.py:673-762 (surface tension as a body force)
//   momentum_step_rk4_2solids    functions.py:765-834
//   pressure_projection_amg with a density array constant to rounding (functions.py:1049,
//   :1331, :1352-1362)
// New code beside momentum.hip (whose tuned gamma = 0 kernels stay as they are): one LDS-tiled
// kernel per RK4 stage, templated on the number of solids, with the general edge-aware
// stencils grad2 / upwind3 of rmt_internal.hpp and plain IEEE division throughout.
#include "rmt_internal.hpp"

namespace rmt {

// Tile geometry shared by the curvature and the stage kernels (k_mom_stage's edge-tile
// layout): the outer field on the tile + 3, the field derived from it on the tile + 2.  grad2
// of the derived field reaches +-1 inside the grid and 2 cells inwards at a grid edge, which
// the + 2 halo holds even when the last tile is one cell wide; the derived field is itself a
// grad2 (one more cell) of the outer one, and upwind3 of the outer field reaches +-2.
constexpr int M2_TX = 64, M2_TY = 16, M2_T = 256;
constexpr int M2_UX = M2_TX + 6, M2_UY = M2_TY + 6;   // outer plane
constexpr int M2_GX = M2_TX + 4, M2_GY = M2_TY + 4;   // derived plane

// ------------------------------------------------------------------ curvature ----
// functions.py:837-861: n = grad(phi) / (sqrt(phi_x^2 + phi_y^2) + 1e-12), kappa = d_x n_x +
// d_y n_y, every derivative grad_central_*_2nd.  phi on the tile + 3, n on the tile + 2.
__global__ void __launch_bounds__(M2_T) k_curvature(const double *__restrict__ phi, int ny,
                                                    int nx, double dx, double dy,
                                                    double *__restrict__ kappa) {
    __shared__ double sp[M2_UY * M2_UX], snx[M2_GY * M2_GX], sny[M2_GY * M2_GX];
    const int i0 = blockIdx.x * M2_TX, j0 = blockIdx.y * M2_TY;
    const double h2x = 2 * dx, h2y = 2 * dy;
    for (int q = threadIdx.x; q < M2_UX * M2_UY; q += M2_T) {
        const int ry = q / M2_UX, rx = q % M2_UX, j = j0 - 3 + ry, i = i0 - 3 + rx;
        sp[q] = (j >= 0 && j < ny && i >= 0 && i < nx) ? phi[(long)j * nx + i] : 0.0;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < M2_GX * M2_GY; q += M2_T) {
        const int ry = q / M2_GX, rx = q % M2_GX, j = j0 - 2 + ry, i = i0 - 2 + rx;
        double a = 0.0, b = 0.0;
        if (j >= 0 && j < ny && i >= 0 && i < nx) {
            const double *f = sp + (ry + 1) * M2_UX + rx + 1;
            const double px = grad2(f, 1, i, nx, h2x), py = grad2(f, M2_UX, j, ny, h2y);
            const double mag = sqrt(px * px + py * py) + 1e-12;
            a = px / mag; b = py / mag;
        }
        snx[q] = a; sny[q] = b;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < M2_TX * M2_TY; q += M2_T) {
        const int ry = q / M2_TX, rx = q % M2_TX, j = j0 + ry, i = i0 + rx;
        if (j >= ny || i >= nx) continue;
        const int o = (ry + 2) * M2_GX + rx + 2;
        kappa[(long)j * nx + i] = grad2(snx + o, 1, i, nx, h2x) + grad2(sny + o, M2_GX, j, ny, h2y);
    }
}

// -------------------------------------------------------------- contact force ----
// grad2 on an accessor f(o) of the value o cells along the line from cell k
template <class F>
__device__ __forceinline__ double grad2f(F f, int k, int n, double h2) {
    if (k == 0) return (-3 * f(0) + 4 * f(1) - f(2)) / h2;
    if (k == n - 1) return (3 * f(0) - 4 * f(-1) + f(-2)) / h2;
    return (f(1) - f(-1)) / h2;
}

// functions.py:864-895, operand for operand; np.sign: sign(0) = 0, sign(NaN) = NaN
__global__ void k_contact_force(const double *__restrict__ phi1, const double *__restrict__ phi2,
                                int ny, int nx, double k_rep, double w_c, double dx, double dy,
                                double *__restrict__ fx, double *__restrict__ fy) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    auto p12 = [&](long cc) { return 0.5 * (phi1[cc] - phi2[cc]); };
    const double a = phi1[c], b = phi2[c], m = 0.5 * (a - b);
    const double delta = fabs(m) < w_c ? (1.0 + cos(M_PI * m / w_c)) / (2.0 * w_c) : 0.0;
    const double gx = grad2f([&](int o) { return p12(c + o); }, i, nx, 2 * dx);
    const double gy = grad2f([&](int o) { return p12(c + (long)o * nx); }, j, ny, 2 * dy);
    const double gmag = sqrt(gx * gx + gy * gy) + 1e-12;
    const double n12x = gx / gmag, n12y = gy / gmag;
    const double active = (a < 0.0 || b < 0.0) ? 1.0 : 0.0;
    const double s = m != m ? m : (m > 0.0 ? 1.0 : (m < 0.0 ? -1.0 : 0.0));
    fx[c] = k_rep * delta * s * n12x * active;
    fy[c] = k_rep * delta * s * n12y * active;
}

// functions.py:696-704: st = -gamma * kappa * grad(H)
__global__ void k_st_force(const double *__restrict__ H, const double *__restrict__ kap, int ny,
                           int nx, double gamma, double dx, double dy, double *__restrict__ fx,
                           double *__restrict__ fy) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const double g = -gamma * kap[c];
    fx[c] = g * grad2(H + c, 1, i, nx, 2 * dx);
    fy[c] = g * grad2(H + c, nx, j, ny, 2 * dy);
}

// np.minimum (o may be a)
__global__ void k_nanmin(const double *a, const double *__restrict__ b, long n, double *o) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c < n) o[c] = nanmin(a[c], b[c]);
}

// ------------------------------------------------------------------ RK4 stage ----
// The planes one stage reads besides u, v, p and the previous stage's k.  NS = 1: s[0..2] the
// elastic stress, H[0] the Heaviside, phi the level set (eta_s term on phi <= 0), f the
// surface-tension force.  NS = 2: s[0..2], H[0] of solid A and s[3..5], H[1] of solid B, f the
// contact force or null (the scalar 0.0 of k_rep <= 0).
struct M2In {
    const double *s[6];
    const double *H[2];
    const double *phi;
    const double *fx, *fy;
};

// One stage (functions.py:711-741 / :802-825): the BC'd stage velocity u + coef k_prev on the
// tile + 3, the blended stress on the tile + 2, then rhs = adv + (div sigma + f - grad p) /
// (rho + 1e-12) on the tile.  Stages 0..2 store k; stage 3 stores the pre-BC
// u + dt/6 (((k1 + 2 k2) + 2 k3) + k4).
template <int NS>
__global__ void __launch_bounds__(M2_T) k_mom2_stage(
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ p,
    const double *__restrict__ kpu, const double *__restrict__ kpv, double coef, int stage,
    int bc, double lid, M2In in, int visc, double mu_f, double eta_s, double rho_s, double rho_f,
    double dt6, double dx, double dy, int ny, int nx, const double *__restrict__ k1u,
    const double *__restrict__ k1v, const double *__restrict__ k2u,
    const double *__restrict__ k2v, double *__restrict__ ku, double *__restrict__ kv,
    double *__restrict__ outu, double *__restrict__ outv) {
    __shared__ double su[M2_UY * M2_UX], sv[M2_UY * M2_UX];
    __shared__ double gxx[M2_GY * M2_GX], gxy[M2_GY * M2_GX], gyy[M2_GY * M2_GX];
    const int i0 = blockIdx.x * M2_TX, j0 = blockIdx.y * M2_TY;
    const double h2x = 2 * dx, h2y = 2 * dy;
    // 1. stage velocity, BC applied (functions.py:714 / :803)
    for (int q = threadIdx.x; q < M2_UX * M2_UY; q += M2_T) {
        const int ry = q / M2_UX, rx = q % M2_UX, j = j0 - 3 + ry, i = i0 - 3 + rx;
        double a = 0.0, b = 0.0;
        if (j >= 0 && j < ny && i >= 0 && i < nx) {
            const BCSrc s = bc_source(bc, lid, j, i, ny, nx);
            a = s.u_const ? s.u_val
                          : (stage == 0 ? u[s.u_src] : u[s.u_src] + coef * kpu[s.u_src]);
            b = s.v_const ? s.v_val
                          : (stage == 0 ? v[s.v_src] : v[s.v_src] + coef * kpv[s.v_src]);
        }
        su[q] = a; sv[q] = b;
    }
    __syncthreads();
    // 2. blended stress; stress cell (ry, rx) is the velocity cell (ry + 1, rx + 1)
    for (int q = threadIdx.x; q < M2_GX * M2_GY; q += M2_T) {
        const int ry = q / M2_GX, rx = q % M2_GX, j = j0 - 2 + ry, i = i0 - 2 + rx;
        double xx = 0.0, xy = 0.0, yy = 0.0;
        if (j >= 0 && j < ny && i >= 0 && i < nx) {
            const long c = (long)j * nx + i;
            const double *fu = su + (ry + 1) * M2_UX + rx + 1, *fv = sv + (ry + 1) * M2_UX + rx + 1;
            const double dudx = grad2(fu, 1, i, nx, h2x), dvdy = grad2(fv, M2_UX, j, ny, h2y);
            const double dudy = grad2(fu, M2_UX, j, ny, h2y), dvdx = grad2(fv, 1, i, nx, h2x);
            const double fxx = 2 * mu_f * dudx, fyy = 2 * mu_f * dvdy, fxy = mu_f * (dudy + dvdx);
            if constexpr (NS == 1) {
                double ex = in.s[0][c], exy = in.s[1][c], ey = in.s[2][c];
                if (visc && in.phi[c] <= 0.0) {   // Kelvin-Voigt (functions.py:717-730)
                    ex = ex + eta_s * dudx;
                    ey = ey + eta_s * dvdy;
                    exy = exy + eta_s * 0.5 * (dudy + dvdx);
                }
                const double h = in.H[0][c], omh = 1 - h;
                xx = h * fxx + omh * ex;
                yy = h * fyy + omh * ey;
                xy = h * fxy + omh * exy;
            } else {   // functions.py:812-814
                const double ha = in.H[0][c], hb = in.H[1][c], hf = ha + hb - 1.0;
                const double oa = 1.0 - ha, ob = 1.0 - hb;
                xx = hf * fxx + oa * in.s[0][c] + ob * in.s[3][c];
                yy = hf * fyy + oa * in.s[2][c] + ob * in.s[5][c];
                xy = hf * fxy + oa * in.s[1][c] + ob * in.s[4][c];
            }
        }
        gxx[q] = xx; gxy[q] = xy; gyy[q] = yy;
    }
    __syncthreads();
    // 3. the right-hand side and the RK4 combination
    for (int q = threadIdx.x; q < M2_TX * M2_TY; q += M2_T) {
        const int ry = q / M2_TX, rx = q % M2_TX, j = j0 + ry, i = i0 + rx;
        if (j >= ny || i >= nx) continue;
        const long c = (long)j * nx + i;
        const int og = (ry + 2) * M2_GX + rx + 2, ou = (ry + 3) * M2_UX + rx + 3;
        const double divx = grad2(gxx + og, 1, i, nx, h2x) + grad2(gxy + og, M2_GX, j, ny, h2y);
        const double divy = grad2(gxy + og, 1, i, nx, h2x) + grad2(gyy + og, M2_GX, j, ny, h2y);
        const double uc = su[ou], vc = sv[ou];
        const double uadv = -uc * upwind3(su + ou, 1, i, nx, uc, dx) -
                            vc * upwind3(su + ou, M2_UX, j, ny, vc, dy);
        const double vadv = -uc * upwind3(sv + ou, 1, i, nx, uc, dx) -
                            vc * upwind3(sv + ou, M2_UX, j, ny, vc, dy);
        const double dpx = grad2(p + c, 1, i, nx, h2x), dpy = grad2(p + c, nx, j, ny, h2y);
        double rho;
        if constexpr (NS == 1) {
            const double h = in.H[0][c];
            rho = (1 - h) * rho_s + h * rho_f;
        } else {
            const double ha = in.H[0][c], hb = in.H[1][c];
            rho = (ha + hb - 1.0) * rho_f + (1.0 - ha) * rho_s + (1.0 - hb) * rho_s;
        }
        const double den = rho + 1e-12;
        const double bx = in.fx ? in.fx[c] : 0.0, by = in.fy ? in.fy[c] : 0.0;
        const double r1 = uadv + (divx + bx - dpx) / den;
        const double r2 = vadv + (divy + by - dpy) / den;
        if (stage < 3) {
            ku[c] = r1; kv[c] = r2;
        } else {
            outu[c] = u[c] + dt6 * (k1u[c] + 2 * k2u[c] + 2 * kpu[c] + r1);
            outv[c] = v[c] + dt6 * (k1v[c] + 2 * k2v[c] + 2 * kpv[c] + r2);
        }
    }
}

// the four stages and the final BC (functions.py:743-760 / :827-833); w: 6 planes (k1, k2, k3)
template <int NS>
static int mom2_stages(rmt_ctx *ctx, const rmt_momentum_params *P, const M2In &in,
                       const double *u, const double *v, const double *p, double *w,
                       double *u_new, double *v_new) {
    const int ny = ctx->ny, nx = ctx->nx;
    const long n = (long)ny * nx;
    double *ku[3] = {w, w + 2 * n, w + 4 * n}, *kv[3] = {w + n, w + 3 * n, w + 5 * n};
    const double coef[4] = {0.0, 0.5 * P->dt, 0.5 * P->dt, P->dt}, dt6 = P->dt / 6.0;
    const dim3 grid((nx + M2_TX - 1) / M2_TX, (ny + M2_TY - 1) / M2_TY);
    const int visc = NS == 1 && P->eta_s > 0.0;
    for (int s = 0; s < 4; ++s) {
        const double *kpu = s ? ku[s - 1] : u, *kpv = s ? kv[s - 1] : v;
        k_mom2_stage<NS><<<grid, M2_T, 0, ctx->stream>>>(
            u, v, p, kpu, kpv, coef[s], s, P->bc_kind, P->lid, in, visc, P->mu_f, P->eta_s,
            P->rho_s, P->rho_f, dt6, P->dx, P->dy, ny, nx, ku[0], kv[0], ku[1], kv[1],
            s < 3 ? ku[s] : nullptr, s < 3 ? kv[s] : nullptr, u_new, v_new);
        RMT_LAUNCHED();
    }
    return rmt_apply_velocity_bc(ctx, P->bc_kind, P->lid, u_new, v_new);
}

static int mom2_check(rmt_ctx *ctx, const rmt_momentum_params *P) {
    RMT_CHECK(ctx && P, RMT_EINVAL, "null argument");
    RMT_CHECK(P->bc_kind >= 0 && P->bc_kind <= 3, RMT_EINVAL, "unknown velocity bc kind");
    RMT_CHECK(ctx->ny >= 5 && ctx->nx >= 5, RMT_EINVAL, "grid too small for the stencils");
    return RMT_OK;
}

// rhs = rho * divU / dt pointwise (functions.py:1331); rhs may be div
__global__ void k_rhs_rho(const double *__restrict__ rho, const double *div, long n, double dt,
                          double *rhs) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c < n) rhs[c] = rho[c] * div[c] / dt;
}
// a = a* - (dt / rho) grad p_c, p = p_prev + p_c (functions.py:1352-1361), before the BC
__global__ void k_correct_rho(const double *__restrict__ a_s, const double *__restrict__ b_s,
                              const double *__restrict__ rho, const double *__restrict__ gx,
                              const double *__restrict__ gy, const double *__restrict__ pc,
                              const double *__restrict__ p_prev, long n, double dt,
                              double *__restrict__ a, double *__restrict__ b,
                              double *__restrict__ p) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double f = dt / rho[c];
    a[c] = a_s[c] - f * gx[c];
    b[c] = b_s[c] - f * gy[c];
    p[c] = p_prev ? p_prev[c] + pc[c] : pc[c];
}

// two_disc_contact.py:80-84: q * (phi <= 0).astype(float); out may be q
__global__ void k_mask_solid(const double *q, const double *__restrict__ phi, long n,
                             double *out) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c < n) out[c] = q[c] * (phi[c] <= 0.0 ? 1.0 : 0.0);
}
// the operands of benchmarks/common.py:110-115 disc_centroid (count, sum x, sum y over
// phi <= 0) as planes for reduce_sum
__global__ void k_solid_moments(const double *__restrict__ phi, const double *__restrict__ X,
                                const double *__restrict__ Y, long n, double *__restrict__ m) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= n) return;
    const bool s = phi[c] <= 0.0;
    m[c] = s ? 1.0 : 0.0; m[n + c] = s ? X[c] : 0.0; m[2 * n + c] = s ? Y[c] : 0.0;
}
// functions.py:792-795 / two_disc_contact.py:94-95: the n = 2 mixture density
__global__ void k_mixture_density(const double *__restrict__ phi_a,
                                  const double *__restrict__ phi_b, long n, double w_t,
                                  double rho_s, double rho_f, double *__restrict__ rho) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double ha = heaviside(phi_a[c], w_t), hb = heaviside(phi_b[c], w_t);
    rho[c] = (ha + hb - 1) * rho_f + (1 - ha) * rho_s + (1 - hb) * rho_s;
}
__global__ void k_negate(const double *__restrict__ x, long n, double *__restrict__ o) {
    const long c = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (c < n) o[c] = -x[c];
}

}  // namespace rmt

using namespace rmt;

extern "C" {

int rmt_compute_curvature(rmt_ctx *ctx, const double *phi, double dx, double dy, double *kappa) {
    RMT_CHECK(ctx && phi && kappa, RMT_EINVAL, "null argument");
    RMT_CHECK(ctx->ny >= 5 && ctx->nx >= 5, RMT_EINVAL, "grid too small for the stencils");
    const dim3 grid((ctx->nx + M2_TX - 1) / M2_TX, (ctx->ny + M2_TY - 1) / M2_TY);
    k_curvature<<<grid, M2_T, 0, ctx->stream>>>(phi, ctx->ny, ctx->nx, dx, dy, kappa);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_compute_contact_force(rmt_ctx *ctx, const double *phi1, const double *phi2, double k_rep,
                              double w_c, double dx, double dy, double *fx, double *fy) {
    RMT_CHECK(ctx && phi1 && phi2 && fx && fy, RMT_EINVAL, "null argument");
    RMT_CHECK(ctx->ny >= 5 && ctx->nx >= 5, RMT_EINVAL, "grid too small for the stencils");
    const long n = (long)ctx->ny * ctx->nx;
    k_contact_force<<<grid1d(n, 256), 256, 0, ctx->stream>>>(phi1, phi2, ctx->ny, ctx->nx, k_rep,
                                                              w_c, dx, dy, fx, fy);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_momentum_step_rk4_st(rmt_ctx *ctx, const rmt_momentum_params *P, double gamma,
                             const double *u, const double *v, const double *p, const double *X1,
                             const double *X2, const double *phi, double *u_new, double *v_new,
                             double *sxx, double *sxy, double *syy, double *J) {
    RMT_TRY(mom2_check(ctx, P));
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(ensure_scratch(ctx, 10 * n * sizeof(double)));
    double *w = ctx->scratch, *H = w + 6 * n, *kap = w + 7 * n, *fx = w + 8 * n, *fy = w + 9 * n;
    const double w_cut = P->stress_band ? P->w_t : 0.0, clamp = P->stress_band ? P->detg_clamp : 0.0;
    RMT_TRY(rmt_solid_cauchy_stress(ctx, X1, X2, P->dx, P->dy, P->mu_s, P->kappa, phi, w_cut,
                                    clamp, 0, sxx, sxy, syy, J));
    RMT_TRY(rmt_smoothed_heaviside(ctx, phi, n, P->w_t, H));
    RMT_TRY(rmt_compute_curvature(ctx, phi, P->dx, P->dy, kap));
    k_st_force<<<grid1d(n, 256), 256, 0, ctx->stream>>>(H, kap, ctx->ny, ctx->nx, gamma, P->dx,
                                                         P->dy, fx, fy);
    RMT_LAUNCHED();
    const M2In in{{sxx, sxy, syy, nullptr, nullptr, nullptr}, {H, nullptr}, phi, fx, fy};
    return mom2_stages<1>(ctx, P, in, u, v, p, w, u_new, v_new);
}

int rmt_momentum_step_rk4_2solids(rmt_ctx *ctx, const rmt_momentum_params *P, double k_rep,
                                  double w_c, const double *u, const double *v, const double *p,
                                  const double *X1a, const double *X2a, const double *X1b,
                                  const double *X2b, const double *phi_a, const double *phi_b,
                                  double *u_new, double *v_new, double *Jmin) {
    RMT_TRY(mom2_check(ctx, P));
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(ensure_scratch(ctx, 17 * n * sizeof(double)));
    double *w = ctx->scratch, *sa = w + 6 * n, *sb = w + 9 * n, *Ha = w + 12 * n, *Hb = w + 13 * n;
    double *fx = w + 14 * n, *fy = w + 15 * n, *Jb = w + 16 * n;
    // functions.py:787-790: w_cut = 0 (the one-sided interior stress), detg_clamp as passed
    RMT_TRY(rmt_solid_cauchy_stress(ctx, X1a, X2a, P->dx, P->dy, P->mu_s, P->kappa, phi_a, 0.0,
                                    P->detg_clamp, 0, sa, sa + n, sa + 2 * n, Jmin));
    RMT_TRY(rmt_solid_cauchy_stress(ctx, X1b, X2b, P->dx, P->dy, P->mu_s, P->kappa, phi_b, 0.0,
                                    P->detg_clamp, 0, sb, sb + n, sb + 2 * n, Jb));
    k_nanmin<<<grid1d(n, 256), 256, 0, ctx->stream>>>(Jmin, Jb, n, Jmin);
    RMT_LAUNCHED();
    RMT_TRY(rmt_smoothed_heaviside(ctx, phi_a, n, P->w_t, Ha));
    RMT_TRY(rmt_smoothed_heaviside(ctx, phi_b, n, P->w_t, Hb));
    const bool contact = k_rep > 0.0;
    if (contact)
        RMT_TRY(rmt_compute_contact_force(ctx, phi_a, phi_b, k_rep, w_c, P->dx, P->dy, fx, fy));
    const M2In in{{sa, sa + n, sa + 2 * n, sb, sb + n, sb + 2 * n}, {Ha, Hb}, nullptr,
                  contact ? fx : nullptr, contact ? fy : nullptr};
    return mom2_stages<2>(ctx, P, in, u, v, p, w, u_new, v_new);
}

int rmt_mask_solid(rmt_ctx *ctx, const double *q, const double *phi, double *out) {
    RMT_CHECK(ctx && q && phi && out, RMT_EINVAL, "null argument");
    const long n = (long)ctx->ny * ctx->nx;
    k_mask_solid<<<grid1d(n, 256), 256, 0, ctx->stream>>>(q, phi, n, out);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mixture_density(rmt_ctx *ctx, const double *phi_a, const double *phi_b, double w_t,
                        double rho_s, double rho_f, double *rho) {
    RMT_CHECK(ctx && phi_a && phi_b && rho, RMT_EINVAL, "null argument");
    const long n = (long)ctx->ny * ctx->nx;
    k_mixture_density<<<grid1d(n, 256), 256, 0, ctx->stream>>>(phi_a, phi_b, n, w_t, rho_s, rho_f,
                                                               rho);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_two_solid_diag(rmt_ctx *ctx, const double *phi_a, const double *phi_b, const double *X,
                       const double *Y, const double *Jmin, double *out5) {
    RMT_CHECK(ctx && phi_a && phi_b && X && Y && Jmin && out5, RMT_EINVAL, "null argument");
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(ensure_scratch(ctx, 3 * n * sizeof(double)));
    double *m = ctx->scratch, *r = ctx->red + RED_BLOCKS + 20;   // 7 result slots
    const double *phis[2] = {phi_a, phi_b};
    for (int s = 0; s < 2; ++s) {
        k_solid_moments<<<grid1d(n, 256), 256, 0, ctx->stream>>>(phis[s], X, Y, n, m);
        RMT_LAUNCHED();
        for (int k = 0; k < 3; ++k) RMT_TRY(reduce_sum(ctx, m + k * n, n, r + 3 * s + k));
    }
    // min J = -max(-J), a NaN kept as Jmin.min() keeps it (two_disc_contact.py:104)
    k_negate<<<grid1d(n, 256), 256, 0, ctx->stream>>>(Jmin, n, m);
    RMT_LAUNCHED();
    RMT_TRY(reduce_max(ctx, m, n, r + 6));
    double h[7];
    RMT_HIP(hipMemcpyAsync(h, r, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    out5[0] = h[1] / h[0]; out5[1] = h[2] / h[0];   // no solid cell: NaN, as the reference
    out5[2] = h[4] / h[3]; out5[3] = h[5] / h[3];
    out5[4] = -h[6];
    return RMT_OK;
}

int rmt_pressure_projection_rho_field(rmt_ctx *ctx, const double *a_star, const double *b_star,
                                      double dx, double dy, double dt, const double *rho,
                                      int bc_kind, double lid, const double *p_prev, double *a,
                                      double *b, double *p) {
    RMT_CHECK(ctx && a_star && b_star && rho && a && b && p, RMT_EINVAL, "null argument");
    RMT_CHECK(bc_kind >= 0 && bc_kind <= 3, RMT_EINVAL, "unknown velocity bc kind");
    const long n = (long)ctx->ny * ctx->nx;
    RMT_TRY(ensure_scratch(ctx, (4 * n + n / 8192 + 8) * sizeof(double)));
    double *rhs = ctx->scratch, *pc = rhs + n, *gx = pc + n, *gy = gx + n, *part = gy + n;
    if (p_prev) {
        // functions.py:1049: d_f = dt / float(np.mean(rho)), the sum in np.sum's order
        double s;
        RMT_TRY(np_sum(ctx, rho, n, part, &s));
        RMT_TRY(rmt_divergence_rc(ctx, a_star, b_star, p_prev, dt / (s / (double)n), dx, dy, rhs));
    } else {
        RMT_TRY(rmt_divergence_central(ctx, a_star, b_star, dx, dy, rhs));
    }
    k_rhs_rho<<<grid1d(n, 256), 256, 0, ctx->stream>>>(rho, rhs, n, dt, rhs);
    RMT_LAUNCHED();
    RMT_TRY(dct_solve(ctx, rhs, dx, dy, pc));
    RMT_TRY(rmt_pressure_gradient(ctx, pc, dx, dy, gx, gy));
    k_correct_rho<<<grid1d(n, 256), 256, 0, ctx->stream>>>(a_star, b_star, rho, gx, gy, pc, p_prev,
                                                            n, dt, a, b, p);
    RMT_LAUNCHED();
    RMT_TRY(rmt_apply_velocity_bc(ctx, bc_kind, lid, a, b));
    return sub_mean_rows(ctx, p, ctx->ny, ctx->nx);
}

}  // extern "C"
