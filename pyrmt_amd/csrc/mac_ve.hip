// mac_ve.hip -- the coupling of the viscoelastic constitutive layer (viscoelastic.hip) to the
// periodic staggered tier (macper.hip): the kernels of one step of
// benchmarks/mac_viscoelastic_extension.py (a soft blob at the stagnation point of a four-roll
// mill) that neither of the two has.
//   rmt_mac_ve_centre_kinematics       :106, :119-120   u_c, v_c and the velocity gradient
//   rmt_mac_ve_face_force              :125-131         f_su, f_sv, Hu, Hv, chi = 1 - H
//   rmt_mac_per_imex_elastic_rhs /
//   rmt_mac_per_predictor_imex_elastic mac.py:560-584   right-hand side, two Helmholtz solves
//   rmt_mac_ve_lock                    :139-155         forcing and the lock to the mill
//   rmt_mac_ve_record                  :159-171         the step's record and stop test
// Planes are (ny, nx), ny, nx >= 3, i fastest.  The face averages wrap (np.roll); the gradients
// do not: they are utils.py:5-14, one-sided at the first and last column / row.  Every
// expression keeps the reference's operand order (-ffp-contract=off): the kernels give its bits
// except through sin (H), exp (the exact lock) and the FFT pair.  No kernel forms an index from
// data: every address comes from the thread's cell and the extents, so huge and non-finite
// values pass through as values.
#include "macper.hpp"

namespace rmt {

// utils.py:8-13 from three taps: at the low end (f0, f1, f2) = (f[k], f[k+1], f[k+2]), at the
// high end (f[k], f[k-1], f[k-2]), inside (f[k+1], f[k-1], unused)
__device__ __forceinline__ double mve_g3(double f0, double f1, double f2, int k, int n,
                                         double h2) {
    if (k == 0) return (-3 * f0 + 4 * f1 - f2) / h2;
    if (k == n - 1) return (3 * f0 - 4 * f1 + f2) / h2;
    return (f0 - f1) / h2;
}
// the offsets of the three taps of mve_g3 at index k of n
__device__ __forceinline__ void mve_taps(int k, int n, int &o0, int &o1, int &o2) {
    if (k == 0) { o0 = 0; o1 = 1; o2 = 2; }
    else if (k == n - 1) { o0 = 0; o1 = -1; o2 = -2; }
    else { o0 = 1; o1 = -1; o2 = 0; }
}

// ------------------------------------------------------------ centre kinematics ----
// One thread a cell: the averages of its three taps along each axis are formed from the face
// planes as needed (each 0.5 * (f + f_next), the bits of the stored u_c / v_c).
__global__ void __launch_bounds__(256) k_mve_kin(
    const double *__restrict__ u, const double *__restrict__ v, int ny, int nx, double twodx,
    double twody, double *__restrict__ uc, double *__restrict__ vc, double *__restrict__ L11,
    double *__restrict__ L12, double *__restrict__ L21, double *__restrict__ L22) {
    const long c = blockIdx.x * 256L + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    auto UC = [&](int jj, int ii) {
        const long r = (long)jj * nx;
        return 0.5 * (u[r + ii] + u[r + (ii + 1 == nx ? 0 : ii + 1)]);
    };
    auto VC = [&](int jj, int ii) {
        return 0.5 * (v[(long)jj * nx + ii] + v[(long)(jj + 1 == ny ? 0 : jj + 1) * nx + ii]);
    };
    int a0, a1, a2, b0, b1, b2;
    mve_taps(i, nx, a0, a1, a2);
    mve_taps(j, ny, b0, b1, b2);
    uc[c] = UC(j, i);
    vc[c] = VC(j, i);
    L11[c] = mve_g3(UC(j, i + a0), UC(j, i + a1), UC(j, i + a2), i, nx, twodx);
    L12[c] = mve_g3(UC(j + b0, i), UC(j + b1, i), UC(j + b2, i), j, ny, twody);
    L21[c] = mve_g3(VC(j, i + a0), VC(j, i + a1), VC(j, i + a2), i, nx, twodx);
    L22[c] = mve_g3(VC(j + b0, i), VC(j + b1, i), VC(j + b2, i), j, ny, twody);
}

// ------------------------------------------------------------------- face force ----
// A workgroup owns an MVE_TX x MVE_TY tile of cells and stages H and S = (1 - H) G b_e of the
// periodic window around it in LDS: three cells west / south, two east / north, loaded through
// wrapped indices (so a partial tile and an extent below the tile see the same neighbours as
// any other cell).  div S is then formed on the tile plus one column west (x component) and
// one row south (y component) -- a cell's gradient taps lie within two cells of it in the
// window, on the side utils.py:8-13 puts them for the cell's own index -- and the faces
// average it with its wrapped neighbour.  H (one sine in the band) is evaluated once a window
// cell, not once a tap.
constexpr int MVE_TX = 32, MVE_TY = 16, MVE_LO = 3, MVE_HI = 2;
constexpr int MVE_WX = MVE_TX + MVE_LO + MVE_HI, MVE_WY = MVE_TY + MVE_LO + MVE_HI;
constexpr int MVE_THREADS = 256;

template <int WX>
__device__ __forceinline__ double mve_gx(const double (*s)[WX], int a, int b, int gi, int nx,
                                         double h2) {
    int o0, o1, o2;
    mve_taps(gi, nx, o0, o1, o2);
    return mve_g3(s[a][b + o0], s[a][b + o1], s[a][b + o2], gi, nx, h2);
}
template <int WX>
__device__ __forceinline__ double mve_gy(const double (*s)[WX], int a, int b, int gj, int ny,
                                         double h2) {
    int o0, o1, o2;
    mve_taps(gj, ny, o0, o1, o2);
    return mve_g3(s[a + o0][b], s[a + o1][b], s[a + o2][b], gj, ny, h2);
}

__global__ void __launch_bounds__(MVE_THREADS) k_mve_face_force(
    const double *__restrict__ be11, const double *__restrict__ be12,
    const double *__restrict__ be22, const double *__restrict__ phi, int ny, int nx, double G,
    double w_t, double twodx, double twody, double *__restrict__ f_su,
    double *__restrict__ f_sv, double *__restrict__ Hu, double *__restrict__ Hv,
    double *__restrict__ chi) {
    __shared__ double sxx[MVE_WY][MVE_WX], sxy[MVE_WY][MVE_WX], syy[MVE_WY][MVE_WX],
        sh[MVE_WY][MVE_WX];
    __shared__ double dvx[MVE_TY][MVE_TX + 1], dvy[MVE_TY + 1][MVE_TX];
    const int i0 = blockIdx.x * MVE_TX, j0 = blockIdx.y * MVE_TY, t = threadIdx.x;
    for (int q = t; q < MVE_WY * MVE_WX; q += MVE_THREADS) {
        const int lj = q / MVE_WX, li = q % MVE_WX;
        const long g = (long)macp_wrap(j0 - MVE_LO + lj, ny) * nx + macp_wrap(i0 - MVE_LO + li, nx);
        const double H = heaviside(phi[g], w_t);
        const double s = (1 - H) * G;
        sh[lj][li] = H;
        sxx[lj][li] = s * be11[g];
        sxy[lj][li] = s * be12[g];
        syy[lj][li] = s * be22[g];
    }
    __syncthreads();
    // tile cell (lj, li) is window cell (lj + MVE_LO, li + MVE_LO); dvx column li is the cell
    // column i0 - 1 + li, dvy row lj the cell row j0 - 1 + lj
    for (int q = t; q < MVE_TY * (MVE_TX + 1); q += MVE_THREADS) {
        const int lj = q / (MVE_TX + 1), li = q % (MVE_TX + 1);
        const int a = lj + MVE_LO, b = li + MVE_LO - 1;
        const int gj = macp_wrap(j0 + lj, ny), gi = macp_wrap(i0 - 1 + li, nx);
        dvx[lj][li] = mve_gx<MVE_WX>(sxx, a, b, gi, nx, twodx)
                    + mve_gy<MVE_WX>(sxy, a, b, gj, ny, twody);
    }
    for (int q = t; q < (MVE_TY + 1) * MVE_TX; q += MVE_THREADS) {
        const int lj = q / MVE_TX, li = q % MVE_TX;
        const int a = lj + MVE_LO - 1, b = li + MVE_LO;
        const int gj = macp_wrap(j0 - 1 + lj, ny), gi = macp_wrap(i0 + li, nx);
        dvy[lj][li] = mve_gx<MVE_WX>(sxy, a, b, gi, nx, twodx)
                    + mve_gy<MVE_WX>(syy, a, b, gj, ny, twody);
    }
    __syncthreads();
    for (int q = t; q < MVE_TY * MVE_TX; q += MVE_THREADS) {
        const int lj = q / MVE_TX, li = q % MVE_TX, gj = j0 + lj, gi = i0 + li;
        if (gj >= ny || gi >= nx) continue;
        const long c = (long)gj * nx + gi;
        const int a = lj + MVE_LO, b = li + MVE_LO;
        const double H = sh[a][b];
        f_su[c] = 0.5 * (dvx[lj][li + 1] + dvx[lj][li]);
        f_sv[c] = 0.5 * (dvy[lj + 1][li] + dvy[lj][li]);
        Hu[c] = 0.5 * (H + sh[a][b - 1]);
        Hv[c] = 0.5 * (H + sh[a - 1][b]);
        chi[c] = 1.0 - H;
    }
}

// ---------------------------------------------------- elastic IMEX right-hand side ----
// mac.py:566-579 at every face: the IMEX advection term (macp_ustar / macp_vstar, imex = 1),
// the force inside the solve and the defect c_el (1 - chi_face) lap that takes the constant
// stabiliser out of the fluid.
__global__ void __launch_bounds__(256) k_mve_rhs(
    const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ chi,
    const double *__restrict__ fu, const double *__restrict__ fv, int ny, int nx, MacpCoef k,
    double c_el, double rho, double *__restrict__ ru, double *__restrict__ rv) {
    const long c = blockIdx.x * 256L + threadIdx.x;
    if (c >= (long)ny * nx) return;
    const int j = (int)(c / nx), i = (int)(c % nx);
    const int ip = i + 1 == nx ? 0 : i + 1, im = i == 0 ? nx - 1 : i - 1;
    const long r = (long)j * nx, rp = (long)(j + 1 == ny ? 0 : j + 1) * nx,
               rm = (long)(j == 0 ? ny - 1 : j - 1) * nx;
    const double uc = u[c], uE = u[r + ip], uW = u[r + im], uN = u[rp + i], uS = u[rm + i];
    const double vc = v[c], vE = v[r + ip], vW = v[r + im], vN = v[rp + i], vS = v[rm + i];
    const double au = macp_ustar(uc, uE, uW, uN, uS, vc, vW, vN, v[rp + im], k, 1);
    const double av = macp_vstar(vc, vE, vW, vN, vS, uc, uE, uS, u[rm + ip], k, 1);
    const double lapu = ((uE - 2 * uc) + uW) / k.dx2 + ((uN - 2 * uc) + uS) / k.dy2;
    const double lapv = ((vE - 2 * vc) + vW) / k.dx2 + ((vN - 2 * vc) + vS) / k.dy2;
    const double xc = chi[c];
    const double chi_u = 0.5 * (xc + chi[r + im]), chi_v = 0.5 * (xc + chi[rm + i]);
    ru[c] = (au + k.dt * fu[c] / rho) + c_el * (1.0 - chi_u) * lapu;
    rv[c] = (av + k.dt * fv[c] / rho) + c_el * (1.0 - chi_v) * lapv;
}

// ------------------------------------------------------------------------- lock ----
// MVE_EXPLICIT :152-155, u* + dt (f_s + Hf beta (mill - u)) / rho; MVE_IMEX :147-150 and
// MVE_ELASTIC :139-141, mill + (u* [+ dt f_s / rho] - mill) exp(-dt beta Hf / rho), ndb the
// host's -dt * beta.  One component a call; out may be star.
enum { MVE_EXPLICIT = 0, MVE_IMEX = 1, MVE_ELASTIC = 2 };
template <int MODE>
__global__ void __launch_bounds__(256) k_mve_lock(
    const double *star, const double *__restrict__ u, const double *__restrict__ f_s,
    const double *__restrict__ Hf, const double *__restrict__ mill, long n, double dt, double beta,
    double ndb, double rho, double *out) {
    const long c = blockIdx.x * 256L + threadIdx.x;
    if (c >= n) return;
    if (MODE == MVE_EXPLICIT) {
        const double f = f_s[c] + Hf[c] * beta * (mill[c] - u[c]);
        out[c] = star[c] + dt * f / rho;
        return;
    }
    double s = star[c];
    if (MODE == MVE_IMEX) s = s + dt * f_s[c] / rho;
    const double ep = exp(ndb * Hf[c] / rho);
    const double m = mill[c];
    out[c] = m + (s - m) * ep;
}

// ------------------------------------------------------------------- record ----
// :159-171 as one reduction ("Reduction contract": every cell reaches the result,
// NaN as in the reference): the largest eigenvalue of b_e over phi <= 0 (nanmax; -inf without
// such a cell), the number of those cells, max |u| (np.max: a NaN comes out) and the number of
// non-finite cells of u.  MR_RB workgroups leave partials in ctx->red, one folds them: a
// constant launch shape.
constexpr int VR_RB = 256, VR_T = 256, VR_NQ = 4;
static_assert(VR_NQ * VR_RB <= RED_BLOCKS + 64, "ctx->red holds the partials");
struct VrAcc { double mx, ct, um, bad; };
__device__ __forceinline__ void vr_fold(VrAcc *s, VrAcc &a) {
    s[threadIdx.x] = a;
    __syncthreads();
    tree_fold<VR_T>([&](int t, int w) {
        s[t].mx = nanmax(s[t].mx, s[w].mx);
        s[t].ct = s[t].ct + s[w].ct;
        s[t].um = nanmax(s[t].um, s[w].um);
        s[t].bad = s[t].bad + s[w].bad;
    });
    a = s[0];
}
__global__ void __launch_bounds__(VR_T) k_mve_record_p1(
    const double *__restrict__ b11, const double *__restrict__ b12,
    const double *__restrict__ b22, const double *__restrict__ phi, const double *__restrict__ u,
    long n, double *__restrict__ part) {
    __shared__ VrAcc s[VR_T];
    VrAcc a = {-INFINITY, 0.0, -INFINITY, 0.0};
    for (long k = blockIdx.x * (long)VR_T + threadIdx.x; k < n; k += (long)VR_RB * VR_T) {
        if (phi[k] <= 0.0) {
            const double p = b11[k], q = b12[k], r = b22[k];
            const double tr = 0.5 * (p + r), h = p - r;
            a.mx = nanmax(a.mx, tr + sqrt(nanmax(0.25 * (h * h) + q * q, 0.0)));
            a.ct += 1.0;
        }
        const double w = u[k];
        a.um = nanmax(a.um, fabs(w));
        if (!isfinite(w)) a.bad += 1.0;
    }
    vr_fold(s, a);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a.mx; part[VR_RB + blockIdx.x] = a.ct;
        part[2 * VR_RB + blockIdx.x] = a.um; part[3 * VR_RB + blockIdx.x] = a.bad;
    }
}
__global__ void __launch_bounds__(VR_T) k_mve_record_p2(const double *__restrict__ part,
                                                        const double *__restrict__ b11, long at,
                                                        double *__restrict__ out5) {
    __shared__ VrAcc s[VR_T];
    static_assert(VR_RB == VR_T, "one partial a thread");
    const int t = threadIdx.x;
    VrAcc a = {part[t], part[VR_RB + t], part[2 * VR_RB + t], part[3 * VR_RB + t]};
    vr_fold(s, a);
    if (t == 0) {
        out5[0] = a.mx; out5[1] = a.ct; out5[2] = b11[at]; out5[3] = a.um;
        out5[4] = a.bad == 0.0 ? 1.0 : 0.0;
    }
}

static int mve_extents(rmt_ctx *ctx, const char *what) {
    RMT_CHECK(ctx && ctx->ny >= 3 && ctx->nx >= 3, RMT_EINVAL, what);
    return RMT_OK;
}
static bool mve_distinct(const void *const *outs, int no, const void *const *ins, int ni) {
    for (int a = 0; a < no; ++a) {
        for (int b = 0; b < ni; ++b)
            if (outs[a] == ins[b]) return false;
        for (int b = a + 1; b < no; ++b)
            if (outs[a] == outs[b]) return false;
    }
    return true;
}

static int mve_rhs(rmt_ctx *ctx, const double *u, const double *v, double twodx, double twody,
                   double dx2, double dy2, double dt, double c_el, double rho, const double *chi,
                   const double *fu, const double *fv, double *ru, double *rv) {
    const long n = N_CELLS;
    k_mve_rhs<<<grid1d(n, 256), 256, 0, ctx->stream>>>(
        u, v, chi, fu, fv, ctx->ny, ctx->nx, MacpCoef{0.0, dx2, dy2, twodx, twody, dt}, c_el, rho,
        ru, rv);
    RMT_LAUNCHED();
    return RMT_OK;
}

}  // namespace rmt
using namespace rmt;

int rmt_mac_ve_centre_kinematics(rmt_ctx *ctx, const double *u, const double *v, double dx,
                                 double dy, double *u_c, double *v_c, double *const *L) {
    RMT_TRY(mve_extents(ctx, "rmt_mac_ve_centre_kinematics: a context with ny, nx >= 3"));
    RMT_CHECK(u && v && u_c && v_c && L && L[0] && L[1] && L[2] && L[3], RMT_EINVAL,
              "rmt_mac_ve_centre_kinematics: null argument");
    const void *outs[6] = {u_c, v_c, L[0], L[1], L[2], L[3]}, *ins[2] = {u, v};
    RMT_CHECK(mve_distinct(outs, 6, ins, 2), RMT_EINVAL,
              "rmt_mac_ve_centre_kinematics: the outputs are six planes of their own");
    k_mve_kin<<<grid1d(N_CELLS, 256), 256, 0, ctx->stream>>>(u, v, ctx->ny, ctx->nx, 2 * dx,
                                                             2 * dy, u_c, v_c, L[0], L[1], L[2],
                                                             L[3]);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_ve_face_force(rmt_ctx *ctx, const double *const *be, const double *phi, double G,
                          double w_t, double dx, double dy, double *f_su, double *f_sv, double *Hu,
                          double *Hv, double *chi) {
    RMT_TRY(mve_extents(ctx, "rmt_mac_ve_face_force: a context with ny, nx >= 3"));
    RMT_CHECK(be && be[0] && be[1] && be[2] && phi && f_su && f_sv && Hu && Hv && chi, RMT_EINVAL,
              "rmt_mac_ve_face_force: null argument");
    const void *outs[5] = {f_su, f_sv, Hu, Hv, chi}, *ins[4] = {be[0], be[1], be[2], phi};
    RMT_CHECK(mve_distinct(outs, 5, ins, 4), RMT_EINVAL,
              "rmt_mac_ve_face_force: the outputs are five planes of their own");
    const dim3 tiles((ctx->nx + MVE_TX - 1) / MVE_TX, (ctx->ny + MVE_TY - 1) / MVE_TY);
    k_mve_face_force<<<tiles, MVE_THREADS, 0, ctx->stream>>>(be[0], be[1], be[2], phi, ctx->ny,
                                                             ctx->nx, G, w_t, 2 * dx, 2 * dy, f_su,
                                                             f_sv, Hu, Hv, chi);
    RMT_LAUNCHED();
    return RMT_OK;
}

static int mve_rhs_args(rmt_ctx *ctx, const double *u, const double *v, const double *chi,
                        const double *fu, const double *fv, double *ru, double *rv) {
    RMT_TRY(mve_extents(ctx, "elastic IMEX predictor: a context with ny, nx >= 3"));
    RMT_CHECK(u && v && chi && fu && fv && ru && rv, RMT_EINVAL,
              "elastic IMEX predictor: null argument");
    const void *outs[2] = {ru, rv}, *ins[5] = {u, v, chi, fu, fv};
    RMT_CHECK(mve_distinct(outs, 2, ins, 5), RMT_EINVAL, "elastic IMEX predictor: not in place");
    return RMT_OK;
}

int rmt_mac_per_imex_elastic_rhs(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                                 double twody, double dx2, double dy2, double dt, double c_el,
                                 double rho, const double *chi, const double *fu,
                                 const double *fv, double *rhs_u, double *rhs_v) {
    RMT_TRY(mve_rhs_args(ctx, u, v, chi, fu, fv, rhs_u, rhs_v));
    return mve_rhs(ctx, u, v, twodx, twody, dx2, dy2, dt, c_el, rho, chi, fu, fv, rhs_u, rhs_v);
}

int rmt_mac_per_predictor_imex_elastic(rmt_ctx *ctx, const double *u, const double *v,
                                       double twodx, double twody, double dx2, double dy2,
                                       double dt, double c_el, double coef, double rho,
                                       const double *chi, const double *fu, const double *fv,
                                       const double *lx, const double *ly, double *u_star,
                                       double *v_star) {
    RMT_TRY(mve_rhs_args(ctx, u, v, chi, fu, fv, u_star, v_star));
    RMT_CHECK(lx && ly, RMT_EINVAL, "elastic IMEX predictor: null symbol");
    RMT_TRY(macp_workspace(ctx, 0));
    RMT_TRY(macp_plan(ctx, lx, ly));
    RMT_TRY(mve_rhs(ctx, u, v, twodx, twody, dx2, dy2, dt, c_el, rho, chi, fu, fv, u_star,
                    v_star));
    RMT_TRY(macp_solve(ctx, u_star, 1, coef, u_star));                       // mac.py:580-583
    return macp_solve(ctx, v_star, 1, coef, v_star);
}

int rmt_mac_ve_lock(rmt_ctx *ctx, int mode, long n, const double *star, const double *u,
                    const double *f_s, const double *Hf, const double *mill, double dt,
                    double beta, double rho, double *out) {
    RMT_CHECK(ctx && n >= 1 && star && Hf && mill && out, RMT_EINVAL,
              "rmt_mac_ve_lock: null argument");
    RMT_CHECK(mode >= MVE_EXPLICIT && mode <= MVE_ELASTIC, RMT_EINVAL,
              "rmt_mac_ve_lock: mode 0 explicit, 1 imex, 2 imex-elastic");
    RMT_CHECK((mode == MVE_ELASTIC || f_s) && (mode != MVE_EXPLICIT || u), RMT_EINVAL,
              "rmt_mac_ve_lock: the mode's planes (explicit: u, f_s; imex: f_s)");
    const double ndb = -dt * beta;
    const unsigned g = grid1d(n, 256);
    if (mode == MVE_EXPLICIT)
        k_mve_lock<MVE_EXPLICIT><<<g, 256, 0, ctx->stream>>>(star, u, f_s, Hf, mill, n, dt, beta,
                                                             ndb, rho, out);
    else if (mode == MVE_IMEX)
        k_mve_lock<MVE_IMEX><<<g, 256, 0, ctx->stream>>>(star, u, f_s, Hf, mill, n, dt, beta, ndb,
                                                         rho, out);
    else
        k_mve_lock<MVE_ELASTIC><<<g, 256, 0, ctx->stream>>>(star, u, f_s, Hf, mill, n, dt, beta,
                                                            ndb, rho, out);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_mac_ve_record(rmt_ctx *ctx, long n, const double *const *be, const double *phi,
                      const double *u, long at, double *out5) {
    RMT_CHECK(ctx && n >= 1 && be && be[0] && be[1] && be[2] && phi && u && out5, RMT_EINVAL,
              "rmt_mac_ve_record: null argument");
    RMT_CHECK(at >= 0 && at < n, RMT_EINVAL, "rmt_mac_ve_record: `at` is a flat index below n");
    k_mve_record_p1<<<VR_RB, VR_T, 0, ctx->stream>>>(be[0], be[1], be[2], phi, u, n, ctx->red);
    k_mve_record_p2<<<1, VR_T, 0, ctx->stream>>>(ctx->red, be[0], at, out5);
    RMT_LAUNCHED();
    return RMT_OK;
}
