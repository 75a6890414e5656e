// viscoelastic.hip -- the viscoelastic constitutive layer (pyRMT/viscoelastic.py): the
// upper-convected Maxwell update of the Finger tensor b_e, its log-conformation form
// psi = log(b_e) (Fattal & Kupferman 2004) with the explicit and the Strang steppers, the two
// matrix functions, the stress, and the reduction the uniform-extension loop reads.
//   rmt_ve_ucm_rhs / _steps    :27-54   ucm_local_rhs, ucm_local_step x nsteps
//   rmt_ve_stress              :167-179 viscoelastic_stress
//   rmt_ve_sym_log / _exp      :63-84   through _sym_eig2
//   rmt_ve_logconf_rhs         :87-116  logconf_local_rhs
//   rmt_ve_relax_exact         :133-147
//   rmt_ve_logconf_steps       :119-125, :150-164  either stepper x nsteps
//   rmt_ve_lam_max             benchmarks/mac_viscoelastic_uniform.py:30-32, :90-92
// Every kernel is elementwise over n cells of equally long planes (a cell's symmetric tensor
// is three planes 11, 12, 22; a velocity gradient four planes 11, 12, 21, 22); the fused
// steppers keep a cell's state in registers between steps.  Every expression keeps the
// reference's operand order (-ffp-contract=off): the arithmetic kernels give the reference's
// bits, the others differ from it only through exp, log, sin, cos and atan2 -- each evaluated
// where the reference evaluates it, never rewritten (no 1 / exp(x) for exp(-x), no double
// angle).  np.maximum's NaN rule is nanmax.  An output plane may be its input plane.
#include "rmt_internal.hpp"

namespace rmt {

// The elementwise launch: VE_T threads a workgroup, at most VE_MAXB workgroups, each thread
// walking k, k + blocks * VE_T, ...
constexpr int VE_T = 256, VE_MAXB = 2048;
inline unsigned ve_blocks(long n) {
    return (unsigned)std::max(1L, std::min<long>((n + VE_T - 1) / VE_T, VE_MAXB));
}

struct VeS3 { double a, b, c; };               // [[a, b], [b, c]]
struct VeL4 { double l11, l12, l21, l22; };
struct VeIn3 { const double *p[3]; };
struct VeIn4 { const double *p[4]; };
struct VeOut3 { double *p[3]; };

__device__ __forceinline__ VeS3 ve_load(const VeIn3 &P, long k) {
    return {P.p[0][k], P.p[1][k], P.p[2][k]};
}
__device__ __forceinline__ VeL4 ve_load(const VeIn4 &P, long k) {
    return {P.p[0][k], P.p[1][k], P.p[2][k], P.p[3][k]};
}
__device__ __forceinline__ void ve_store(const VeOut3 &P, long k, const VeS3 &s) {
    P.p[0][k] = s.a; P.p[1][k] = s.b; P.p[2][k] = s.c;
}

// ------------------------------------------------------------------------- UCM ----
__device__ __forceinline__ VeS3 ucm_rhs(const VeS3 &b, const VeL4 &L, double inv_tau) {  // :35-42
    const double D11 = 2.0 * (L.l11 * b.a + L.l12 * b.b);
    const double D12 = (L.l11 * b.b + L.l12 * b.c) + (L.l21 * b.a + L.l22 * b.b);
    const double D22 = 2.0 * (L.l21 * b.b + L.l22 * b.c);
    return {D11 - inv_tau * (b.a - 1.0), D12 - inv_tau * b.b, D22 - inv_tau * (b.c - 1.0)};
}
__device__ __forceinline__ VeS3 ucm_step(const VeS3 &b, const VeL4 &L, double inv_tau,
                                         double dt) {                                   // :48-54
    const VeS3 k1 = ucm_rhs(b, L, inv_tau);
    const VeS3 p = {b.a + dt * k1.a, b.b + dt * k1.b, b.c + dt * k1.c};
    const VeS3 k2 = ucm_rhs(p, L, inv_tau);
    return {b.a + 0.5 * dt * (k1.a + k2.a), b.b + 0.5 * dt * (k1.b + k2.b),
            b.c + 0.5 * dt * (k1.c + k2.c)};
}

__global__ void __launch_bounds__(VE_T) k_ve_ucm_rhs(VeIn3 B, VeIn4 Lp, long n, double inv_tau,
                                                     VeOut3 O) {
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride)
        ve_store(O, k, ucm_rhs(ve_load(B, k), ve_load(Lp, k), inv_tau));
}

// track (each of its three entries may be null): nsteps values a component is compared with
// after each step; err[k] is the largest |component - track| met, as the driver's running
// max(err, abs(..)) keeps it (a NaN difference never replaces err)
__global__ void __launch_bounds__(VE_T) k_ve_ucm_steps(VeIn3 B, VeIn4 Lp, long n, double inv_tau,
                                                       double dt, int nsteps, VeIn3 track,
                                                       double *err, VeOut3 O) {
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride) {
        VeS3 b = ve_load(B, k);
        const VeL4 L = ve_load(Lp, k);
        double e = 0.0;
        for (int s = 0; s < nsteps; ++s) {
            b = ucm_step(b, L, inv_tau, dt);
            if (err) {
                const double v[3] = {b.a, b.b, b.c};
                for (int c = 0; c < 3; ++c)
                    if (track.p[c]) {
                        const double d = fabs(v[c] - track.p[c][s]);
                        if (d > e) e = d;
                    }
            }
        }
        ve_store(O, k, b);
        if (err) err[k] = e;
    }
}

__global__ void __launch_bounds__(VE_T) k_ve_stress(VeIn3 B, long n, double G, VeIn3 R, int zener,
                                                    double G_inf, VeOut3 O) {        // :174-179
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride) {
        const VeS3 b = ve_load(B, k);
        VeS3 s = {G * b.a, G * b.b, G * b.c};
        if (zener) {
            const VeS3 r = ve_load(R, k);
            s.a = s.a + G_inf * r.a; s.b = s.b + G_inf * r.b; s.c = s.c + G_inf * r.c;
        }
        ve_store(O, k, s);
    }
}

// ------------------------------------------------------------ log-conformation ----
struct VeEig { double l1, l2, th; };
__device__ __forceinline__ VeEig sym_eig2(const VeS3 &s) {                             // :66-68
    const double tr = 0.5 * (s.a + s.c);
    const double h = s.a - s.c;
    const double d = sqrt(nanmax(0.25 * (h * h) + s.b * s.b, 0.0));
    return {tr + d, tr - d, 0.5 * atan2(2.0 * s.b, h)};
}
// R diag(f1, f2) R^T                                                                     :76, :84
__device__ __forceinline__ VeS3 ve_rotate(double cs, double sn, double f1, double f2) {
    return {cs * cs * f1 + sn * sn * f2, cs * sn * (f1 - f2), sn * sn * f1 + cs * cs * f2};
}
__device__ __forceinline__ VeS3 sym_log(const VeS3 &s) {                                // :73-76
    const VeEig e = sym_eig2(s);
    const double f1 = log(nanmax(e.l1, 1e-300)), f2 = log(nanmax(e.l2, 1e-300));
    return ve_rotate(cos(e.th), sin(e.th), f1, f2);
}
__device__ __forceinline__ VeS3 sym_exp(const VeS3 &s) {                                // :81-84
    const VeEig e = sym_eig2(s);
    const double f1 = exp(e.l1), f2 = exp(e.l2);
    return ve_rotate(cos(e.th), sin(e.th), f1, f2);
}

__device__ __forceinline__ VeS3 logconf_rhs(const VeS3 &p, const VeL4 &L, double inv_tau) {
    const VeEig e = sym_eig2(p);                                                        // :92-116
    const double cs = cos(e.th), sn = sin(e.th);
    const double a11 = cs * L.l11 + sn * L.l21, a12 = cs * L.l12 + sn * L.l22;
    const double a21 = -sn * L.l11 + cs * L.l21, a22 = -sn * L.l12 + cs * L.l22;
    const double M11 = a11 * cs + a12 * sn, M12 = -a11 * sn + a12 * cs;
    const double M21 = a21 * cs + a22 * sn, M22 = -a21 * sn + a22 * cs;
    const double lam1 = exp(e.l1), lam2 = exp(e.l2);
    const double denom = lam2 - lam1;
    const bool deg = fabs(denom) < 1e-10;
    const double em1 = exp(-e.l1);      // :106 and :109 call it with the same argument
    const double ratio = deg ? em1 : (e.l2 - e.l1) / denom;
    const double E11 = 2.0 * M11 + inv_tau * (em1 - 1.0);
    const double E22 = 2.0 * M22 + inv_tau * (exp(-e.l2) - 1.0);
    const double E12 = ratio * (lam2 * M12 + lam1 * M21);
    return {cs * cs * E11 - 2.0 * cs * sn * E12 + sn * sn * E22,
            cs * sn * (E11 - E22) + (cs * cs - sn * sn) * E12,
            sn * sn * E11 + 2.0 * cs * sn * E12 + cs * cs * E22};
}
__device__ __forceinline__ VeS3 logconf_step(const VeS3 &p, const VeL4 &L, double inv_tau,
                                             double dt) {                             // :121-125
    const VeS3 k1 = logconf_rhs(p, L, inv_tau);
    const VeS3 q = {p.a + dt * k1.a, p.b + dt * k1.b, p.c + dt * k1.c};
    const VeS3 k2 = logconf_rhs(q, L, inv_tau);
    return {p.a + 0.5 * dt * (k1.a + k2.a), p.b + 0.5 * dt * (k1.b + k2.b),
            p.c + 0.5 * dt * (k1.c + k2.c)};
}
// e = exp(-dt / tau), evaluated once on the host as the reference's scalar is        :142-147
__device__ __forceinline__ VeS3 relax_exact(const VeS3 &p, double e) {
    VeS3 b = sym_exp(p);
    b.a = 1.0 + (b.a - 1.0) * e;
    b.b = b.b * e;
    b.c = 1.0 + (b.c - 1.0) * e;
    return sym_log(b);
}

enum { VE_LOG = 0, VE_EXP = 1, VE_RELAX = 2 };
template <int FN>
__global__ void __launch_bounds__(VE_T) k_ve_sym_fn(VeIn3 A, long n, double e, VeOut3 O) {
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride) {
        const VeS3 s = ve_load(A, k);
        ve_store(O, k, FN == VE_LOG ? sym_log(s) : FN == VE_EXP ? sym_exp(s) : relax_exact(s, e));
    }
}

__global__ void __launch_bounds__(VE_T) k_ve_logconf_rhs(VeIn3 P, VeIn4 Lp, long n,
                                                         double inv_tau, VeOut3 O) {
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride)
        ve_store(O, k, logconf_rhs(ve_load(P, k), ve_load(Lp, k), inv_tau));
}

// RELAX: the Strang stepper with its two exact half-relaxations (e_half = exp(-(dt / 2) / tau));
// without it the stepper is logconf_step with the inv_tau given -- the explicit step, and the
// Strang step where relax_exact is the identity (tau = inf or dt / 2 == 0, inv_tau = 0 then)
template <bool RELAX>
__global__ void __launch_bounds__(VE_T) k_ve_logconf_steps(VeIn3 P, VeIn4 Lp, long n,
                                                           double inv_tau, double dt,
                                                           double e_half, int nsteps, VeOut3 O) {
    const long stride = (long)gridDim.x * VE_T;
    for (long k = blockIdx.x * (long)VE_T + threadIdx.x; k < n; k += stride) {
        VeS3 p = ve_load(P, k);
        const VeL4 L = ve_load(Lp, k);
        for (int s = 0; s < nsteps; ++s) {
            if (RELAX) p = relax_exact(p, e_half);
            p = logconf_step(p, L, inv_tau, dt);
            if (RELAX) p = relax_exact(p, e_half);
        }
        ve_store(O, k, p);
    }
}

// ------------------------------------------------------------------- reduction ----
// The largest eigenvalue over phi <= 0 and the count of those cells: VL_RB workgroups of VL_T
// threads leave partials in ctx->red, one workgroup folds them (a constant launch shape, so
// the result does not depend on n's split; nanmax: a NaN inside the mask comes out).
constexpr int VL_RB = 256, VL_T = 256;
static_assert(2 * VL_RB <= RED_BLOCKS + 64, "ctx->red holds the partials");
__device__ __forceinline__ void vl_fold(double *smx, double *sct, double &mx, double &ct) {
    smx[threadIdx.x] = mx; sct[threadIdx.x] = ct;
    __syncthreads();
    tree_fold<VL_T>([&](int t, int u) {
        smx[t] = nanmax(smx[t], smx[u]);
        sct[t] = sct[t] + sct[u];
    });
    mx = smx[0]; ct = sct[0];
}
__global__ void __launch_bounds__(VL_T) k_ve_lam_p1(VeIn3 B, const double *__restrict__ phi,
                                                    long n, double *__restrict__ part) {
    __shared__ double smx[VL_T], sct[VL_T];
    double mx = -INFINITY, ct = 0.0;
    for (long k = blockIdx.x * (long)VL_T + threadIdx.x; k < n; k += (long)VL_RB * VL_T)
        if (phi[k] <= 0.0) {
            const VeS3 b = ve_load(B, k);
            const double tr = 0.5 * (b.a + b.c), h = b.a - b.c;
            mx = nanmax(mx, tr + sqrt(nanmax(0.25 * (h * h) + b.b * b.b, 0.0)));
            ct += 1.0;
        }
    vl_fold(smx, sct, mx, ct);
    if (threadIdx.x == 0) { part[blockIdx.x] = mx; part[VL_RB + blockIdx.x] = ct; }
}
__global__ void __launch_bounds__(VL_T) k_ve_lam_p2(const double *__restrict__ part,
                                                    const double *__restrict__ b11, long at,
                                                    double *__restrict__ out3) {
    __shared__ double smx[VL_T], sct[VL_T];
    static_assert(VL_RB == VL_T, "one partial a thread");
    double mx = part[threadIdx.x], ct = part[VL_RB + threadIdx.x];
    vl_fold(smx, sct, mx, ct);
    if (threadIdx.x == 0) { out3[0] = mx; out3[1] = ct; out3[2] = b11[at]; }
}

static int ve_in3(const double *const *p, VeIn3 &o, const char *what) {
    RMT_CHECK(p && p[0] && p[1] && p[2], RMT_EINVAL, what);
    o = {{p[0], p[1], p[2]}};
    return RMT_OK;
}
static int ve_in4(const double *const *p, VeIn4 &o) {
    RMT_CHECK(p && p[0] && p[1] && p[2] && p[3], RMT_EINVAL, "L: four planes (11, 12, 21, 22)");
    o = {{p[0], p[1], p[2], p[3]}};
    return RMT_OK;
}
static int ve_out3(double *const *p, VeOut3 &o) {
    RMT_CHECK(p && p[0] && p[1] && p[2], RMT_EINVAL, "out: three planes (11, 12, 22)");
    o = {{p[0], p[1], p[2]}};
    return RMT_OK;
}
static inline double ve_inv_tau(double tau) { return tau == INFINITY ? 0.0 : 1.0 / tau; }   // :38

}  // namespace rmt
using namespace rmt;

#define VE_LAUNCH(kernel, n) kernel<<<ve_blocks(n), VE_T, 0, ctx->stream>>>

int rmt_ve_launch_shape(long n, int *blocks, int *threads) {
    RMT_CHECK(n >= 1 && blocks && threads, RMT_EINVAL, "rmt_ve_launch_shape: n >= 1");
    *blocks = (int)ve_blocks(n); *threads = VE_T;
    return RMT_OK;
}

int rmt_ve_ucm_rhs(rmt_ctx *ctx, long n, const double *const *b, const double *const *L,
                   double tau, double *const *out) {
    RMT_CHECK(ctx && n >= 1, RMT_EINVAL, "rmt_ve_ucm_rhs: a context and n >= 1");
    VeIn3 B; VeIn4 Lp; VeOut3 O;
    RMT_TRY(ve_in3(b, B, "b: three planes (11, 12, 22)")); RMT_TRY(ve_in4(L, Lp));
    RMT_TRY(ve_out3(out, O));
    VE_LAUNCH(k_ve_ucm_rhs, n)(B, Lp, n, ve_inv_tau(tau), O);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_ve_ucm_steps(rmt_ctx *ctx, long n, const double *const *b, const double *const *L,
                     double tau, double dt, int nsteps, const double *const *track,
                     double *const *out, double *out_err) {
    RMT_CHECK(ctx && n >= 1 && nsteps >= 1, RMT_EINVAL, "rmt_ve_ucm_steps: n, nsteps >= 1");
    RMT_CHECK(!track == !out_err, RMT_EINVAL, "rmt_ve_ucm_steps: track and out_err go together");
    VeIn3 B, T = {}; VeIn4 Lp; VeOut3 O;
    RMT_TRY(ve_in3(b, B, "b: three planes (11, 12, 22)")); RMT_TRY(ve_in4(L, Lp));
    RMT_TRY(ve_out3(out, O));
    if (track) T = {{track[0], track[1], track[2]}};
    VE_LAUNCH(k_ve_ucm_steps, n)(B, Lp, n, ve_inv_tau(tau), dt, nsteps, T, out_err, O);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_ve_stress(rmt_ctx *ctx, long n, const double *const *b, double G,
                  const double *const *bref, double G_inf, double *const *out) {
    RMT_CHECK(ctx && n >= 1, RMT_EINVAL, "rmt_ve_stress: a context and n >= 1");
    VeIn3 B, R = {}; VeOut3 O;
    RMT_TRY(ve_in3(b, B, "b: three planes (11, 12, 22)")); RMT_TRY(ve_out3(out, O));
    const int zener = bref != nullptr && G_inf != 0.0;                                  // :175
    if (zener) RMT_TRY(ve_in3(bref, R, "bref: three planes (11, 12, 22)"));
    VE_LAUNCH(k_ve_stress, n)(B, n, G, R, zener, G_inf, O);
    RMT_LAUNCHED();
    return RMT_OK;
}

template <int FN>
static int ve_sym_fn(rmt_ctx *ctx, long n, const double *const *a, double e, double *const *out) {
    RMT_CHECK(ctx && n >= 1, RMT_EINVAL, "a context and n >= 1");
    VeIn3 A; VeOut3 O;
    RMT_TRY(ve_in3(a, A, "three planes (11, 12, 22)")); RMT_TRY(ve_out3(out, O));
    VE_LAUNCH(k_ve_sym_fn<FN>, n)(A, n, e, O);
    RMT_LAUNCHED();
    return RMT_OK;
}
int rmt_ve_sym_log(rmt_ctx *ctx, long n, const double *const *a, double *const *out) {
    return ve_sym_fn<VE_LOG>(ctx, n, a, 0.0, out);
}
int rmt_ve_sym_exp(rmt_ctx *ctx, long n, const double *const *a, double *const *out) {
    return ve_sym_fn<VE_EXP>(ctx, n, a, 0.0, out);
}

int rmt_ve_logconf_rhs(rmt_ctx *ctx, long n, const double *const *psi, const double *const *L,
                       double tau, double *const *out) {
    RMT_CHECK(ctx && n >= 1, RMT_EINVAL, "rmt_ve_logconf_rhs: a context and n >= 1");
    VeIn3 P; VeIn4 Lp; VeOut3 O;
    RMT_TRY(ve_in3(psi, P, "psi: three planes (11, 12, 22)")); RMT_TRY(ve_in4(L, Lp));
    RMT_TRY(ve_out3(out, O));
    VE_LAUNCH(k_ve_logconf_rhs, n)(P, Lp, n, ve_inv_tau(tau), O);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_ve_relax_exact(rmt_ctx *ctx, long n, const double *const *psi, double tau, double dt,
                       double *const *out) {
    RMT_CHECK(ctx && n >= 1, RMT_EINVAL, "rmt_ve_relax_exact: a context and n >= 1");
    if (tau == INFINITY || dt == 0.0) {                                             // :140-141
        VeIn3 P; VeOut3 O;
        RMT_TRY(ve_in3(psi, P, "psi: three planes (11, 12, 22)")); RMT_TRY(ve_out3(out, O));
        for (int c = 0; c < 3; ++c)
            if (O.p[c] != P.p[c])
                RMT_HIP(hipMemcpyAsync(O.p[c], P.p[c], n * sizeof(double),
                                       hipMemcpyDeviceToDevice, ctx->stream));
        return RMT_OK;
    }
    return ve_sym_fn<VE_RELAX>(ctx, n, psi, std::exp(-dt / tau), out);
}

int rmt_ve_logconf_steps(rmt_ctx *ctx, long n, const double *const *psi, const double *const *L,
                         double tau, double dt, int nsteps, int strang, double *const *out) {
    RMT_CHECK(ctx && n >= 1 && nsteps >= 1, RMT_EINVAL, "rmt_ve_logconf_steps: n, nsteps >= 1");
    VeIn3 P; VeIn4 Lp; VeOut3 O;
    RMT_TRY(ve_in3(psi, P, "psi: three planes (11, 12, 22)")); RMT_TRY(ve_in4(L, Lp));
    RMT_TRY(ve_out3(out, O));
    const double half = 0.5 * dt;                                                   // :161-163
    if (strang && !(tau == INFINITY || half == 0.0))
        VE_LAUNCH(k_ve_logconf_steps<true>, n)(P, Lp, n, 0.0, dt, std::exp(-half / tau), nsteps, O);
    else
        VE_LAUNCH(k_ve_logconf_steps<false>, n)(P, Lp, n, strang ? 0.0 : ve_inv_tau(tau), dt, 1.0,
                                                nsteps, O);
    RMT_LAUNCHED();
    return RMT_OK;
}

int rmt_ve_lam_max(rmt_ctx *ctx, long n, const double *const *b, const double *phi, long at,
                   double *out3) {
    RMT_CHECK(ctx && n >= 1 && phi && out3, RMT_EINVAL, "rmt_ve_lam_max: null argument");
    RMT_CHECK(at >= 0 && at < n, RMT_EINVAL, "rmt_ve_lam_max: `at` is a flat index below n");
    VeIn3 B;
    RMT_TRY(ve_in3(b, B, "b: three planes (11, 12, 22)"));
    k_ve_lam_p1<<<VL_RB, VL_T, 0, ctx->stream>>>(B, phi, n, ctx->red);
    k_ve_lam_p2<<<1, VL_T, 0, ctx->stream>>>(ctx->red, B.p[0], at, out3);
    RMT_LAUNCHED();
    return RMT_OK;
}
