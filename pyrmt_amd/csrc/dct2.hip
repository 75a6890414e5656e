// dct2.hip -- the DCT-II Neumann Poisson solve of the MAC grid (mac.py:104-123) on MI355X.
//
// mac.py:118-123 solves the cell-centred Neumann Poisson problem with an orthonormal
// DCT-II both ways.  The orthonormal scalings cancel between the forward and the inverse
// transform (they are diagonal per axis), so the solve runs the unnormalised pair
// y = D x (y_k = 2 sum_n x_n cos(pi k (2n+1) / 2N)) and x = D^-1 y: equal to rounding,
// like every FFT-based DCT against pocketfft's.  Makhoul's method: D x is 2 Re(w_k V_k),
// V = FFT_N of the even/odd-reordered x, w_k = e^{-i pi k/2N}; D^-1 builds
// V_k = 1/2 conj(w_k) (y_k - i y_{N-k}) and inverts the FFT.  Two rows share one complex
// FFT (their spectra separate by conjugate symmetry), the whole row resident in LDS
// (fft_lds.hpp).
//   MODE 0: forward along rows; 1: forward, / eig ((0,0) -> 0), inverse (fused column
//   solve); 2: inverse along rows.
#include "fft_lds.hpp"

namespace rmt {

// (odd n: the even samples are one more than the odd ones, (n + 1) / 2 of them)
__device__ __forceinline__ int mk_src(int m, int n) { return m < (n + 1) / 2 ? 2 * m : 2 * (n - 1 - m) + 1; }

// factor(8192)'s plan: radices 2, 8, 8, 8, 8 (ascending), twiddle offsets 0, 1, 15, 127, 1023
template <int NT>
__device__ __forceinline__ void fft_8192(double2 *z, const double2 *__restrict__ W) {
    fft_pass_k<2, 1, NT, 8192>(z, W);
    fft_pass_k<8, 2, NT, 8192>(z, W + 1);
    fft_pass_k<8, 16, NT, 8192>(z, W + 15);
    fft_pass_k<8, 128, NT, 8192>(z, W + 127);
    fft_pass_k<8, 1024, NT, 8192>(z, W + 1023);
}

// K8192: n = 8192 (compile-time passes, fft_8192: the same arithmetic as fft_lds)
template <int MODE, int BIG, bool K8192 = false>
__global__ void __launch_bounds__(FftT<BIG>::T) k_dct2(const double *__restrict__ src,
                                                       double *__restrict__ dst, int rows, int n,
                                                       const double2 *__restrict__ W,
                                                       const double2 *__restrict__ Wq, Radices rd,
                                                       const double *__restrict__ lamr,
                                                       const double *__restrict__ lamk, int row0,
                                                       double scale,
                                                       const double *__restrict__ mroot = nullptr,
                                                       double mcount = 1.0) {
    constexpr int DCT_T = FftT<BIG>::T;
    extern __shared__ double2 z[];
    constexpr int PER = DCT_MAXM / DCT_T;
    const int rA = 2 * blockIdx.x, rB = rA + 1, tid = threadIdx.x;
    const bool hasB = rB < rows;
    const double *sa = src + (long)rA * n, *sb = src + (long)rB * n;
    double *da = dst + (long)rA * n, *db = dst + (long)rB * n;
    if constexpr (MODE != 2) {
        // mroot (MODE 0, nullable): the rows' tree root -- x - root / count on the load, the
        // values k_sub_tree_mean would have left in src
        const double mean = mroot ? mroot[0] / mcount : 0.0;
        for (int m = tid; m < n; m += DCT_T) {
            const int q = mk_src(m, n);
            if (mroot) z[m] = make_double2(sa[q] - mean, hasB ? sb[q] - mean : 0.0);
            else z[m] = make_double2(sa[q], hasB ? sb[q] : 0.0);
        }
        __syncthreads();
        if constexpr (K8192) fft_8192<DCT_T>(z, W);
        else fft_lds<BIG, FftT<BIG>::T, DCT_MAXM>(z, n, rd, W);
        double2 y[PER];
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int k = tid + t * DCT_T;
            if (k < n) {
                const double2 Zk = z[k], Zm = z[k ? n - k : 0], w = Wq[k];
                y[t].x = w.x * (Zk.x + Zm.x) - w.y * (Zk.y - Zm.y);
                y[t].y = w.x * (Zk.y + Zm.y) + w.y * (Zk.x - Zm.x);
                if constexpr (MODE == 1) {
                    y[t].x = (row0 + rA == 0 && k == 0) ? 0.0 : y[t].x / (lamr[row0 + rA] + lamk[k]);
                    y[t].y = hasB ? y[t].y / (lamr[row0 + rB] + lamk[k]) : 0.0;
                }
            }
        }
        if constexpr (MODE == 0) {
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const int k = tid + t * DCT_T;
                if (k < n) { da[k] = y[t].x * scale; if (hasB) db[k] = y[t].y * scale; }
            }
            return;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int k = tid + t * DCT_T;
            if (k < n) z[k] = y[t];
        }
    } else {
        for (int k = tid; k < n; k += DCT_T) z[k] = make_double2(sa[k], hasB ? sb[k] : 0.0);
    }
    __syncthreads();
    // inverse: conj(Z), Z_k = V^a_k + i V^b_k, V_k = 1/2 conj(w_k) (y_k - i y_{n-k})
    {
        double2 c[PER];
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int k = tid + t * DCT_T;
            if (k < n) {
                const double2 Y = z[k], Ym = k ? z[n - k] : make_double2(0.0, 0.0);
                const double2 w = Wq[k];   // (cos, -sin); conj(w) = (cos, sin)
                const double cs = w.x, sn = -w.y;
                const double vax = 0.5 * (cs * Y.x + sn * Ym.x), vay = 0.5 * (sn * Y.x - cs * Ym.x);
                const double vbx = 0.5 * (cs * Y.y + sn * Ym.y), vby = 0.5 * (sn * Y.y - cs * Ym.y);
                c[t] = make_double2(vax - vby, -(vay + vbx));
            }
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int k = tid + t * DCT_T;
            if (k < n) z[k] = c[t];
        }
    }
    __syncthreads();
    if constexpr (K8192) fft_8192<DCT_T>(z, W);
    else fft_lds<BIG, FftT<BIG>::T, DCT_MAXM>(z, n, rd, W);
    const double s = scale / n;
    for (int m = tid; m < n; m += DCT_T) {
        const double2 R = z[m];
        const int q = mk_src(m, n);
        da[q] = R.x * s;
        if (hasB) db[q] = -R.y * s;
    }
}

// The launch table: [mode][variant] -> kernel and its threads.  dct2_pass launches from it
// and dct2_plan walks it for the LDS attribute.
enum { K2_GENERIC, K2_BIG, K2_8192, K2_VARIANTS };
struct Dct2Kernel { decltype(&k_dct2<0, 0>) fn; int threads; };
static const Dct2Kernel K_DCT2[3][K2_VARIANTS] = {
    {{k_dct2<0, 0>, FftT<0>::T}, {k_dct2<0, 1>, FftT<1>::T}, {k_dct2<0, 0, true>, FftT<0>::T}},
    {{k_dct2<1, 0>, FftT<0>::T}, {k_dct2<1, 1>, FftT<1>::T}, {k_dct2<1, 0, true>, FftT<0>::T}},
    {{k_dct2<2, 0>, FftT<0>::T}, {k_dct2<2, 1>, FftT<1>::T}, {k_dct2<2, 0, true>, FftT<0>::T}}};

struct Dct2Plan {
    int ny = 0, nx = 0, big = 0;
    double dx = 0, dy = 0;
    int radx[16] = {0}, rady[16] = {0}, npx = 0, npy = 0;
    int kx = K2_GENERIC, ky = K2_GENERIC;   // the axis's column of K_DCT2
    double2 *Wx = nullptr, *Wy = nullptr, *Qx = nullptr, *Qy = nullptr;
    double *lamx = nullptr, *lamy = nullptr, *T = nullptr;
};

void dct2_destroy(Dct2Plan *P) {
    if (!P) return;
    (void)hipFree(P->Wx); (void)hipFree(P->Wy); (void)hipFree(P->Qx); (void)hipFree(P->Qy);
    (void)hipFree(P->lamx); (void)hipFree(P->lamy); (void)hipFree(P->T);
    delete P;
}

static int quarter_twiddles(int n, double2 **Q) {
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<double2> h(n);
    for (int k = 0; k < n; ++k) {
        long double a = PI * k / (2.0L * n);
        h[k] = make_double2((double)cosl(a), (double)-sinl(a));
    }
    RMT_HIP(hipMalloc(Q, n * sizeof(double2)));
    RMT_UPLOAD(*Q, h.data(), n * sizeof(double2));
    return RMT_OK;
}

// mac.py:104-115 eigenvalues per axis: -2 (1 - cos(pi k / n)) / h**2 (h**2: libm pow, as a
// Python float)
static void mac_lambda(int n, double h, std::vector<double> &lam) {
    lam.resize(n);
    const double h2 = std::pow(h, 2.0);
    for (int k = 0; k < n; ++k) lam[k] = -2.0 * (1.0 - std::cos(M_PI * k / n)) / h2;
}

int dct2_plan(rmt_ctx *ctx, int ny, int nx, double dx, double dy) {
    Dct2Plan *P = ctx->dct2;
    if (P && P->ny == ny && P->nx == nx && P->dx == dx && P->dy == dy) return RMT_OK;
    if (P) { dct2_destroy(P); ctx->dct2 = nullptr; }
    P = new Dct2Plan;
    P->ny = ny; P->nx = nx; P->dx = dx; P->dy = dy;
    if (!factor(nx, P->radx, &P->npx) || !factor(ny, P->rady, &P->npy) || !lds_fits(nx) ||
        !lds_fits(ny)) {
        delete P;
        set_error("DCT-II solve: N must be 2 .. 8192 and factor into radices <= 23");
        return RMT_ENOTSUP;
    }
    P->big = big_radix(P->radx, P->npx) || big_radix(P->rady, P->npy);
    // n = 8192: the compile-time plan (factor(8192) is always 2, 8, 8, 8, 8)
    P->kx = nx == 8192 ? K2_8192 : P->big ? K2_BIG : K2_GENERIC;
    P->ky = ny == 8192 ? K2_8192 : P->big ? K2_BIG : K2_GENERIC;
    ctx->dct2 = P;
    RMT_TRY(twiddles(nx, P->radx, P->npx, &P->Wx));
    RMT_TRY(twiddles(ny, P->rady, P->npy, &P->Wy));
    RMT_TRY(quarter_twiddles(nx, &P->Qx));
    RMT_TRY(quarter_twiddles(ny, &P->Qy));
    std::vector<double> lx, ly;
    mac_lambda(nx, dx, lx);
    mac_lambda(ny, dy, ly);
    RMT_HIP(hipMalloc(&P->lamx, nx * sizeof(double)));
    RMT_HIP(hipMalloc(&P->lamy, ny * sizeof(double)));
    RMT_UPLOAD(P->lamx, lx.data(), nx * 8);
    RMT_UPLOAD(P->lamy, ly.data(), ny * 8);
    RMT_HIP(hipMalloc(&P->T, (size_t)nx * ny * sizeof(double)));
    // more than 64 KB of dynamic LDS needs the attribute, on this plan's device
    for (const auto &row : K_DCT2)
        for (const Dct2Kernel &k : row)
            RMT_HIP(hipFuncSetAttribute((const void *)k.fn,
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)FFT_LDS_MAX));
    return RMT_OK;
}

// one DCT-II pass over nrows rows along axis (0: length nx, 1: length ny; MODE 1 needs 1)
int dct2_pass(rmt_ctx *ctx, int mode, int axis, const double *src, double *dst,
                     int nrows, int row0, const double *mroot, double mcount) {
    Dct2Plan *P = ctx->dct2;
    RMT_CHECK(mode >= 0 && mode <= 2, RMT_EINVAL, "dct2_pass: mode 0, 1 or 2");
    RMT_CHECK(!mroot || mode == 0, RMT_EINVAL, "dct2_pass: the mean is taken on a forward pass");
    const int n = axis == 0 ? P->nx : P->ny;
    const Radices rd = axis == 0 ? radices(P->radx, P->npx) : radices(P->rady, P->npy);
    const double2 *W = axis == 0 ? P->Wx : P->Wy, *Q = axis == 0 ? P->Qx : P->Qy;
    const Dct2Kernel &k = K_DCT2[mode][axis == 0 ? P->kx : P->ky];
    k.fn<<<(nrows + 1) / 2, k.threads, (size_t)n * sizeof(double2), ctx->stream>>>(
        src, dst, nrows, n, W, Q, rd, P->lamx, P->lamy, row0, 1.0, mroot, mcount);
    RMT_LAUNCHED();
    return RMT_OK;
}

// the caller's eigenvalues (eig = lam_x[None, :] + lam_y[:, None] of mac.py:104-115)
int dct2_set_lambda(rmt_ctx *ctx, const double *lamx, const double *lamy) {
    Dct2Plan *P = ctx->dct2;
    RMT_CHECK(P, RMT_EINVAL, "dct2_set_lambda: no plan");
    RMT_HIP(hipMemcpyAsync(P->lamx, lamx, P->nx * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipMemcpyAsync(P->lamy, lamy, P->ny * 8, hipMemcpyHostToDevice, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    P->dx = P->dy = -1.0;   // next dct2_plan call recomputes the reference's own values
    return RMT_OK;
}

// mac.py:118-123: p = D^-1 (D rhs / eig), (0,0) -> 0; rhs and p are (ny, nx), may alias
int dct2_solve(rmt_ctx *ctx, const double *rhs, double *p, const double *mroot, double mcount) {
    Dct2Plan *P = ctx->dct2;
    RMT_CHECK(P, RMT_EINVAL, "dct2_solve: no plan");
    const int ny = P->ny, nx = P->nx;
    RMT_TRY(dct2_pass(ctx, 0, 0, rhs, p, ny, 0, mroot, mcount));
    transpose(ctx, ctx->stream, p, ny, nx, P->T);
    RMT_TRY(dct2_pass(ctx, 1, 1, P->T, P->T, nx, 0));
    transpose(ctx, ctx->stream, P->T, nx, ny, p);
    return dct2_pass(ctx, 2, 0, p, p, ny, 0);
}
}  // namespace rmt
