// dct1.hip -- functions.py:1091-1119 DCT-I Neumann Poisson solve on MI355X.
//
// p = idctn(dctn(rhs, type=1) / eig, type=1) - mean(p).  An unnormalised DCT-I of length
// n is the length-M = 2(n-1) DFT of the even extension [x0 .. x_{n-1}, x_{n-2} .. x1]
// (the construction pocketfft uses inside scipy); that DFT is real, so TWO rows packed as
// the real and imaginary parts of one complex sequence come back separated in Re and Im.
// scipy's inverse DCT-I is the forward one scaled by 1/(2(n-1)) per axis.
//
// Main path (n - 1 < 4096, a product of radices 2..23, 29, 31 -- the last two as matrix-form
// passes, fft_pass_mat): k_dct1 -- one workgroup per row,
// the row's even extension packed as a length-(n-1) complex sequence resident in LDS
// (<= 64 KB, two workgroups per CU), the LDS FFT of fft_lds.hpp,
// then the packed-real split into the DCT-I.  A 2D solve is five launches:
//   rows (x)  ->  transpose  ->  columns: DCT, / eig, inverse DCT, fused  ->  transpose
//   ->  rows (x, inverse, + the row sums of the mean).
// HBM traffic: 10 planes per solve.  Reading the columns in place instead of transposing
// (strided, XCD-grouped workgroups) measured slower: 380 us for the fused column pass
// against 63 + 234 + 43 us with the transposes.  Other sizes: rocFFT R2C rounds.
// An axis with n - 1 odd and a product of pairwise coprime radices 3 .. 13 (n = 4096) runs
// k_dct1s instead of k_dct1 in the same launches: the even-symmetric prime-factor FFT on half
// the row (32 KB, four workgroups per CU), see there.
#include "fft_lds.hpp"
#include "rocfft_util.hpp"

namespace rmt {

constexpr int K1_MAXN = DCT_MAXM / 2;   // k_dct1's complex FFT length (n <= 4097)

// One axis of the LDS path (rows of length n, complex FFT length n - 1)
struct DctAxis {
    int n = 0;
    int rad[16] = {0}, np = 0;       // k_dct1's radices (factor)
    double2 *W = nullptr;            // and per-pass twiddle tables (twiddles())
    // half-row path (k_dct1s, when ns > 0): pairwise coprime radices of n - 1 and the read-out
    // table
    int sym[4] = {0}, ns = 0;
    unsigned short *tab = nullptr;
    bool k4095 = false;              // n = 4096: both kernels' compile-time plan 13, 9, 7, 5
};

struct DctPlan {
    int ny = 0, nx = 0;
    RocfftPlans fft;          // fallback: R2C along x, along y (null on a square grid: [0])
    double *E = nullptr;      // even-extended rows (real)
    double *C = nullptr;      // R2C output (complex, interleaved)
    double *T = nullptr;      // transposed real plane
    double *lamx = nullptr, *lamy = nullptr;
    double dx = 0, dy = 0;
    // LDS FFT path
    bool lds = false;
    int big = 0;              // a radix above 13 present
    int mat = 0;              // a matrix-form radix (29, 31) present
    DctAxis ax[2];            // [0] along x, [1] along y
};

void dct_destroy(DctPlan *P) {
    if (!P) return;
    (void)hipFree(P->E); (void)hipFree(P->C); (void)hipFree(P->T);
    (void)hipFree(P->lamx); (void)hipFree(P->lamy);
    for (DctAxis &A : P->ax) { (void)hipFree(A.W); (void)hipFree(A.tab); }
    delete P;
}

// functions.py:1091-1104: lam = -2 (1 - cos(pi k / (n-1))) / h**2, eig = lam_x + lam_y,
// eig[0,0] = 1.  (h**2 of a numpy float64 scalar is libm pow.)
static void host_lambda(int n, double h, std::vector<double> &lam) {
    lam.resize(n);
    double h2 = std::pow(h, 2.0);
    for (int k = 0; k < n; ++k) lam[k] = -2.0 * (1.0 - std::cos(M_PI * k / (n - 1))) / h2;
}

// The half-row plan of an axis (k_dct1s; tools/dct_sym_model.py): N = n - 1 odd and a product
// of pairwise coprime radices from {13, 11, 9, 7, 5, 3}, in that (pass) order.  4095 gives
// 13, 9, 7, 5; four radices at the most below K1_MAXN.
static bool sym_factor(int N, int *rad, int *np) {
    int n = 0, m = N;
    for (int R : {13, 11, 9, 7, 5, 3})
        if (m % R == 0 && n < 4 && !(R == 3 && N % 9 == 0)) { rad[n++] = R; m /= R; }
    *np = n;
    return N >= 3 && N < K1_MAXN && m == 1;
}
// Its read-out table: the slot that holds C at frequency k (N + 1) / 2 after the in-place
// prime-factor passes, k = 0 .. (N - 1) / 2 (slot(i) = min(i, N - i))
static int sym_table(int N, const int *rad, int np, unsigned short **tab) {
    std::vector<unsigned short> h((N + 1) / 2);
    for (int k = 0; k <= (N - 1) / 2; ++k) {
        const long k2 = (long)k * ((N + 1) / 2) % N;
        long sig = 0;
        for (int q = 0; q < np; ++q) sig += (k2 % rad[q]) * (N / rad[q]);
        sig %= N;
        h[k] = (unsigned short)std::min(sig, N - sig);
    }
    RMT_HIP(hipMalloc(tab, h.size() * sizeof(unsigned short)));
    RMT_UPLOAD(*tab, h.data(), h.size() * sizeof(unsigned short));
    return RMT_OK;
}

// ------------------------------------------------------------- rocFFT fallback --
static int make_r2c(rocfft_plan *plan, size_t M, size_t batch) {
    rocfft_plan_description d = nullptr;
    RMT_TRY(rocfft_ok(rocfft_plan_description_create(&d), "description_create"));
    size_t istr = 1, ostr = 1, idist = M, odist = M / 2 + 1;
    RMT_TRY(rocfft_ok(rocfft_plan_description_set_data_layout(
                          d, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved,
                          nullptr, nullptr, 1, &istr, idist, 1, &ostr, odist), "set_data_layout"));
    int s = rocfft_ok(rocfft_plan_create(plan, rocfft_placement_notinplace,
                                         rocfft_transform_type_real_forward,
                                         rocfft_precision_double, 1, &M, batch, d), "plan_create");
    rocfft_plan_description_destroy(d);
    return s;
}

// E[r][k] = src[r][k] (k < n), src[r][M-k] (n <= k < M): even extension of each row.
__global__ void k_even_ext(const double *__restrict__ src, int rows, int n,
                           double *__restrict__ E) {
    const long M = 2L * (n - 1);
    long q = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (q >= (long)rows * M) return;
    long r = q / M, k = q % M;
    E[q] = src[r * n + (k < n ? k : M - k)];
}

// out[k][r] = scale * Re(C[r][k]) (/ (lamx[k] + lamy[r]) when lam given: the reference's
// eig[kj][ki] = lam_x[ki] + lam_y[kj], with (0,0) -> 1), LDS-tiled transpose.
constexpr int TT = 32;
__global__ void __launch_bounds__(TT * 8) k_real_T(const double *__restrict__ C, int rows, int n,
                                                   double scale, const double *__restrict__ lamr,
                                                   const double *__restrict__ lamk,
                                                   double *__restrict__ out) {
    __shared__ double tile[TT][TT + 1];
    int k0 = blockIdx.x * TT, r0 = blockIdx.y * TT;
    for (int rr = threadIdx.y; rr < TT; rr += 8) {
        int r = r0 + rr, k = k0 + threadIdx.x;
        if (r < rows && k < n) tile[rr][threadIdx.x] = C[2 * ((long)r * n + k)];
    }
    __syncthreads();
    for (int kk = threadIdx.y; kk < TT; kk += 8) {
        int k = k0 + kk, r = r0 + threadIdx.x;
        if (r < rows && k < n) {
            double v = tile[threadIdx.x][kk] * scale;
            if (lamr) {
                // orientation of this round: rows r = x-frequency ki, k = y-frequency kj
                double e = (k == 0 && r == 0) ? 1.0 : lamr[r] + lamk[k];
                v = v / e;
            }
            out[(long)k * rows + r] = v;
        }
    }
}

// One round along the rows of src (rows x n) -> out (n x rows).
static int round_rows(rmt_ctx *ctx, DctPlan *P, rocfft_plan plan, const double *src, int rows,
                      int n, double scale, const double *lamr, const double *lamk, double *out) {
    const long M = 2L * (n - 1);
    k_even_ext<<<grid1d((long)rows * M, 256), 256, 0, ctx->stream>>>(src, rows, n, P->E);
    RMT_LAUNCHED();
    RMT_TRY(P->fft.on(ctx->stream));
    void *in[1] = {P->E}, *o[1] = {P->C};
    RMT_TRY(rocfft_ok(rocfft_execute(plan, in, o, P->fft.info), "execute"));
    dim3 g((n + TT - 1) / TT, (rows + TT - 1) / TT);
    k_real_T<<<g, dim3(TT, 8), 0, ctx->stream>>>(P->C, rows, n, scale, lamr, lamk, out);
    RMT_LAUNCHED();
    return RMT_OK;
}

// ---------------------------------------------------------------- LDS FFT path --
// factor(4095)'s plan (n = 4096): radices 13, 9, 7, 5 (descending), twiddle offsets 0, 12, 116,
// 818 -- the radix-13 butterflies need no twiddles (Ns = 1), the radix-5 pass takes the large
// table
template <int NT>
__device__ __forceinline__ void fft_4095d(double2 *z, const double2 *__restrict__ W) {
    fft_pass_k<13, 1, NT, 4095>(z, W);
    fft_pass_k<9, 13, NT, 4095>(z, W + 12);
    fft_pass_k<7, 117, NT, 4095>(z, W + 116);
    fft_pass_k<5, 819, NT, 4095>(z, W + 818);
}

// The two ends that k_dct1 and k_dct1s share.  The start: only the listed rows (rm_inv: only
// the others)
__device__ __forceinline__ bool row_left_out(const unsigned char *__restrict__ rowmark,
                                             int rm_inv) {
    return rowmark && (rowmark[blockIdx.x] != 0) == (rm_inv != 0);
}
// The end of a row pass: thread tid holds X_k in xa[t] and X_{N-k} in xb[t], k = tid + t NT
// (ALL: for every t; else where k <= N / 2.  ODD: N is odd, so k never meets N - k).  The row
// goes to o scaled; with rs, rs[r] is the sum k_rowsum would take of the row written: the row
// staged in the n doubles d of LDS, 256 strided partials, then the halving tree (ops.hip) --
// one partial per thread at NT = 256, the first 256 threads' otherwise.
template <int NT, int PP, bool ALL, bool ODD>
__device__ __forceinline__ void put_row_sum(const double (&xa)[PP], const double (&xb)[PP],
                                            int tid, int N, int n, double scale, double *o,
                                            double *d, double *rs, int r) {
    static_assert(NT >= 256, "put_row_sum: the row sum is k_rowsum's, 256 partials");
    __shared__ double red[256];
#pragma unroll
    for (int t = 0; t < PP; ++t) {
        const int k = tid + t * NT;
        if (ALL || k <= N / 2) {
            o[k] = xa[t] * scale;
            if (ODD || N - k != k) o[N - k] = xb[t] * scale;
        }
    }
    if (rs) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int k = tid + t * NT;
            if (ALL || k <= N / 2) { d[k] = xa[t] * scale; d[N - k] = xb[t] * scale; }
        }
        __syncthreads();
        if (NT == 256 || tid < 256) {
            double acc = 0.0;
            for (int k = tid; k < n; k += 256) acc += d[k];
            red[tid] = acc;
        }
        __syncthreads();
        tree_fold<256>(red, fold_add(), tid);
        if (tid == 0) rs[r] = red[0];
    }
}

// DCT-I of one real row per workgroup.  The even extension e (length M = 2N, N = n - 1) is
// real, so its length-M DFT -- the unnormalised DCT-I -- comes from ONE length-N complex FFT
// of z_m = e_{2m} + i e_{2m+1} (the packed-real FFT): with Z = FFT_N(z), Z_N = Z_0 and
// W^k = e^{-2 pi i k / M} = c_k - i s_k,
//   X_k     = (S + c_k T - s_k D) / 2,   X_{N-k} = (S - c_k T + s_k D) / 2,
//   S = Re Z_k + Re Z_{N-k},  D = Re Z_k - Re Z_{N-k},  T = Im Z_k + Im Z_{N-k}.
// Read as doubles, z IS e (d[j] = e_j), so packing is the even extension itself.  N complex
// entries = 64 KB for n = 4096: two workgroups share a CU, one's HBM traffic hiding behind
// the other's LDS passes.  SOLVE: rows are x-frequencies kx of the transposed plane; forward
// DCT, / eig (functions.py:1091-1104: lam_x[kx] + lam_y[ky], (0,0) -> 1), inverse DCT.
// (launch bounds: two workgroups per CU -- 4 waves per SIMD at 512 threads, 128 VGPRs)
template <int BIG> struct K1T { static constexpr int T = BIG ? 256 : 512; };

// every load issued before the first LDS write: a dynamic-trip loop here compiled to one
// HBM round trip per iteration (load, wait, write), ~8 serial misses per row
template <int NT>
__device__ __forceinline__ void put_row_even(double *d, int N, const double *__restrict__ x) {
    constexpr int L = (K1_MAXN + NT) / NT;   // j <= N <= K1_MAXN
    double v[L];
#pragma unroll
    for (int t = 0; t < L; ++t) {
        const int j = threadIdx.x + t * NT;
        if (j <= N) v[t] = x[j];
    }
#pragma unroll
    for (int t = 0; t < L; ++t) {
        const int j = threadIdx.x + t * NT;
        if (j <= N) {
            d[j] = v[t];
            if (j >= 1 && j < N) d[2 * N - j] = v[t];
        }
    }
}

// K4095: n = 4096 (compile-time passes, fft_4095d)
template <bool SOLVE, int BIG, bool K4095 = false>
__global__ void __launch_bounds__(K1T<BIG>::T, BIG ? 2 : 4) k_dct1(const double *__restrict__ src,
                                                      double *__restrict__ dst, int rows, int n,
                                                      const double2 *__restrict__ W,
                                                      Radices rd, double scale,
                                                      const double *__restrict__ lamr,
                                                      const double *__restrict__ lamk, int row0,
                                                      double *__restrict__ rs,
                                                      const unsigned char *__restrict__ rowmark,
                                                      int rm_inv = 0) {
    if (row_left_out(rowmark, rm_inv)) return;
    constexpr int NT = K1T<BIG>::T;
    constexpr int PP = (K1_MAXN / 2 + NT - 1) / NT;   // (k, N - k) pairs per thread, N < K1_MAXN
    extern __shared__ double2 z[];
    const int N = K4095 ? 4095 : n - 1, r = blockIdx.x;
    double *d = (double *)z;
    const double2 *Wq0 = W + (N - 1);   // after the N - 1 pass twiddles: W^k, k = 0 .. N
    put_row_even<NT>(d, N, src + (long)r * n);
    // SOLVE runs the transform twice (forward, then inverse on the divided spectrum): one
    // loop, so that the FFT is inlined once
#pragma unroll 1
    for (int it = 0; it < (SOLVE ? 2 : 1); ++it) {
        __syncthreads();
        if constexpr (K4095) fft_4095d<NT>(z, W);
        else fft_lds<BIG, NT, K1_MAXN>(z, N, rd, W, z + N);
        // opaque per iteration: keeps the twiddle / eigenvalue loads below from being hoisted
        // above the FFT (they would hold ~40 registers across it)
        const double2 *Wq = Wq0;
        const double *lr = lamr, *lk = lamk;
        int tid = threadIdx.x;
        asm volatile("" : "+s"(Wq), "+s"(lr), "+s"(lk), "+v"(tid));
        double xa[PP], xb[PP];   // X_k, X_{N-k} for k = tid + t NT <= N / 2
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int k = tid + t * NT;
            if (k <= N / 2) {
                const double2 A = z[k], B = z[k ? N - k : 0], w = Wq[k];
                const double S = A.x + B.x, D = A.x - B.x, T = A.y + B.y;
                const double c = w.x, sn = -w.y;
                xa[t] = 0.5 * (S + c * T - sn * D);
                xb[t] = 0.5 * (S - c * T + sn * D);
            }
        }
        if (SOLVE && it == 0) {
            const int kx = row0 + r;
            __syncthreads();   // every Z read
#pragma unroll
            for (int t = 0; t < PP; ++t) {
                const int k = tid + t * NT;
                if (k <= N / 2) {
                    const double ea = (kx == 0 && k == 0) ? 1.0 : lr[kx] + lk[k];
                    const double ya = xa[t] / ea;
                    d[k] = ya;
                    if (k >= 1) d[2 * N - k] = ya;
                    const int kb = N - k;
                    if (kb != k) {
                        const double yb = xb[t] / (lr[kx] + lk[kb]);
                        d[kb] = yb;
                        if (kb >= 1 && kb < N) d[2 * N - kb] = yb;
                    }
                }
                // one pair's divisions at a time: interleaved, their expansions spill
                __builtin_amdgcn_sched_barrier(0);
            }
            continue;
        }
        put_row_sum<NT, PP, false, false>(xa, xb, tid, N, n, scale, dst + (long)r * n, d, rs, r);
    }
}

// ------------------------------------------------ DCT-I on half the row (k_dct1s) --
// k_dct1 uses that the even extension e is real; this kernel also uses that it is even
// (tools/dct_sym_model.py states the index maps in numpy).  For N = n - 1
// odd, 2N = 2 N is a coprime split (Good-Thomas): the even- and odd-index halves a, b of e,
// indexed by m = j mod N, are real and even, so their length-N DFTs A, B are real and ONE
// complex DFT of c = a + i b gives both:  c_m = (x_m, x_{N-m}) for even m, (x_{N-m}, x_m) for
// odd m, and  X_k = Re C + (-1)^k Im C,  X_{N-k} = Re C - (-1)^k Im C  at  C = C_{k (N+1)/2}.
// c_{N-m} = c_m, and every stage of the transform keeps that symmetry, so LDS holds only
// slot(i) = min(i, N - i), i.e. (N + 1) / 2 complex values: 32 KB for n = 4096.  With N a
// product of pairwise coprime radices the DFT is the prime-factor algorithm in place: radix R
// (s = N / R) transforms the lines (R q + j s) mod N, j < R, with dft<R> and no twiddles; line
// s - q mirrors line q, so q = 0 .. (s - 1) / 2 are computed, and line 0, its own mirror,
// writes k <= (R - 1) / 2.  No twiddle table, no packed-real split; the read-out order is a
// table of 16-bit slots (sym_table).  256 threads per row, four workgroups per CU.
constexpr int K1S_T = 256;
struct SymRad { int R[4]; int n; };

template <int R, int NT, int NMAX>
__device__ __forceinline__ void sym_pass(double2 *z, const int N, const int s) {
    constexpr int LPT = ((NMAX / R + 1) / 2 + NT - 1) / NT;   // lines per thread (max)
    const int nl = (s + 1) / 2;
    // opaque per pass, as in fft_pass
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    double2 v[LPT][R];
#pragma unroll
    for (int b = 0; b < LPT; ++b) {
        const int q = tid + b * NT;
        if (q < nl) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                int i = R * q + j * s;   // < 3 N / 2
                if (i >= N) i -= N;
                v[b][j] = z[min(i, N - i)];
            }
        }
    }
    __syncthreads();
    // (opaque again: the R slot addresses are formed anew, not held across the butterfly)
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int b = 0; b < LPT; ++b) {
        const int q = tid + b * NT;
        if (q < nl) {
            dft<R>(v[b]);
#pragma unroll
            for (int k = 0; k < R; ++k) {
                int i = R * q + k * s;
                if (i >= N) i -= N;
                if (k <= R / 2 || q != 0) z[min(i, N - i)] = v[b][k];
            }
        }
    }
    __syncthreads();
}

// same interface as k_dct1 (rows, SOLVE, row0, scale, rs, rowmark / rm_inv); K4095: the
// n = 4096 plan 13, 9, 7, 5 with constant index math
template <bool SOLVE, bool K4095>
__global__ void __launch_bounds__(K1S_T, 4) k_dct1s(const double *__restrict__ src,
                                                    double *__restrict__ dst, int rows, int n,
                                                    const unsigned short *__restrict__ tab,
                                                    SymRad sr, double scale,
                                                    const double *__restrict__ lamr,
                                                    const double *__restrict__ lamk, int row0,
                                                    double *__restrict__ rs,
                                                    const unsigned char *__restrict__ rowmark,
                                                    int rm_inv = 0) {
    if (row_left_out(rowmark, rm_inv)) return;
    constexpr int NT = K1S_T;
    // slots per thread, (N + 1) / 2 <= K1_MAXN / 2 (K4095: exactly PP each, no guards)
    constexpr int PP = (K1_MAXN / 2 + NT - 1) / NT;
    extern __shared__ double2 z[];
    const int N = K4095 ? 4095 : n - 1, H = N / 2, r = blockIdx.x;
    double *d = (double *)z;
    {
        // every load issued before the first LDS write (put_row_even)
        const double *x = src + (long)r * n;
        double va[PP], vb[PP];
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int m = threadIdx.x + t * NT;
            if (K4095 || m <= H) { va[t] = x[m]; vb[t] = x[N - m]; }
        }
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int m = threadIdx.x + t * NT;
            if (K4095 || m <= H) z[m] = (m & 1) ? make_double2(vb[t], va[t]) : make_double2(va[t], vb[t]);
        }
    }
#pragma unroll 1
    for (int it = 0; it < (SOLVE ? 2 : 1); ++it) {
        __syncthreads();
        if constexpr (K4095) {
            sym_pass<13, NT, 4095>(z, 4095, 315);
            sym_pass<9, NT, 4095>(z, 4095, 455);
            sym_pass<7, NT, 4095>(z, 4095, 585);
            sym_pass<5, NT, 4095>(z, 4095, 819);
        } else {
            for (int q = 0; q < sr.n; ++q) {
                const int s = N / sr.R[q];
                switch (sr.R[q]) {
                    case 3: sym_pass<3, NT, K1_MAXN>(z, N, s); break;
                    case 5: sym_pass<5, NT, K1_MAXN>(z, N, s); break;
                    case 7: sym_pass<7, NT, K1_MAXN>(z, N, s); break;
                    case 9: sym_pass<9, NT, K1_MAXN>(z, N, s); break;
                    case 11: sym_pass<11, NT, K1_MAXN>(z, N, s); break;
                    case 13: sym_pass<13, NT, K1_MAXN>(z, N, s); break;
                }
            }
        }
        // opaque per iteration: the table / eigenvalue loads below, indexed from it, are not
        // hoisted above the passes
        const unsigned short *tb = tab;
        const double *lr = lamr, *lk = lamk;
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        int sl[PP];
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int k = tid + t * NT;
            if (K4095 || k <= H) sl[t] = tb[k];
        }
        double xa[PP], xb[PP];   // X_k, X_{N-k} for k = tid + t NT <= H
#pragma unroll
        for (int t = 0; t < PP; ++t) {
            const int k = tid + t * NT;
            if (K4095 || k <= H) {
                const double2 C = z[sl[t]];
                const double im = (k & 1) ? -C.y : C.y;
                xa[t] = C.x + im;
                xb[t] = C.x - im;
            } else {
                xa[t] = xb[t] = 0.0;   // (defined on every path: not carried round the loop)
            }
        }
        if (SOLVE && it == 0) {
            const int kx = row0 + r;
            const double lx = lr[kx];
#pragma unroll
            for (int t = 0; t < PP; ++t) {
                const int k = tid + t * NT;
                if (K4095 || k <= H) {
                    const double ea = (kx == 0 && k == 0) ? 1.0 : lx + lk[k];
                    xa[t] = xa[t] / ea;
                    xb[t] = xb[t] / (lx + lk[N - k]);
                }
                // one pair's divisions at a time (k_dct1)
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();   // every C read
            // the thread holding X_k and X_{N-k} holds the pair c_k of the inverse transform
#pragma unroll
            for (int t = 0; t < PP; ++t) {
                const int k = tid + t * NT;
                if (K4095 || k <= H) z[k] = (k & 1) ? make_double2(xb[t], xa[t]) : make_double2(xa[t], xb[t]);
            }
            continue;
        }
        put_row_sum<NT, PP, K4095, true>(xa, xb, tid, N, n, scale, dst + (long)r * n, d, rs, r);
    }
}

// The launch tables: [solve][variant] -> kernel and its threads.  dct_pass launches from
// them and dct_plan walks them for the LDS attribute, so a kernel that can be launched
// cannot be missing there.
enum { K1_GENERIC, K1_BIG, K1_4095, K1_VARIANTS };
struct Dct1Kernel { decltype(&k_dct1<false, 0>) fn; int threads; };
struct Dct1sKernel { decltype(&k_dct1s<false, false>) fn; int threads; };
static const Dct1Kernel K_DCT1[2][K1_VARIANTS] = {
    {{k_dct1<false, 0>, K1T<0>::T}, {k_dct1<false, 1>, K1T<1>::T}, {k_dct1<false, 0, true>, K1T<0>::T}},
    {{k_dct1<true, 0>, K1T<0>::T}, {k_dct1<true, 1>, K1T<1>::T}, {k_dct1<true, 0, true>, K1T<0>::T}}};
static const Dct1sKernel K_DCT1S[2][2] = {   // [solve][n == 4096]
    {{k_dct1s<false, false>, K1S_T}, {k_dct1s<false, true>, K1S_T}},
    {{k_dct1s<true, false>, K1S_T}, {k_dct1s<true, true>, K1S_T}}};

int dct_plan(rmt_ctx *ctx, double dx, double dy) {
    DctPlan *P = ctx->dct;
    if (P && P->dx == dx && P->dy == dy) return RMT_OK;
    if (!P) {
        P = ctx->dct = new DctPlan;
        P->ny = ctx->ny; P->nx = ctx->nx;
        DctAxis &X = P->ax[0], &Y = P->ax[1];
        X.n = P->nx; Y.n = P->ny;
        // k_dct1's complex FFT length: N = n - 1 (half the even extension)
        const int Nx = P->nx - 1, Ny = P->ny - 1;
        P->lds = !ctx->opt.dct_rocfft && Nx >= 2 && Ny >= 2 && Nx < K1_MAXN && Ny < K1_MAXN &&
                 factor(Nx, X.rad, &X.np, true) && factor(Ny, Y.rad, &Y.np, true) &&
                 lds_fits(Nx) && lds_fits(Ny);
        P->big = big_radix(X.rad, X.np) || big_radix(Y.rad, Y.np);
        P->mat = mat_radix(X.rad, X.np) || mat_radix(Y.rad, Y.np);
        // (a matrix pass needs a second length-M buffer: both planes within the LDS budget)
        if (P->mat) P->lds = P->lds && lds_fits(2 * Nx + 64) && lds_fits(2 * Ny + 64);
        for (DctAxis &A : P->ax) {
            // dct_sym: an eligible axis of the LDS path runs on half the row (every eligible
            // length also has a k_dct1 plan, so P->lds is decided as before)
            if (!(P->lds && ctx->opt.dct_sym && sym_factor(A.n - 1, A.sym, &A.ns))) A.ns = 0;
            A.k4095 = A.n == 4096;   // factor(4095) and sym_factor(4095): 13, 9, 7, 5
        }
    }
    if (P->lds && !P->T) {
        for (DctAxis &A : P->ax) {
            RMT_TRY(twiddles(A.n - 1, A.rad, A.np, &A.W, true));
            if (A.ns) RMT_TRY(sym_table(A.n - 1, A.sym, A.ns, &A.tab));
        }
        // more than 64 KB of dynamic LDS needs the attribute, on this plan's device
        for (const auto &row : K_DCT1)
            for (const Dct1Kernel &k : row)
                RMT_HIP(hipFuncSetAttribute((const void *)k.fn,
                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)FFT_LDS_MAX));
        for (const auto &row : K_DCT1S)
            for (const Dct1sKernel &k : row)
                RMT_HIP(hipFuncSetAttribute((const void *)k.fn,
                                            hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)FFT_LDS_MAX));
    }
    if (!P->lds && !P->fft.plan[0]) {
        RMT_TRY(rocfft_ready());
        size_t Mx = 2 * (size_t)(P->nx - 1), My = 2 * (size_t)(P->ny - 1);
        RMT_TRY(make_r2c(&P->fft.plan[0], Mx, P->ny));
        if (P->ny != P->nx) RMT_TRY(make_r2c(&P->fft.plan[1], My, P->nx));
        RMT_TRY(P->fft.finish());
        size_t ne = std::max((size_t)P->ny * Mx, (size_t)P->nx * My);
        RMT_HIP(hipMalloc(&P->E, ne * sizeof(double)));
        RMT_HIP(hipMalloc(&P->C, 2 * (size_t)P->ny * P->nx * sizeof(double)));
    }
    if (!P->T) {
        RMT_HIP(hipMalloc(&P->T, (size_t)P->ny * P->nx * sizeof(double)));
        RMT_HIP(hipMalloc(&P->lamx, P->nx * sizeof(double)));
        RMT_HIP(hipMalloc(&P->lamy, P->ny * sizeof(double)));
    }
    std::vector<double> lx, ly;
    host_lambda(P->nx, dx, lx);
    host_lambda(P->ny, dy, ly);
    RMT_UPLOAD(P->lamx, lx.data(), lx.size() * 8);
    RMT_UPLOAD(P->lamy, ly.data(), ly.size() * 8);
    P->dx = dx; P->dy = dy;
    return RMT_OK;
}

// One LDS DCT-I pass over nrows rows of length n (axis 0: n = nx, axis 1: n = ny).  SOLVE
// (axis 1 only): forward, / eig, inverse, with rows = x-frequencies row0 .. row0 + nrows.
// Every kernel gets the same argument list: a plain row pass never reads the eigenvalues or
// row0, and the checks below keep rs and rowmark null on a solve.
int dct_pass(rmt_ctx *ctx, bool solve, int axis, const double *src, double *dst, int nrows,
             int row0, double scale, double *rs, const unsigned char *rowmark, bool unmarked) {
    DctPlan *P = ctx->dct;
    RMT_CHECK(P && P->lds, RMT_ENOTSUP, "dct_pass: no LDS DCT plan for this grid");
    RMT_CHECK(!solve || axis == 1, RMT_EINVAL, "dct_pass: the solve pass runs along y");
    RMT_CHECK(!rs || (!solve && nrows <= ctx->rsum_len), RMT_EINVAL, "dct_pass: row sums");
    RMT_CHECK(!rowmark || (!solve && !rs), RMT_EINVAL, "dct_pass: row marks on a plain row pass");
    if (nrows <= 0) return RMT_OK;
    const DctAxis &A = P->ax[axis != 0];
    const int n = A.n;
    const unsigned g = (unsigned)nrows;   // one row per workgroup
    hipStream_t st = ctx->stream;
    if (A.ns) {
        // this axis runs on half the row (dct_sym): n doubles of LDS
        SymRad sr{};
        for (int k = 0; k < A.ns; ++k) sr.R[k] = A.sym[k];
        sr.n = A.ns;
        const Dct1sKernel &k = K_DCT1S[solve][A.k4095];
        k.fn<<<g, k.threads, (size_t)n * sizeof(double), st>>>(
            src, dst, nrows, n, A.tab, sr, scale, P->lamx, P->lamy, row0, rs, rowmark, unmarked);
    } else {
        // (a matrix-form pass stages a second length-(n - 1) sequence and its R roots after the row)
        const size_t lds = (size_t)(P->mat ? 2 * (n - 1) + 32 : n - 1) * sizeof(double2);
        const Dct1Kernel &k = K_DCT1[solve][P->big ? K1_BIG : A.k4095 ? K1_4095 : K1_GENERIC];
        k.fn<<<g, k.threads, lds, st>>>(src, dst, nrows, n, A.W, radices(A.rad, A.np), scale,
                                        P->lamx, P->lamy, row0, rs, rowmark, unmarked);
    }
    RMT_LAUNCHED();
    return RMT_OK;
}

bool dct_lds_ready(rmt_ctx *ctx) { return ctx->dct && ctx->dct->lds; }

// ------------------------------------------------------------------ transposes --
// out (C x R) = in (R x C) transposed, 64 x 64 tiles through LDS.  rowmark (nullable) with
// mode 1: only the 64-row blocks of in holding no marked row; mode 2: only those holding one
__global__ void __launch_bounds__(256) k_transpose(const double *__restrict__ in, int R, int C,
                                                   double *__restrict__ out,
                                                   const unsigned char *__restrict__ rowmark = nullptr,
                                                   int mode = 0) {
    __shared__ double t[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    if (rowmark) {
        const bool any = __syncthreads_or(threadIdx.x < 64 && r0 + tx < R && rowmark[r0 + tx] != 0);
        if (any != (mode == 2)) return;
    }
    for (int rr = ty; rr < 64; rr += 4) {
        const int r = r0 + rr, c = c0 + tx;
        if (r < R && c < C) t[rr][tx] = in[(long)r * C + c];
    }
    __syncthreads();
    for (int cc = ty; cc < 64; cc += 4) {
        const int c = c0 + cc, r = r0 + tx;
        if (r < R && c < C) out[(long)c * R + r] = t[tx][cc];
    }
}

// k_transpose with 16-B accesses (R, C even, 16-B aligned planes): a lane moves a pair of
// adjacent doubles on both sides, through the same padded 64 x 64 LDS tile
__global__ void __launch_bounds__(256) k_transpose2(const double *__restrict__ in, int R, int C,
                                                    double *__restrict__ out,
                                                    const unsigned char *__restrict__ rowmark,
                                                    int mode) {
    __shared__ double t[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (rowmark) {
        const int l = threadIdx.x & 63;
        const bool any = __syncthreads_or(threadIdx.x < 64 && r0 + l < R && rowmark[r0 + l] != 0);
        if (any != (mode == 2)) return;
    }
    double2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // rows ty + 8k, columns 2tx, 2tx + 1
        const int r = r0 + ty + 8 * k, c = c0 + 2 * tx;
        v[k] = (r < R && c < C) ? *(const double2 *)(in + (long)r * C + c) : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        t[ty + 8 * k][2 * tx] = v[k].x;
        t[ty + 8 * k][2 * tx + 1] = v[k].y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // output row c0 + ty + 8k, columns r0 + 2tx, + 1
        const int c = c0 + ty + 8 * k, r = r0 + 2 * tx;
        if (c < C && r < R)
            *(double2 *)(out + (long)c * R + r) = make_double2(t[2 * tx][ty + 8 * k], t[2 * tx + 1][ty + 8 * k]);
    }
}

void transpose(const rmt_ctx *ctx, hipStream_t st, const double *in, int R, int C, double *out,
               const unsigned char *rowmark, int mode) {
    // transpose2 = 0 (RMT_TRANSPOSE2=0): the 8-B kernel
    if (ctx->opt.transpose2 && R % 2 == 0 && C % 2 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
        k_transpose2<<<dim3((C + 63) / 64, (R + 63) / 64), 256, 0, st>>>(in, R, C, out, rowmark, mode);
    else
        k_transpose<<<dim3((C + 63) / 64, (R + 63) / 64), 256, 0, st>>>(in, R, C, out, rowmark, mode);
}

// ---------------------------------------------------------------------- solves --
static int dct_lds_solve(rmt_ctx *ctx, DctPlan *P, const double *rhs, double *p, double *rs) {
    const int ny = P->ny, nx = P->nx;
    hipStream_t st = ctx->stream;
    // forward along x: p <- DCT_x(rhs) (p doubles as scratch), then T <- p^T (nx x ny)
    RMT_TRY(dct_pass(ctx, false, 0, rhs, p, ny, 0, 1.0));
    transpose(ctx, st, p, ny, nx, P->T);
    // columns: DCT_y, / eig, inverse DCT_y (scaled), in place on T
    RMT_TRY(dct_pass(ctx, true, 1, P->T, P->T, nx, 0, 1.0 / (2.0 * (ny - 1))));
    transpose(ctx, st, P->T, nx, ny, p);
    // inverse along x, in place (+ the row sums of the result)
    RMT_TRY(dct_pass(ctx, false, 0, p, p, ny, 0, 1.0 / (2.0 * (nx - 1)), rs));
    RMT_LAUNCHED();
    return RMT_OK;
}

// the row blocks of pc whose rows are all unmarked are final before the marked rows are
// redone: transposed ahead (beside the extrapolation chain); dct_solve_after_rows with the
// same marks then transposes only the others
int dct_transpose_unmarked(rmt_ctx *ctx, const double *pc, const unsigned char *rowmark) {
    DctPlan *P = ctx->dct;
    RMT_CHECK(P && P->lds && rowmark, RMT_ENOTSUP, "dct_transpose_unmarked: LDS DCT plan needed");
    transpose(ctx, ctx->stream, pc, P->ny, P->nx, P->T, rowmark, 1);
    RMT_LAUNCHED();
    return RMT_OK;
}

int dct_solve_after_rows(rmt_ctx *ctx, double *pc, double *dev_root,
                         const unsigned char *early_marks) {
    DctPlan *P = ctx->dct;
    RMT_CHECK(P && P->lds && P->ny <= ctx->rsum_len, RMT_ENOTSUP,
              "dct_solve_after_rows: LDS DCT plan needed");
    const int ny = P->ny, nx = P->nx;
    transpose(ctx, ctx->stream, pc, ny, nx, P->T, early_marks, early_marks ? 2 : 0);
    RMT_TRY(dct_pass(ctx, true, 1, P->T, P->T, nx, 0, 1.0 / (2.0 * (ny - 1))));
    transpose(ctx, ctx->stream, P->T, nx, ny, pc);
    RMT_TRY(dct_pass(ctx, false, 0, pc, pc, ny, 0, 1.0 / (2.0 * (nx - 1)), ctx->rsum));
    return rowtree_sums(ctx, ny, dev_root);
}

int dct_solve(rmt_ctx *ctx, const double *rhs, double dx, double dy, double *p,
              double *dev_root) {
    RMT_TRY(dct_plan(ctx, dx, dy));
    DctPlan *P = ctx->dct;
    const int ny = P->ny, nx = P->nx;
    if (P->lds) {
        const bool fuse = dev_root && ny <= ctx->rsum_len;
        RMT_TRY(dct_lds_solve(ctx, P, rhs, p, fuse ? ctx->rsum : nullptr));
        if (fuse) return rowtree_sums(ctx, ny, dev_root);
    } else {
        rocfft_plan px = P->fft.plan[0], py = P->fft.plan[1] ? P->fft.plan[1] : px;
        // forward: along x (rows of rhs) -> T[ki][j]; along y -> p[kj][ki] / eig
        RMT_TRY(round_rows(ctx, P, px, rhs, ny, nx, 1.0, nullptr, nullptr, P->T));
        RMT_TRY(round_rows(ctx, P, py, P->T, nx, ny, 1.0, P->lamx, P->lamy, p));
        // inverse: same transform, scaled by 1/(2(n-1)) per axis
        RMT_TRY(round_rows(ctx, P, px, p, ny, nx, 1.0 / (2.0 * (nx - 1)), nullptr, nullptr, P->T));
        RMT_TRY(round_rows(ctx, P, py, P->T, nx, ny, 1.0 / (2.0 * (ny - 1)), nullptr, nullptr, p));
    }
    RMT_TRY(sub_mean_rows(ctx, p, ny, nx));
    if (dev_root) RMT_HIP(hipMemsetAsync(dev_root, 0, sizeof(double), ctx->stream));
    return RMT_OK;
}

}  // namespace rmt
