// fft_lds.hpp -- the FFT of one sequence resident in LDS, shared by the DCT-I (dct1.hip) and
// DCT-II (dct2.hip) solvers: a mixed-radix Stockham FFT, radices grouped into in-register
// composite butterflies of up to 10 (dft<R>), twiddles from a global per-pass table; the host
// helpers that plan it (factor, radices, twiddles).
#pragma once
#include "rmt_internal.hpp"
#include "dft_consts.hpp"
#include <algorithm>
#include <vector>

namespace rmt {

constexpr int DCT_MAXM = 8192;    // complex LDS entries (128 KB)

// Radix plan of a length-M FFT: prime factors (2 .. 23), then 2s grouped into 8 / 4, 3s into
// 9, a leftover 2 with a 5 (10) or a 3 (6): M = 8190 = 2 3^2 5 7 13 runs as 9, 10, 7, 13 --
// four LDS passes instead of six.  mat: also 29 and 31, as matrix-form passes (fft_pass_mat;
// k_dct1 only).  false if a prime factor > 23 (> 31 with mat) remains.
inline bool is_mat_radix(int R) { return R == 29 || R == 31; }
inline bool factor(int M, int *rad, int *np, bool mat = false) {
    if (M < 2 || M > DCT_MAXM) return false;
    int cnt[32] = {0}, m = M;
    for (int q : {2, 3, 5, 7, 11, 13, 17, 19, 23})
        while (m % q == 0) { ++cnt[q]; m /= q; }
    if (mat)
        for (int q : {29, 31})
            while (m % q == 0) { ++cnt[q]; m /= q; }
    if (m != 1) return false;
    int n = 0;
    auto put = [&](int r) { if (n < 16) rad[n++] = r; };
    while (cnt[2] >= 3) { put(8); cnt[2] -= 3; }
    if (cnt[2] == 2) { put(4); cnt[2] = 0; }
    while (cnt[3] >= 2) { put(9); cnt[3] -= 2; }
    if (cnt[2] && cnt[5]) { put(10); --cnt[2]; --cnt[5]; }
    if (cnt[2] && cnt[3]) { put(6); --cnt[2]; --cnt[3]; }
    for (int q : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
        while (cnt[q]) { put(q); --cnt[q]; }
    // ascending: the largest radix runs last, where Ns (the base-twiddle count) is M / R
    std::sort(rad, rad + n);
    // but 4095 (n = 4096) descending, 13, 9, 7, 5: measured faster, and
    // the order fft_4095d is written for
    if (M == 4095) std::reverse(rad, rad + n);
    *np = n;
    return n < 16;
}

inline bool big_radix(const int *rad, int np) {
    for (int k = 0; k < np; ++k) if (rad[k] > 13 && !is_mat_radix(rad[k])) return true;
    return false;
}
inline bool mat_radix(const int *rad, int np) {
    for (int k = 0; k < np; ++k) if (is_mat_radix(rad[k])) return true;
    return false;
}

// Twiddles of the Stockham passes, in pass order: pass (R, Ns) holds e^{-2 pi i k r / (Ns R)}
// at [(r - 1) Ns + k], r = 1 .. R-1, k < Ns (M - 1 entries in all, L2-resident: every
// workgroup reads the same table), from long double, exact where k r / (Ns R) is a multiple
// of 1/4.  post: then k_dct1's packed-real split factors e^{-2 pi i k / (2M)}, k = 0 .. M.
inline double2 unit_root(long t, long L) {
    const long double PI = 3.141592653589793238462643383279502884L;
    t %= L;
    if ((4 * t) % L == 0) {
        const int e = (int)(4 * t / L);
        const double c[4] = {1.0, 0.0, -1.0, 0.0}, sn[4] = {0.0, 1.0, 0.0, -1.0};
        return make_double2(c[e], -sn[e]);
    }
    const long double a = 2.0L * PI * t / L;
    return make_double2((double)cosl(a), (double)-sinl(a));
}
inline int twiddles(int M, const int *rad, int np, double2 **W, bool post = false) {
    std::vector<double2> h;
    h.reserve(2 * (size_t)M + 2);
    int Ns = 1;
    for (int q = 0; q < np; ++q) {
        const int R = rad[q], L = Ns * R;
        for (int r = 1; r < R; ++r)
            for (int k = 0; k < Ns; ++k) h.push_back(unit_root((long)k * r, L));
        Ns = L;
    }
    if (post)
        for (long k = 0; k <= M; ++k) h.push_back(unit_root(k, 2L * M));
    h.push_back(make_double2(1.0, 0.0));
    RMT_HIP(hipMalloc(W, h.size() * sizeof(double2)));
    RMT_UPLOAD(*W, h.data(), h.size() * sizeof(double2));
    return RMT_OK;
}

// LDS budget of one FFT workgroup: the length-M sequence + 4 KB static
constexpr size_t FFT_LDS_MAX = 160 * 1024 - 4096;
inline bool lds_fits(int M) { return (size_t)M * sizeof(double2) <= FFT_LDS_MAX; }

// Threads per workgroup: 1024 (16 waves, 128 VGPRs) for radices up to 13; 512 when a radix
// 17 / 19 / 23 pass is in the plan (its butterfly alone holds ~45 complex values).
template <int BIG> struct FftT { static constexpr int T = BIG ? 512 : 1024; };

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(__builtin_fma(a.x, b.x, -a.y * b.y), __builtin_fma(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// a * e^{-2 pi i t / R}, t a constant after unrolling (exact for multiples of R / 4)
template <int R>
__device__ __forceinline__ double2 wmul(double2 a, int t) {
    t %= R;
    if (t == 0) return a;
    if (4 * t == R) return make_double2(a.y, -a.x);
    if (2 * t == R) return make_double2(-a.x, -a.y);
    if (4 * t == 3 * R) return make_double2(-a.y, a.x);
    const double c = Rc<R>::c[t], sn = Rc<R>::s[t];
    return make_double2(__builtin_fma(a.x, c, a.y * sn), __builtin_fma(a.y, c, -(a.x * sn)));
}

constexpr bool is_prime(int R) {
    for (int d = 2; d * d <= R; ++d) if (R % d == 0) return false;
    return R >= 2;
}
// first factor of a composite radix: 8 = 2 x 4, 9 = 3 x 3, 10 = 2 x 5, 6 = 2 x 3, 4 = 2 x 2
constexpr int split(int R) { return R % 2 == 0 ? 2 : 3; }

// forward DFT of length R in registers (e^{-2 pi i n k / R}), constants from dft_consts.hpp
template <int R>
__device__ __forceinline__ void dft(double2 *v) {
    if constexpr (R == 2) {
        const double2 a = v[0], b = v[1];
        v[0] = cadd(a, b); v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        const double2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
        const double2 t2 = cadd(v[1], v[3]), t3 = csub(v[1], v[3]);
        v[0] = cadd(t0, t2); v[2] = csub(t0, t2);
        v[1] = make_double2(t1.x + t3.y, t1.y - t3.x);   // t1 - i t3
        v[3] = make_double2(t1.x - t3.y, t1.y + t3.x);   // t1 + i t3
    } else if constexpr (is_prime(R)) {
        // odd prime: X_m = A_m -/+ i S_m from the symmetric / antisymmetric input pairs
        constexpr int K = (R - 1) / 2;
        double2 a[K], b[K];
        double2 x0 = v[0];
#pragma unroll
        for (int j = 1; j <= K; ++j) {
            a[j - 1] = cadd(v[j], v[R - j]);
            b[j - 1] = csub(v[j], v[R - j]);
            x0 = cadd(x0, a[j - 1]);
        }
#pragma unroll
        for (int m = 1; m <= K; ++m) {
            double2 A = v[0], S = make_double2(0.0, 0.0);
#pragma unroll
            for (int j = 1; j <= K; ++j) {
                const double c = Rc<R>::c[(j * m) % R], sn = Rc<R>::s[(j * m) % R];
                A.x = __builtin_fma(a[j - 1].x, c, A.x);
                A.y = __builtin_fma(a[j - 1].y, c, A.y);
                S.x = __builtin_fma(b[j - 1].x, sn, S.x);
                S.y = __builtin_fma(b[j - 1].y, sn, S.y);
            }
            v[m] = make_double2(A.x + S.y, A.y - S.x);        // A - i S
            v[R - m] = make_double2(A.x - S.y, A.y + S.x);    // A + i S
        }
        v[0] = x0;
    } else {
        // R = A B: n = B n1 + n2, k = k1 + A k2; DFT_A over n1, twiddle w_R^{n2 k1}, DFT_B
        constexpr int A = split(R), B = R / A;
        double2 y[R];
#pragma unroll
        for (int n2 = 0; n2 < B; ++n2) {
            double2 t[A];
#pragma unroll
            for (int n1 = 0; n1 < A; ++n1) t[n1] = v[B * n1 + n2];
            dft<A>(t);
#pragma unroll
            for (int k1 = 0; k1 < A; ++k1) y[n2 * A + k1] = wmul<R>(t[k1], n2 * k1);
        }
#pragma unroll
        for (int k1 = 0; k1 < A; ++k1) {
            double2 t[B];
#pragma unroll
            for (int n2 = 0; n2 < B; ++n2) t[n2] = y[n2 * A + k1];
            dft<B>(t);
#pragma unroll
            for (int k2 = 0; k2 < B; ++k2) v[k1 + A * k2] = t[k2];
        }
    }
}

// Per pass: radix, Ns (product of the earlier radices), 1/Ns for divide-free index math, and
// the offset of the pass's twiddles in the table
struct Pass { int R, Ns; float inv; int tw; };
struct Radices { Pass p[16]; int n; };

inline Radices radices(const int *rad, int np) {
    Radices rd{};
    int Ns = 1, off = 0;
    for (int k = 0; k < np; ++k) {
        rd.p[k] = Pass{rad[k], Ns, (float)(1.0 / Ns), off};
        off += (rad[k] - 1) * Ns;
        Ns *= rad[k];
    }
    rd.n = np;
    return rd;
}

// one Stockham pass of radix R over z[0..M): load every butterfly's twiddles (global table,
// issued first) and inputs, twiddle them -> barrier -> DFT_R -> write -> barrier
template <int R, int NT, int MAXN>
__device__ __forceinline__ void fft_pass(double2 *z, int M, const Pass &ps,
                                         const double2 *__restrict__ tw) {
    constexpr int BPT = (MAXN / R + NT - 1) / NT;      // butterflies per thread (max)
    const int nb = M / R, Ns = ps.Ns;
    // opaque per pass: the per-thread addresses below are not hoisted out of a caller's loop
    // (k_dct1's two transforms), where they would hold registers across every pass
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    double2 v[BPT][R];
    int o[BPT];
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = tid + b * NT;
        if (j < nb) {
            int g = (int)((float)j * ps.inv), k = j - g * Ns;   // j = g Ns + k
            if (k < 0) { --g; k += Ns; } else if (k >= Ns) { ++g; k -= Ns; }
            o[b] = g * Ns * R + k;
            double2 w[R - 1];
            if (Ns > 1) {
                const double2 *t = tw + ps.tw + k;
#pragma unroll
                for (int r = 1; r < R; ++r) w[r - 1] = t[(r - 1) * Ns];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) v[b][r] = z[j + r * nb];
            if (Ns > 1)
#pragma unroll
                for (int r = 1; r < R; ++r) v[b][r] = cmul(v[b][r], w[r - 1]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = tid + b * NT;
        if (j < nb) {
            dft<R>(v[b]);
#pragma unroll
            for (int r = 0; r < R; ++r) z[o[b] + r * Ns] = v[b][r];
        }
    }
    __syncthreads();
}

// A Stockham pass of an odd prime radix R too large for one butterfly per thread (29, 31:
// the radix-31 pass of M = 1023 has 33 butterflies, and a register butterfly holds 31 complex
// values), in matrix form: every (butterfly, input) pair stages its twiddled input in t, then
// every (butterfly, output pair m / R - m) forms dft<R>'s sums A_m, S_m from them -- the same
// operations in the same order as dft<R>, spread over the workgroup.  t: M + R complex LDS
// entries after z (the R roots of unity at t + M).
template <int R, int NT>
__device__ void fft_pass_mat(double2 *z, int M, const Pass &ps, const double2 *__restrict__ tw,
                             double2 *t) {
    constexpr int K = (R - 1) / 2;
    const int nb = M / R, Ns = ps.Ns;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    double2 *cs = t + M;
    if (tid < R) cs[tid] = make_double2(Rc<R>::c[tid], Rc<R>::s[tid]);
    for (int q = tid; q < nb * R; q += NT) {
        const int j = q / R, r = q - j * R;
        double2 v = z[j + r * nb];
        if (Ns > 1 && r > 0) {
            const int k = j % Ns;
            v = cmul(v, tw[ps.tw + (r - 1) * Ns + k]);
        }
        t[q] = v;
    }
    __syncthreads();
    for (int q = tid; q < nb * (K + 1); q += NT) {
        const int j = q / (K + 1), m = q - j * (K + 1);
        const double2 *v = t + j * R;
        const int g = j / Ns, k = j - g * Ns, o = g * Ns * R + k;
        if (m == 0) {
            double2 x0 = v[0];
            for (int i = 1; i <= K; ++i) x0 = cadd(x0, cadd(v[i], v[R - i]));
            z[o] = x0;
        } else {
            double2 A = v[0], S = make_double2(0.0, 0.0);
            int e = 0;
            for (int i = 1; i <= K; ++i) {
                e += m;
                if (e >= R) e -= R;   // (i m) mod R
                const double2 a = cadd(v[i], v[R - i]), b = csub(v[i], v[R - i]), w = cs[e];
                A.x = __builtin_fma(a.x, w.x, A.x);
                A.y = __builtin_fma(a.y, w.x, A.y);
                S.x = __builtin_fma(b.x, w.y, S.x);
                S.y = __builtin_fma(b.y, w.y, S.y);
            }
            z[o + m * Ns] = make_double2(A.x + S.y, A.y - S.x);         // A - i S
            z[o + (R - m) * Ns] = make_double2(A.x - S.y, A.y + S.x);   // A + i S
        }
    }
    __syncthreads();
}

// the radix passes of rd over z[0..M), M <= MAXN, NT threads (scr: fft_pass_mat's buffer)
template <int BIG, int NT, int MAXN>
__device__ void fft_lds(double2 *z, int M, const Radices &rd, const double2 *__restrict__ tw,
                        double2 *scr = nullptr) {
    for (int q = 0; q < rd.n; ++q) {
        const Pass &ps = rd.p[q];
        switch (ps.R) {
            case 2: fft_pass<2, NT, MAXN>(z, M, ps, tw); break;
            case 3: fft_pass<3, NT, MAXN>(z, M, ps, tw); break;
            case 4: fft_pass<4, NT, MAXN>(z, M, ps, tw); break;
            case 5: fft_pass<5, NT, MAXN>(z, M, ps, tw); break;
            case 6: fft_pass<6, NT, MAXN>(z, M, ps, tw); break;
            case 7: fft_pass<7, NT, MAXN>(z, M, ps, tw); break;
            case 8: fft_pass<8, NT, MAXN>(z, M, ps, tw); break;
            case 9: fft_pass<9, NT, MAXN>(z, M, ps, tw); break;
            case 10: fft_pass<10, NT, MAXN>(z, M, ps, tw); break;
            case 11: fft_pass<11, NT, MAXN>(z, M, ps, tw); break;
            case 13: fft_pass<13, NT, MAXN>(z, M, ps, tw); break;
            case 29: fft_pass_mat<29, NT>(z, M, ps, tw, scr); break;
            case 31: fft_pass_mat<31, NT>(z, M, ps, tw, scr); break;
            default:
                if constexpr (BIG) {
                    switch (ps.R) {
                        case 17: fft_pass<17, NT, MAXN>(z, M, ps, tw); break;
                        case 19: fft_pass<19, NT, MAXN>(z, M, ps, tw); break;
                        case 23: fft_pass<23, NT, MAXN>(z, M, ps, tw); break;
                    }
                }
        }
    }
}

// The same Stockham pass with the radix, Ns and length known at compile time (the n = 4096
// and n = 8192 plans, fft_4095d and fft_8192): constant index math, no pass switch, the same
// arithmetic in the same order as fft_pass (bit-identical results)
template <int R, int NS, int NT, int M>
__device__ __forceinline__ void fft_pass_k(double2 *z, const double2 *__restrict__ tw) {
    constexpr int NB = M / R, BPT = (NB + NT - 1) / NT;
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    double2 v[BPT][R];
    int o[BPT];
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = tid + b * NT;
        if (j < NB) {
            const int g = j / NS, k = j - g * NS;
            o[b] = g * NS * R + k;
            double2 w[R - 1];
            if constexpr (NS > 1) {
#pragma unroll
                for (int r = 1; r < R; ++r) w[r - 1] = tw[(r - 1) * NS + k];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) v[b][r] = z[j + r * NB];
            if constexpr (NS > 1) {
#pragma unroll
                for (int r = 1; r < R; ++r) v[b][r] = cmul(v[b][r], w[r - 1]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int j = tid + b * NT;
        if (j < NB) {
            dft<R>(v[b]);
#pragma unroll
            for (int r = 0; r < R; ++r) z[o[b] + r * NS] = v[b][r];
        }
    }
    __syncthreads();
}

}  // namespace rmt
