// extrap.hip -- functions.py:48-163 extrapolate_reference_map on MI355X, exact semantics.
//
// The reference (serial @njit: the prange at :95 runs serially) fits the targets of a layer in
// raster order and marks each accepted target "known" at once (Gauss-Seidel).  Cramer's rule on
// absolute coordinates amplifies rounding, so any reordering moves results far above rounding
// and a parallel fixed-point iteration needs as many sweeps as the dependency depth (DESIGN.md
// §5).  librmt executes the same dependency DAG, just not in one thread:
//
//   1. k_ex_bits / k_ex_dilate (chip-wide, bit planes of 64-cell words): kbits = (phi < 0);
//      cbits = candidates = interior unknown cells within Chebyshev distance max_layers of a
//      known cell (the only cells that can ever become known); K[L] = "known after layer L",
//      initialised to kbits for every L and OR-ed by each fit of layer L into K[L..ML-1].
//   2. k_ex_sweep (one workgroup of EXW waves): work item = (layer L, row j), taken from an LDS
//      ticket counter in order of j + 5L.  A target (L, j, i) reads the 9x9 window around it, so
//      at its fit the serial state is exactly reproduced when
//        - rows j-4..j+4 of layer L-1 are complete (the window and the 3x3 target test see the
//          state at the start of layer L: K[L-1] is final there), and
//        - rows j-1..j-4 of layer L have finished every target at column <= i+4 (the targets
//          before it in raster order that lie in its window); its own row runs in order.
//      Nothing later in raster order can be inside the window yet: row j+r of layer L waits for
//      row j to pass its columns, and layer L+1 waits for layer L.  Every wait is on a lower
//      ticket, so the lowest active ticket always proceeds.  Rows publish progress ("all my
//      targets left of column c are done, and their stores have reached L2") in an LDS ring.
//   Each fit: lanes own window cells.  Before the wait a lane computes its geometry and
//   glibc-exact weight and loads everything already final (static cells, rows below, its own
//   row, and cells of rows above left of that row's progress), so after the wait only the cells
//   that became final during it are loaded (one round trip, usually none).  Then 12 lanes fold
//   the 12 sums of functions.py:128-145 in loop order, every lane runs the 3x3 solve on the
//   broadcast sums, lane 0 writes.
//
// Visibility: bytes written inside the sweep (fitted X values, K words) are stored with plain
// stores / L2 atomics drained by s_waitcnt vmcnt(0) before the LDS progress word is released,
// and read only with sc1 (L2) loads; bytes fixed before the launch use plain loads.
#include "extrap.hpp"
#include <cstring>
#include "exp_glibc.h"

namespace rmt {

constexpr int EXW = 8;                        // waves of the sweep workgroup (2 per SIMD)
constexpr int EX_RING = 1024;                 // progress ring entries (tickets)
constexpr int EX_WIN = 81;                    // 9x9 window
constexpr unsigned EX_DONE = 0x7fffffffu;     // progress of a completed row
constexpr long EX_SPIN_LIMIT = 1L << 25;      // ~1-2 s of polling, then abort (bug guard)

// known bit plane: word (j, w) bit b <=> phi[j, 64w+b] < 0, copied into K[0..ML-1]; row flags
// and the band's row range reset
__global__ void __launch_bounds__(256) k_ex_bits(const double *__restrict__ phi, int ny, int nx,
                                                 int W, int ML, u64 *__restrict__ kbits,
                                                 u64 *__restrict__ K,
                                                 unsigned char *__restrict__ rowcand,
                                                 int *__restrict__ jrange,
                                                 const double *__restrict__ X1,
                                                 const double *__restrict__ X2,
                                                 double *__restrict__ X1o,
                                                 double *__restrict__ X2o, int copy,
                                                 const u64 *__restrict__ kin) {
    const int j = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const long c = (long)j * nx + i;
    const bool in = i < nx;
    // kin: the known plane given directly (slab-decomposed step: gathered bit rows)
    const bool k = in && (kin ? ((kin[(long)j * W + (i >> 6)] >> (i & 63)) & 1) : phi[c] < 0);
    if (in && copy) { X1o[c] = X1[c]; X2o[c] = X2[c]; }
    const u64 m = __ballot(k);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < W) {
        const long wd = (long)j * W + (i >> 6), plane = (long)ny * W;
        kbits[wd] = m;
        for (int L = 0; L < ML; ++L) K[L * plane + wd] = m;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rowcand[j] = 0;
        if (j == 0) { jrange[0] = 0x7fffffff; jrange[1] = -1; }
    }
}

// k_ex_bits when the known plane is given and nothing is copied: one thread per word
__global__ void __launch_bounds__(256) k_ex_bits_w(const u64 *__restrict__ kin, int ny, int W,
                                                   int ML, u64 *__restrict__ kbits,
                                                   u64 *__restrict__ K,
                                                   unsigned char *__restrict__ rowcand,
                                                   int *__restrict__ jrange) {
    const long t = blockIdx.x * 256L + threadIdx.x, plane = (long)ny * W;
    if (t < plane) {
        const u64 m = kin[t];
        kbits[t] = m;
        for (int L = 0; L < ML; ++L) K[L * plane + t] = m;
    }
    if (t < ny) rowcand[t] = 0;
    if (t == 0) { jrange[0] = 0x7fffffff; jrange[1] = -1; }
}

// candidate bit plane: Chebyshev dilation of known by L, minus known, interior cells only
__global__ void __launch_bounds__(256) k_ex_dilate(const u64 *__restrict__ kbits, int ny, int nx,
                                                   int W, int L, u64 *__restrict__ cbits,
                                                   unsigned char *__restrict__ rowcand,
                                                   int *__restrict__ jrange,
                                                   const int *__restrict__ ctl) {
    if (ctl && (!ctl[EXC_FALLBACK] || ctl[EXC_NOOP])) return;   // chain path / no-op call
    const long t = blockIdx.x * 256L + threadIdx.x;
    if (t >= (long)ny * W) return;
    const int j = (int)(t / W), w = (int)(t % W);
    u64 cw = 0;
    const int i0 = 64 * w, lo = max(1, i0) - i0, hi = min(nx - 2, i0 + 63) - i0;
    if (j >= 1 && j <= ny - 2 && hi >= lo) {
        u64 d = 0;
        if (L >= 64) {
            d = ~0ull;   // superset: every interior unknown cell (exact, just more candidates)
        } else {
            for (int jj = max(0, j - L); jj <= min(ny - 1, j + L); ++jj) {
                const u64 *r = kbits + (long)jj * W;
                const u64 a = w > 0 ? r[w - 1] : 0, b = r[w], e = w + 1 < W ? r[w + 1] : 0;
                u64 h = b;
                for (int s = 1; s <= L; ++s)
                    h |= (b << s) | (a >> (64 - s)) | (b >> s) | (e << (64 - s));
                d |= h;
            }
        }
        const u64 cols = (~0ull >> (63 - hi)) & (~0ull << lo);
        cw = d & ~kbits[t] & cols;
    }
    cbits[t] = cw;
    if (cw) {
        rowcand[j] = 1;
        atomicMin(&jrange[0], j);
        atomicMax(&jrange[1], j);
    }
}

// k_ex_none: can ANY first-layer target be accepted when it sees only the original known
// set?  If not, none is accepted in the serial order either (by induction: the first target
// sees exactly that set, is rejected, so the next sees it too ...), the known set never
// grows, every later layer has the same targets and the same fits, and the whole call is
// the identity -- exactly (functions.py:95-161).  This is the N = 8192 case of config 5,
// where det(Aw) ~ 1e-14 < 1e-10 for every fit.  One wave per row;
// the window sums keep the reference's order (raster within the clipped 9x9 window).
// Rows [jb, je) only (the MAC slabs split the candidates by rows; the known plane is whole).
// Each lane builds the candidate mask of one word, the wave then walks the candidate words.
// the no-op test's fit of candidate (j, i) against the original known set: true if accepted
// (the window sums in the reference's order; t: this wave's 6 x 96 LDS rows)
__device__ __forceinline__ bool ex_none_fit(const u64 *__restrict__ kbits, int ny, int nx, int W,
                                            double dx, double dy, double r2, const u64 *tab,
                                            double (*t)[96], int lane, int j, int i) {
    auto K = [&](int jj, int w) -> u64 {
        return (jj < 0 || jj >= ny || w < 0 || w >= W) ? 0 : kbits[(long)jj * W + w];
    };
    const double x0 = dx * i, y0 = dy * j;
    int inc_n = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h, jj = j - 4 + q / 9, ii = i - 4 + q % 9;
        bool inc = false;
        double xi = 0.0, yi = 0.0, w = 0.0;
        if (q < EX_WIN && jj >= 0 && jj < ny && ii >= 0 && ii < nx &&
            ((K(jj, ii >> 6) >> (ii & 63)) & 1)) {
            xi = dx * ii; yi = dy * jj;
            const double ax = xi - x0, ay = yi - y0, d2 = ax * ax + ay * ay;
            if (d2 <= r2) { inc = true; w = exp_glibc_tab(-d2 / r2, tab); }
        }
        inc_n += __popcll(__ballot(inc));
        if (q < 96) {
            const double wa0 = w * 1.0, wa1 = w * xi, wa2 = w * yi;
            t[0][q] = inc ? wa0 * 1.0 : 0.0;  t[1][q] = inc ? wa0 * xi : 0.0;
            t[2][q] = inc ? wa0 * yi : 0.0;   t[3][q] = inc ? wa1 * xi : 0.0;
            t[4][q] = inc ? wa1 * yi : 0.0;   t[5][q] = inc ? wa2 * yi : 0.0;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    double acc = 0.0;
    if (lane < 6)
        for (int q = 0; q < EX_WIN; ++q) acc += t[lane][q];
    __builtin_amdgcn_wave_barrier();
    const double A00 = __shfl(acc, 0), A01 = __shfl(acc, 1), A02 = __shfl(acc, 2);
    const double A11 = __shfl(acc, 3), A12 = __shfl(acc, 4), A22 = __shfl(acc, 5);
    const double M[9] = {A00, A01, A02, A01, A11, A12, A02, A12, A22};
    const double det = (M[0] * (M[4] * M[8] - M[5] * M[7])
                      - M[1] * (M[3] * M[8] - M[5] * M[6])
                      + M[2] * (M[3] * M[7] - M[4] * M[6]));
    return inc_n >= 3 && fabs(det) > 1e-10;
}
// candidate mask of word w0 of row j: unknown interior cells with a known 8-neighbour
__device__ __forceinline__ u64 ex_none_cands(const u64 *__restrict__ kbits, int ny, int nx, int W,
                                             int j, int w0) {
    auto K = [&](int jj, int w) -> u64 {
        return (jj < 0 || jj >= ny || w < 0 || w >= W) ? 0 : kbits[(long)jj * W + w];
    };
    u64 d = 0;
    for (int jj = j - 1; jj <= j + 1; ++jj) {
        const u64 a = K(jj, w0 - 1), b = K(jj, w0), e = K(jj, w0 + 1);
        d |= b | (b << 1) | (a >> 63) | (b >> 1) | (e << 63);
    }
    const int i0 = 64 * w0, lo = max(1, i0) - i0, hi = min(nx - 2, i0 + 63) - i0;
    return hi >= lo ? d & ~K(j, w0) & (~0ull >> (63 - hi)) & (~0ull << lo) : 0;
}
__global__ void __launch_bounds__(256) k_ex_none(const u64 *__restrict__ kbits, int ny, int nx,
                                                 int W, double dx, double dy, double r2,
                                                 int *__restrict__ ctl, int jb, int je) {
    __shared__ double tb[4][6][96];
    __shared__ u64 tab[256];
    for (int s = threadIdx.x; s < 256; s += blockDim.x) tab[s] = kExpTab[s];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // a wave per row, rows strided over the grid (a grid smaller than the rows stops every
    // wave soon after the first fit is found)
    for (int j = jb + blockIdx.x * 4 + wv; j < je && j <= ny - 2; j += gridDim.x * 4) {
    if (j < 1) continue;
    for (int wb = 0; wb < W; wb += 64) {
        if (__hip_atomic_load(ctl + EXC_ANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const int w0 = wb + lane;
        const u64 mine = w0 < W ? ex_none_cands(kbits, ny, nx, W, j, w0) : 0;
        u64 words = __ballot(mine != 0);
        while (words) {
            const int l = __builtin_ctzll(words);
            words &= words - 1;
            u64 cand = __shfl(mine, l);
            const int i0 = 64 * (wb + l);
            while (cand) {
                const int i = i0 + __builtin_ctzll(cand);
                cand &= cand - 1;
                if (ex_none_fit(kbits, ny, nx, W, dx, dy, r2, tab, tb[wv], lane, j, i)) {
                    if (lane == 0) atomicOr(ctl + EXC_ANY, 1);
                    return;
                }
            }
        }
    }
    }
}
// The same test with a fit per wave instead of a row per wave (mac.hip, where no candidate is
// accepted as often as not and the disc's top / bottom rows hold long candidate runs):
// k_ex_cand lists the candidates of rows [jb, je) (a thread per word), k_ex_none_list fits
// them.  Over capacity (cnt > cap), k_ex_none_list runs the row walk above instead.
__global__ void __launch_bounds__(256) k_ex_cand(const u64 *__restrict__ kbits, int ny, int nx,
                                                 int W, int jb, int je, int wb, int we,
                                                 int *__restrict__ list, int cap,
                                                 int *__restrict__ cnt) {
    // words [wb, we) of rows [jb, je)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int j = jb + (int)(t / (we - wb)), w0 = wb + (int)(t % (we - wb)), lane = threadIdx.x & 63;
    u64 m = (j < je && j >= 1 && j <= ny - 2) ? ex_none_cands(kbits, ny, nx, W, j, w0) : 0;
    // one counter update per wave (a single counter: per-word atomics serialise)
    const int c = __popcll(m);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    const int tot = __shfl(incl, 63);
    if (!tot) return;
    int base = 0;
    if (lane == 63) base = atomicAdd(cnt, tot);
    int p = __shfl(base, 63) + incl - c;
    for (; m && p < cap; m &= m - 1, ++p) list[p] = j * nx + 64 * w0 + __builtin_ctzll(m);
}
__global__ void __launch_bounds__(256) k_ex_none_list(const u64 *__restrict__ kbits, int ny,
                                                      int nx, int W, double dx, double dy,
                                                      double r2, int *__restrict__ ctl, int jb,
                                                      int je, const int *__restrict__ list,
                                                      int cap, const int *__restrict__ cnt) {
    __shared__ double tb[4][6][96];
    __shared__ u64 tab[256];
    for (int s = threadIdx.x; s < 256; s += blockDim.x) tab[s] = kExpTab[s];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n = *cnt;
    if (n > cap) {   // (the list overflowed: the row walk of k_ex_none)
        for (int j = jb + blockIdx.x * 4 + wv; j < je && j <= ny - 2; j += gridDim.x * 4) {
            if (j < 1) continue;
            for (int wb = 0; wb < W; wb += 64) {
                if (__hip_atomic_load(ctl + EXC_ANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    return;
                const int w0 = wb + lane;
                const u64 mine = w0 < W ? ex_none_cands(kbits, ny, nx, W, j, w0) : 0;
                u64 words = __ballot(mine != 0);
                while (words) {
                    const int l = __builtin_ctzll(words);
                    words &= words - 1;
                    u64 cand = __shfl(mine, l);
                    const int i0 = 64 * (wb + l);
                    while (cand) {
                        const int i = i0 + __builtin_ctzll(cand);
                        cand &= cand - 1;
                        if (ex_none_fit(kbits, ny, nx, W, dx, dy, r2, tab, tb[wv], lane, j, i)) {
                            if (lane == 0) atomicOr(ctl + EXC_ANY, 1);
                            return;
                        }
                    }
                }
            }
        }
        return;
    }
    for (int q = blockIdx.x * 4 + wv; q < n; q += gridDim.x * 4) {
        if (__hip_atomic_load(ctl + EXC_ANY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        const int c = list[q], j = c / nx, i = c - j * nx;
        if (ex_none_fit(kbits, ny, nx, W, dx, dy, r2, tab, tb[wv], lane, j, i)) {
            if (lane == 0) atomicOr(ctl + EXC_ANY, 1);
            return;
        }
    }
}
__global__ void k_ex_none_fin(int *ctl) {
    if (!ctl[EXC_ANY]) { ctl[EXC_FALLBACK] = 1; ctl[EXC_NOOP] = 1; }
}

// Tiles (MOM_TX x MOM_TY) whose momentum may depend on an extrapolated value (sim.hip runs
// the momentum speculatively, concurrently with the chain, then re-runs these tiles): a tile
// qualifies if the box of `margin` cells around it holds an unknown interior cell and the box
// of margin + ML holds a known one -- every target lies within ML cells of the known set.
// One wave per tile, one box row per lane.
__global__ void __launch_bounds__(256) k_fix_tiles(const u64 *__restrict__ kbits, int ny, int nx,
                                                   int W, int reach, int margin, int tiles_x,
                                                   int ntiles, int *__restrict__ list,
                                                   int *__restrict__ count, int all) {
    const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    if (all) {   // (RMT_FIX_ALL: a test of the tile-list kernels on every tile kind)
        if (lane == 0) list[atomicAdd(count, 1)] = t;
        return;
    }
    const int i0 = (t % tiles_x) * MOM_TX, j0 = (t / tiles_x) * MOM_TY, w0 = i0 >> 6;
    auto cols = [&](int ww, int a, int b) -> u64 {   // bits of word ww for columns [a, b)
        if (ww < 0 || ww >= W) return 0;
        const int lo = max(a - 64 * ww, 0), hi = min(b - 64 * ww, 64);
        if (hi <= lo) return 0;
        const u64 m = hi == 64 ? ~0ull : ((1ull << hi) - 1);
        return m & ~((1ull << lo) - 1);
    };
    bool kn = false, un = false;
    const int j = j0 - reach + lane;   // reach = margin + ML <= 31 rows each side
    if (lane < MOM_TY + 2 * reach && j >= 0 && j < ny) {
        const bool inner = j >= j0 - margin && j < j0 + MOM_TY + margin && j >= 1 && j <= ny - 2;
        for (int d = -1; d <= 1; ++d) {
            const int ww = w0 + d;
            if (ww < 0 || ww >= W) continue;
            const u64 k = kbits[(long)j * W + ww];
            kn |= (k & cols(ww, max(i0 - reach, 0), min(i0 + MOM_TX + reach, nx))) != 0;
            if (inner)
                un |= (~k & cols(ww, max(i0 - margin, 1), min(i0 + MOM_TX + margin, nx - 1))) != 0;
        }
    }
    if (__ballot(kn) && __ballot(un) && lane == 0) list[atomicAdd(count, 1)] = t;
}

__device__ __forceinline__ u64 ld_sc1_u64(const u64 *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1_f64(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 readlane64(u64 v, int l) {
    unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l);
    unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
    u64 b = __double_as_longlong(v);
    return __longlong_as_double((long long)readlane64(b, l));
}

struct ExSweep {
    double *X1e, *X2e;
    const u64 *kbits, *cbits;
    u64 *K;                      // ML planes of ny*W words
    const unsigned char *rowcand;
    const int *jrange;
    int ny, nx, W, ML;
    double dx, dy;
    int *status;   // [0] fitted cells, [1] abort
    const int *ctl;   // chain-path control words (null: no chain path this call)
};

struct ExState {
    u64 *ring;
    int *abort;
    int jlo, jhi, ML;
};

// progress of row j of layer L (EX_DONE if complete or outside the band's rows)
__device__ __forceinline__ unsigned ex_progress(const ExState &S, int L, int j) {
    if (j < S.jlo || j > S.jhi) return EX_DONE;
    const int T = (j + 5 * L - S.jlo) * S.ML + L;
    const u64 e = __hip_atomic_load(&S.ring[T & (EX_RING - 1)], __ATOMIC_ACQUIRE,
                                    __HIP_MEMORY_SCOPE_WORKGROUP);
    const int tag = (int)(e >> 32);
    return tag > T ? EX_DONE : (tag < T ? 0u : (unsigned)e);
}

__device__ __forceinline__ bool ex_spin(const ExState &S, long &spins) {
    if (++spins > EX_SPIN_LIMIT) {
        __hip_atomic_store(S.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return false;
    }
    if ((spins & 63) == 0 &&
        __hip_atomic_load(S.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
        return false;
    __builtin_amdgcn_s_sleep(1);
    return true;
}

__device__ __forceinline__ void ex_publish(const ExState &S, int T, unsigned prog) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's stores reached L2
    __hip_atomic_store(&S.ring[T & (EX_RING - 1)], ((u64)(unsigned)T << 32) | prog,
                       __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A wave's view of the rows around its row j: lane l holds word (wb - 1 + l) of each plane
// (0 outside the grid), so a fit's window masks are read with readlane, not loaded.
struct ExRow {
    u64 ks[9];   // kbits, rows j-4..j+4
    u64 ca[4];   // cbits, rows j-4..j-1 (may become known while this row runs)
    u64 kn[5];   // known: row j = K[L] (start of layer + this row's own fits), rows j+1..j+4 =
                 // K[L-1] (no layer-L fit of those rows lies inside a window of row j yet)
};

// columns cb..cb+8 of a row held one word per lane; la = lane of word cb >> 6, sh = cb & 63
__device__ __forceinline__ unsigned ex_slice(u64 reg, int la, int sh) {
    const u64 lo = readlane64(reg, la), hi = readlane64(reg, la + 1);
    const u64 v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
    return (unsigned)(v & 0x1ff);
}

// 81-bit window mask (bit q = 9 * row + col) as lo (q < 64) / hi (q >= 64)
__device__ __forceinline__ void ex_put(u64 &lo, u64 &hi, int r, unsigned m) {
    const int b = 9 * r;
    if (b + 9 <= 64) lo |= (u64)m << b;
    else if (b < 64) { lo |= (u64)m << b; hi |= (u64)m >> (64 - b); }
    else hi |= (u64)m << (b - 64);
}

constexpr int EXS = 82;   // term buffer row stride (16-B aligned rows)

// diagnostic build (RMT_EX_PROFILE=1): per-phase shader-clock totals, see extrapolate()
constexpr int EX_NPROF = 8;
#define EX_STAMP(k)                                                     \
    if constexpr (PROF) {                                               \
        const long long t_ = __builtin_amdgcn_s_memtime();              \
        prof[k] += t_ - t_last; t_last = t_;                            \
    }

// fit target (j, i) of layer L; returns true if the cell became known
template <bool PROF>
__device__ bool ex_fit(const ExSweep &A, const ExState &S, double *tbuf, const u64 *tab, int L,
                       int j, int i, double r2, int lane, int wb, ExRow &R, bool &ok,
                       long long *prof, long long &t_last) {
    const double x0 = A.dx * i, y0 = A.dy * j;
    const int cb = i - 4, la = (cb >> 6) - wb + 1, sh = cb & 63;
    // static / start-of-layer window masks from the row registers
    u64 KSl = 0, KSh = 0, CAl = 0, CAh = 0, KBl = 0, KBh = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) ex_put(KSl, KSh, r, ex_slice(R.ks[r], la, sh));
#pragma unroll
    for (int r = 0; r < 4; ++r) ex_put(CAl, CAh, r, ex_slice(R.ca[r], la, sh));
#pragma unroll
    for (int r = 0; r < 5; ++r) ex_put(KBl, KBh, r + 4, ex_slice(R.kn[r], la, sh));
    // this lane's cells q = lane and q = lane + 64
    double xi[2], yi[2], w[2], b1[2], b2[2];
    bool maybe[2], kst[2], above[2], below[2];
    long cc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h, jj = j - 4 + q / 9, ii = cb + q % 9;
        const bool in = q < EX_WIN && jj >= 0 && jj < A.ny && ii >= 0 && ii < A.nx;
        cc[h] = in ? (long)jj * A.nx + ii : 0;
        xi[h] = A.dx * ii; yi[h] = A.dy * jj;
        const u64 ksm = h ? KSh : KSl, cam = h ? CAh : CAl, kbm = h ? KBh : KBl;
        kst[h] = (ksm >> lane) & 1;
        above[h] = !kst[h] && ((cam >> lane) & 1);
        below[h] = (kbm >> lane) & 1;
        double d2 = 0.0;
        bool geo = false;
        if (in) {
            const double ax = xi[h] - x0, ay = yi[h] - y0;
            d2 = ax * ax + ay * ay;
            geo = d2 <= r2;
        }
        maybe[h] = geo && (kst[h] || above[h] || below[h]);
        w[h] = maybe[h] ? exp_glibc_tab(-d2 / r2, tab) : 0.0;   // libm exp, bit for bit
        b1[h] = 0.0; b2[h] = 0.0;
    }
    EX_STAMP(1);
    // rows j-1..j-4 of this layer must have passed column i+4
    const unsigned need = (unsigned)(i + 5);
    long spins = 0;
    for (int r = 1; r <= 4; ++r)
        while (ex_progress(S, L, j - r) < need)
            if (!ex_spin(S, spins)) { ok = false; return false; }
    EX_STAMP(2);
    // one round trip: K[L] words of rows j-4..j-1 (lanes 0..7) and every value that may be known
    u64 kw = 0;
    {
        const int r = lane >> 1, jj = j - 4 + r, wd = (cb >> 6) + (lane & 1);
        if (lane < 8 && jj >= 0 && wd >= 0 && wd < A.W)
            kw = ld_sc1_u64(A.K + ((long)L * A.ny + jj) * A.W + wd);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (maybe[h]) {
            if (kst[h]) { b1[h] = A.X1e[cc[h]]; b2[h] = A.X2e[cc[h]]; }
            else { b1[h] = ld_sc1_f64(A.X1e + cc[h]); b2[h] = ld_sc1_f64(A.X2e + cc[h]); }
        }
    u64 KAl = 0, KAh = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const u64 lo = readlane64(kw, 2 * r), hi = readlane64(kw, 2 * r + 1);
        const u64 v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        ex_put(KAl, KAh, r, (unsigned)(v & 0x1ff));
    }
    bool inc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool ka = ((h ? KAh : KAl) >> lane) & 1;
        inc[h] = maybe[h] && (kst[h] || below[h] || (above[h] && ka));
    }
    inc[1] = inc[1] && lane < EX_WIN - 64;
    if constexpr (PROF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    EX_STAMP(3);
    // terms of functions.py:128-145; excluded cells contribute +0.0 (exact: the sums start at
    // +0.0 and never become -0.0)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (h == 1 && lane >= EX_WIN - 64) break;
        const int q = lane + 64 * h;
        double v[12];
        const double wa0 = w[h] * 1.0, wa1 = w[h] * xi[h], wa2 = w[h] * yi[h];
        v[0] = wa0 * b1[h]; v[1] = wa1 * b1[h]; v[2] = wa2 * b1[h];
        v[3] = wa0 * b2[h]; v[4] = wa1 * b2[h]; v[5] = wa2 * b2[h];
        v[6] = wa0 * 1.0; v[7] = wa0 * xi[h]; v[8] = wa0 * yi[h];
        v[9] = wa1 * xi[h]; v[10] = wa1 * yi[h]; v[11] = wa2 * yi[h];
#pragma unroll
        for (int k = 0; k < 12; ++k) tbuf[k * EXS + q] = inc[h] ? v[k] : 0.0;
    }
    const int count = __popcll(__ballot(inc[0])) + __popcll(__ballot(inc[1]));
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    double acc = 0.0;
    if (lane < 12) {
        // functions.py:128-145 loop order; 41 LDS reads issued ahead of the dependent adds
        const double2 *t2 = (const double2 *)(tbuf + lane * EXS);
        double2 t[40];
#pragma unroll
        for (int q2 = 0; q2 < 40; ++q2) t[q2] = t2[q2];
        const double last = tbuf[lane * EXS + 80];
#pragma unroll
        for (int q2 = 0; q2 < 40; ++q2) {
            acc += t[q2].x;
            acc += t[q2].y;
        }
        acc += last;
    }
    __builtin_amdgcn_wave_barrier();
    if constexpr (PROF) asm volatile("" : "+v"(acc));
    EX_STAMP(4);
    if (count < 3) return false;
    const double B10 = readlane_f64(acc, 0), B11 = readlane_f64(acc, 1), B12 = readlane_f64(acc, 2);
    const double B20 = readlane_f64(acc, 3), B21 = readlane_f64(acc, 4), B22 = readlane_f64(acc, 5);
    const double A00 = readlane_f64(acc, 6), A01 = readlane_f64(acc, 7), A02 = readlane_f64(acc, 8);
    const double A11 = readlane_f64(acc, 9), A12 = readlane_f64(acc, 10), A22 = readlane_f64(acc, 11);
    const double M[9] = {A00, A01, A02, A01, A11, A12, A02, A12, A22};
    const double det = (M[0] * (M[4] * M[8] - M[5] * M[7])
                      - M[1] * (M[3] * M[8] - M[5] * M[6])
                      + M[2] * (M[3] * M[7] - M[4] * M[6]));
    if (!(fabs(det) > 1e-10)) return false;
    // utils.py:134-166 fast_solve_3x3, once per right-hand side
    const double inv_det = 1.0 / det;
    double o[2];
    const double bb[2][3] = {{B10, B11, B12}, {B20, B21, B22}};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const double *b = bb[s];
        const double x = (b[0] * (M[4] * M[8] - M[5] * M[7]) -
                          M[1] * (b[1] * M[8] - M[5] * b[2]) +
                          M[2] * (b[1] * M[7] - M[4] * b[2])) * inv_det;
        const double y = (M[0] * (b[1] * M[8] - M[5] * b[2]) -
                          b[0] * (M[3] * M[8] - M[5] * M[6]) +
                          M[2] * (M[3] * b[2] - b[1] * M[6])) * inv_det;
        const double z = (M[0] * (M[4] * b[2] - b[1] * M[7]) -
                          M[1] * (M[3] * b[2] - b[1] * M[6]) +
                          b[0] * (M[3] * M[7] - M[4] * M[6])) * inv_det;
        o[s] = x + y * x0 + z * y0;
    }
    const u64 bit = 1ull << (i & 63);
    if (lane == 0) {
        const long c0 = (long)j * A.nx + i, wd = (long)j * A.W + (i >> 6), plane = (long)A.ny * A.W;
        A.X1e[c0] = o[0];
        A.X2e[c0] = o[1];
        for (int Lp = L; Lp < A.ML; ++Lp)
            __hip_atomic_fetch_or(A.K + Lp * plane + wd, bit, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == (i >> 6) - wb + 1) R.kn[0] |= bit;   // the next targets of this row see it
    if constexpr (PROF) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    EX_STAMP(5);
    return true;
}

template <bool PROF>
__global__ void __launch_bounds__(EXW * 64) k_ex_sweep(ExSweep A, long long *gprof) {
    __shared__ u64 ring[EX_RING];
    __shared__ __attribute__((aligned(16))) double term[EXW][12 * EXS];
    __shared__ u64 tab[256];
    __shared__ int s_ticket, s_abort;
    if (A.ctl && (!A.ctl[EXC_FALLBACK] || A.ctl[EXC_NOOP])) return;   // chain path / no-op
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int s = threadIdx.x; s < EX_RING; s += blockDim.x)
        ring[s] = ((u64)(unsigned)(s - EX_RING) << 32) | EX_DONE;   // virtual done tickets
    for (int s = threadIdx.x; s < 256; s += blockDim.x) tab[s] = kExpTab[s];
    if (threadIdx.x == 0) { s_ticket = 0; s_abort = 0; }
    __syncthreads();
    ExState S{ring, &s_abort, A.jrange[0], A.jrange[1], A.ML};
    if (S.jhi < S.jlo) return;   // no candidates at all
    const int ML = A.ML, W = A.W, ny = A.ny;
    const int ntick = (S.jhi - S.jlo + 1 + 5 * (ML - 1)) * ML;
    double r = 4 * sqrt(A.dx * A.dx + A.dy * A.dy);
    const double r2 = r * r;
    const long plane = (long)ny * W;
    double *tbuf = term[wv];
    int filled = 0;
    bool ok = true;
    long long prof[EX_NPROF] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long t_last = 0;
    if constexpr (PROF) t_last = __builtin_amdgcn_s_memtime();
    for (;;) {
        EX_STAMP(0);
        int T = 0;
        if (lane == 0) T = atomicAdd(&s_ticket, 1);
        T = __builtin_amdgcn_readfirstlane(T);
        if (T >= ntick) break;
        const int L = T % ML, j = S.jlo + T / ML - 5 * L;
        // the ring slot's previous ticket must be complete before it is reused
        long spins = 0;
        const int Tp = T - EX_RING;
        for (;;) {
            const u64 e = __hip_atomic_load(&ring[T & (EX_RING - 1)], __ATOMIC_ACQUIRE,
                                            __HIP_MEMORY_SCOPE_WORKGROUP);
            const int tag = (int)(e >> 32);
            if (tag == Tp && (unsigned)e == EX_DONE) break;
            if (!ex_spin(S, spins)) { ok = false; break; }
        }
        if (!ok) break;
        const bool active = j >= S.jlo && j <= S.jhi && A.rowcand[j];
        if (!active) { ex_publish(S, T, EX_DONE); continue; }
        ex_publish(S, T, 0);
        if constexpr (PROF) prof[7] += 1;
        // rows j-4..j+4 of the previous layer complete
        if (L > 0) {
            for (int rr = -4; rr <= 4 && ok; ++rr)
                while (ex_progress(S, L - 1, j + rr) != EX_DONE)
                    if (!ex_spin(S, spins)) { ok = false; break; }
            if (!ok) break;
        }
        EX_STAMP(6);
        const u64 *Kp = L > 0 ? A.K + (long)(L - 1) * plane : A.kbits, *KL = A.K + (long)L * plane;
        // chunks of 62 words: lanes hold words wb-1 .. wb+62, targets lie in wb .. wb+61
        for (int wb = 0; wb < W && ok; wb += 62) {
            const int wl = wb - 1 + lane;
            const bool wok = wl >= 0 && wl < W;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own earlier K updates landed
            ExRow R;
#pragma unroll
            for (int r = 0; r < 9; ++r) {
                const int jj = j - 4 + r;
                R.ks[r] = wok && jj >= 0 && jj < ny ? A.kbits[(long)jj * W + wl] : 0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jj = j - 4 + r;
                R.ca[r] = wok && jj >= 0 ? A.cbits[(long)jj * W + wl] : 0;
            }
            R.kn[0] = wok ? ld_sc1_u64(KL + (long)j * W + wl) : 0;
#pragma unroll
            for (int r = 1; r < 5; ++r) {
                const int jj = j + r;
                R.kn[r] = wok && jj < ny ? ld_sc1_u64(Kp + (long)jj * W + wl) : 0;
            }
            // targets (functions.py:81-90): candidates unknown at the start of layer L with a
            // known 3x3 neighbour at the start of layer L
            const u64 km1 = wok ? ld_sc1_u64(Kp + (long)(j - 1) * W + wl) : 0;
            const u64 k0 = wok ? ld_sc1_u64(Kp + (long)j * W + wl) : 0;
            const u64 cw = wok ? A.cbits[(long)j * W + wl] : 0;
            const u64 m = km1 | k0 | R.kn[1];
            const u64 a = (u64)__shfl((long long)m, (lane + 63) & 63);
            const u64 e = (u64)__shfl((long long)m, (lane + 1) & 63);
            u64 tw = 0;
            if (lane >= 1 && lane <= 62 && wok)
                tw = cw & ~k0 & (m | (m << 1) | (m >> 1) | (a >> 63) | (e << 63));
            for (u64 lanes = __ballot(tw != 0); lanes && ok; lanes &= lanes - 1) {
                const int src = __builtin_ctzll(lanes);
                for (u64 t = readlane64(tw, src); t && ok; t &= t - 1) {
                    const int i = 64 * (wb - 1 + src) + __builtin_ctzll(t);
                    ex_publish(S, T, (unsigned)i);   // every target left of i is done
                    EX_STAMP(0);
                    if (ex_fit<PROF>(A, S, tbuf, tab, L, j, i, r2, lane, wb, R, ok, prof, t_last))
                        ++filled;
                }
            }
        }
        if (!ok) break;
        ex_publish(S, T, EX_DONE);
    }
    if (lane == 0) {
        atomicAdd(&A.status[0], filled);
        if (!ok) exa_report(A.status, exa_code(EXA_SWEEP, 0, 0));
        if constexpr (PROF)
            for (int k = 0; k < EX_NPROF; ++k) atomicAdd((unsigned long long *)&gprof[k], prof[k]);
    }
}

// byte workspace: both paths' bit planes, the chain path's tables and its record arena
ExWs extrap_layout(void *base, int ny, int nx, int max_layers, size_t *bytes, bool px,
                   bool bump) {
    const int ML = std::max(max_layers, 1), W = (nx + 63) / 64;
    const long plane = (long)ny * W;
    const long interior = (long)std::max(ny - 2, 0) * std::max(nx - 2, 0);
    const long maxt = std::max(64L, std::min((long)ML * interior, 4L * ML * (nx + ny) + 4096));
    char *p = (char *)base;
    size_t o = 0;
    auto take = [&](size_t n) { char *q = p ? p + o : nullptr; o += (n + 255) & ~(size_t)255; return q; };
    ExWs w{};
    w.kbits = (u64 *)take(plane * 8);
    w.cbits = (u64 *)take(plane * 8);
    w.Kold = (u64 *)take(plane * 8 * ML);
    w.rowcand = (unsigned char *)take(ny);
    w.jrange = (int *)take(64);
    w.status = w.jrange + 2;
    w.T = (u64 *)take(plane * 8 * ML);
    w.ACC = (u64 *)take(plane * 8 * ML);
    w.KN = (u64 *)take(plane * 8 * ML);
    w.rowcnt = (int *)take((size_t)ML * ny * 4);
    w.rowoff = (int *)take((size_t)ML * (ny + 1) * 4);
    w.wordoff = (int *)take(plane * 4 * ML);
    w.cbase = (int *)take((size_t)ML * ny * 4);
    w.tcell = (long long *)take(maxt * 8);
    w.recoff = (long long *)take(maxt * 8);
    w.rec_by_chain = (long long *)take(maxt * 8);
    w.chain_of = (int *)take(maxt * 4);
    w.dmark = (int *)take(maxt * 4);
    w.part = (unsigned char *)take(maxt);
    w.loc = (int *)take(maxt * 4);
    w.inv = (int *)take(maxt * 4);
    w.wnext = (int *)take(maxt * 4);
    w.gval = (double *)take(maxt * 16);
    w.rej = (int *)take((size_t)ML * EX_MAXREJ * 4);
    w.ctl = (int *)take(EXC_WORDS * 4);
    // one fixed slot per fit id (no allocation cursor shared by every wave of k_ex_geom) when
    // it fits and bump (rmt_opts::ex_arena_bump) is off; else a bump allocator (~2 KB per record on average at the bench sizes).
    // Offsets are stored in 64-B units.
    const long long cap = (1LL << 31) - 65536;
    w.slots = !bump && maxt * (long long)CH_MAXREC <= cap;
    w.arena_bytes = w.slots ? maxt * (long long)CH_MAXREC : std::min(maxt * 2560LL, cap);
    w.arena = take(w.arena_bytes);
    w.maxt = maxt;
    w.plane = plane;
    w.maxseg = maxt / PX_K + EX_MAXL + 2;
    if (px) {
        w.pns = (int *)take(maxt * 4);
        w.pnd = (int *)take(maxt * 4);
        w.pkey = (int *)take(maxt * PX_S * 4);
        w.pbeta = (double *)take(maxt * PX_S * 8);
        w.pval = (double2 *)take(maxt * 16);
        w.pc = (double2 *)take(maxt * 16);
        w.live = (unsigned char *)take(maxt);
        w.shdr = (int *)take(w.maxseg * PX_H * 4);
        w.sF = (int *)take(w.maxseg * PX_F * 4);
        w.sMT = (double *)take(w.maxseg * PX_F * PX_K * 8);
        w.sNT = (double *)take(w.maxseg * PX_K * PX_K * 8);
        w.sd = (double2 *)take(w.maxseg * PX_K * 16);
        w.spk = (double *)take(w.maxseg * PX_PB * 8);
    }
    if (bytes) *bytes = o;
    return w;
}

// k_ex_none over rows [jb, jb + nrows) of a whole known plane: ctl[EXC_ANY] (zeroed by the
// caller) set iff some first-layer target there is acceptable (MAC slabs, mac.hip)
int extrap_none_rows(rmt_ctx *ctx, const u64 *kbits, int ny, int nx, double dx, double dy,
                     int jb, int je, int *ctl) {
    const double r = 4 * std::sqrt(dx * dx + dy * dy);
    if (je > jb)
        k_ex_none<<<grid1d(je - jb, 4), 256, 0, ctx->stream>>>(kbits, ny, nx, (nx + 63) / 64, dx,
                                                               dy, r * r, ctl, jb, je);
    RMT_LAUNCHED();
    return RMT_OK;
}

size_t extrap_workspace(int ny, int nx, int max_layers, bool px) {
    size_t b = 0;
    extrap_layout(nullptr, ny, nx, max_layers, &b, px);
    return b;
}

// The geometry half of the extrapolation: everything the known plane decides (targets,
// acceptance, chain order, record layouts, the fallback sweep's candidate rows).  In place
// (X1o == X1) with a known plane kin, it reads no map value, so the fused step runs it for the
// next step beside the projection (sim.hip); otherwise (copy or phi-derived known set) the
// map is copied / read here and the call is simply the first half of extrapolate().
int extrap_geometry(rmt_ctx *ctx, const double *X1, const double *X2, const double *phi,
                    double dx, double dy, int max_layers, double *X1o, double *X2o,
                    const u64 *kin, const ExtrapCall &call) {
    const int ny = ctx->ny, nx = ctx->nx;
    const int W = (nx + 63) / 64;
    RMT_CHECK(max_layers > 0 && ny >= 3 && nx >= 3 && ny < (1 << 20) && nx < (1 << 30),
              RMT_EINVAL, "extrapolation grid size");
    const int force = ctx->opt.extrap_mode;
    const bool chain = force != 1 && extrap_chain_supported(ny, nx, max_layers);
    // the parallel mode replaces the chain (never the diagnostic sweep modes)
    const bool par = chain && force == 0 && ctx->opt.extrap_parallel;
    RMT_TRY(ensure_bytes(ctx, extrap_workspace(ny, nx, max_layers, par)));
    const ExWs ws = extrap_layout(ctx->bytes, ny, nx, max_layers, nullptr, par,
                                  ctx->opt.ex_arena_bump);
    ctx->ex_layers = max_layers;
    ctx->ex_chain = chain;
    ctx->ex_par = par;
    const int copy = (X1o != X1) || (X2o != X2);
    if (kin && !copy)
        k_ex_bits_w<<<grid1d((long)ny * W, 256), 256, 0, ctx->stream>>>(
            kin, ny, W, max_layers, ws.kbits, ws.Kold, ws.rowcand, ws.jrange);
    else
        k_ex_bits<<<dim3((nx + 255) / 256, ny), 256, 0, ctx->stream>>>(
            phi, ny, nx, W, max_layers, ws.kbits, ws.Kold, ws.rowcand, ws.jrange, X1, X2, X1o,
            X2o, copy, kin);
    RMT_HIP(hipMemsetAsync(ws.status, 0, 4 * sizeof(int), ctx->stream));
    if (chain) {
        RMT_HIP(hipMemsetAsync(ws.ctl, 0, EXC_WORDS * sizeof(int), ctx->stream));
        if (force == 2) {   // diagnostic: exercise the fallback sweep behind the chain path
            const int one = 1;
            RMT_HIP(hipMemcpyAsync(ws.ctl + EXC_FALLBACK, &one, sizeof(int),
                                   hipMemcpyHostToDevice, ctx->stream));
        }
        // exact shortcut: no target can be accepted -> identity (k_ex_none)
        const double r = 4 * std::sqrt(dx * dx + dy * dy);
        // 64 workgroups: the disc's first rim rows end the search (this runs beside the
        // critical path when sim.hip prepares the next step's geometry early)
        int jb = 0, je = ny;
        if (call.none_rows[1] > call.none_rows[0]) {
            jb = std::max(0, call.none_rows[0]);
            je = std::min(ny, call.none_rows[1]);
        }
        if (call.none_wide && call.cand && je > jb) {
            int *cnt = call.cand + call.cand_cap;
            RMT_HIP(hipMemsetAsync(cnt, 0, sizeof(int), ctx->stream));
            int wb = 0, we = W;
            if (call.none_cols[1] > call.none_cols[0]) {
                wb = std::max(0, call.none_cols[0]);
                we = std::min(W, call.none_cols[1]);
            }
            k_ex_cand<<<grid1d((long)(je - jb) * (we - wb), 256), 256, 0, ctx->stream>>>(
                ws.kbits, ny, nx, W, jb, je, wb, we, call.cand, call.cand_cap, cnt);
            k_ex_none_list<<<1024, 256, 0, ctx->stream>>>(ws.kbits, ny, nx, W, dx, dy, r * r,
                                                           ws.ctl, jb, je, call.cand,
                                                           call.cand_cap, cnt);
        } else {
            k_ex_none<<<call.none_wide ? grid1d(std::max(je - jb, 1), 4)
                                          : std::min<unsigned>(grid1d(ny, 4), 64),
                        256, 0, ctx->stream>>>(
                ws.kbits, ny, nx, W, dx, dy, r * r, ws.ctl, jb, je);
        }
        k_ex_none_fin<<<1, 1, 0, ctx->stream>>>(ws.ctl);
        RMT_LAUNCHED();
        if (call.none_host && force == 0) {
            // the verdict on the host: with no acceptable target every later pass of the call
            // exits at once on the device, so none is launched (extrap_finish: the status words
            // the identity leaves, both zero)
            int any = 1;
            RMT_HIP(hipMemcpyAsync(&any, ws.ctl + EXC_ANY, sizeof(int), hipMemcpyDeviceToHost,
                                   ctx->stream));
            RMT_HIP(hipStreamSynchronize(ctx->stream));
            if (!any) { ctx->ex_noop_skip = true; return RMT_OK; }
        }
        if (par) {
            RMT_TRY(extrap_chain_prep_px(ctx, ws, dx, dy, max_layers));
            RMT_TRY(extrap_par_geometry(ctx, ws, dx, dy, max_layers));
        } else {
            RMT_TRY(extrap_chain_prep(ctx, ws, X1o, X2o, dx, dy, max_layers));
        }
    }
    const int *ctl = chain ? ws.ctl : nullptr;
    k_ex_dilate<<<grid1d((long)ny * W, 256), 256, 0, ctx->stream>>>(
        ws.kbits, ny, nx, W, max_layers, ws.cbits, ws.rowcand, ws.jrange, ctl);
    RMT_LAUNCHED();
    return RMT_OK;
}

// The value half after extrap_geometry (same ctx, same map, same layers): the static terms of
// the records, the fallback sweep (an early exit unless a capacity limit tripped), the chain.
int extrap_finish(rmt_ctx *ctx, double dx, double dy, int max_layers, double *X1o, double *X2o,
                  int *dev_status, const ExtrapCall &call) {
    const int ny = ctx->ny, nx = ctx->nx;
    const int W = (nx + 63) / 64;
    const bool par = ctx->ex_par;
    const ExWs ws = extrap_layout(ctx->bytes, ny, nx, max_layers, nullptr, par,
                                  ctx->opt.ex_arena_bump);
    const int force = ctx->opt.extrap_mode;
    if (ctx->ex_noop_skip) {   // (extrap_geometry: nothing to fit, the map is left as it is)
        ctx->ex_noop_skip = false;
        if (dev_status) RMT_HIP(hipMemsetAsync(dev_status, 0, 2 * sizeof(int), ctx->stream));
        if (call.chain_event) RMT_HIP(hipEventRecord(call.chain_event, ctx->stream));
        return RMT_OK;
    }
    const bool chain = ctx->ex_chain && !par;
    const int *ctl = ctx->ex_chain ? ws.ctl : nullptr;
    if (chain) RMT_TRY(extrap_chain_values(ctx, ws, X1o, X2o, dx, dy, max_layers, call));
    if (ctx->prof && !chain && !par) RMT_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    ExSweep A{X1o, X2o, ws.kbits, ws.cbits, ws.Kold, ws.rowcand, ws.jrange, ny, nx, W,
              max_layers, dx, dy, ws.status, ctl};
    const bool prof = ctx->opt.ex_profile != 0;
    const bool defer = chain && call.sweep_deferred && call.chain_event;
    RMT_CHECK(!defer || !dev_status, RMT_EINVAL,
              "extrap_finish: a deferred sweep leaves the status to the caller");
    if (defer) {
        // the caller's extrap_sweep, beside the chain (both exit at once unless their path
        // is the one the chain prep chose)
    } else if (!prof) {
        k_ex_sweep<false><<<1, EXW * 64, 0, ctx->stream>>>(A, nullptr);
        RMT_LAUNCHED();
    } else {
        // diagnostic: phase totals summed over waves, in shader clocks (s_memtime)
        long long *gp = nullptr, hp[EX_NPROF];
        int hs[2];
        RMT_HIP(hipMalloc(&gp, sizeof(hp)));
        RMT_HIP(hipMemsetAsync(gp, 0, sizeof(hp), ctx->stream));
        hipEvent_t e0, e1;
        RMT_HIP(hipEventCreate(&e0)); RMT_HIP(hipEventCreate(&e1));
        RMT_HIP(hipEventRecord(e0, ctx->stream));
        k_ex_sweep<true><<<1, EXW * 64, 0, ctx->stream>>>(A, gp);
        RMT_LAUNCHED();
        RMT_HIP(hipEventRecord(e1, ctx->stream));
        RMT_HIP(hipMemcpyAsync(hp, gp, sizeof(hp), hipMemcpyDeviceToHost, ctx->stream));
        RMT_HIP(hipMemcpyAsync(hs, ws.status, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
        RMT_HIP(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        RMT_HIP(hipEventElapsedTime(&ms, e0, e1));
        fprintf(stderr, "[ex-prof] %.3f ms fitted=%d rows=%lld | ticket+targets %.3g rowwait %.3g "
                "window %.3g wait %.3g load %.3g sum %.3g solve+store %.3g (Mclk, all waves)\n",
                ms, hs[0], hp[7], hp[0] / 1e6, hp[6] / 1e6, hp[1] / 1e6, hp[2] / 1e6,
                hp[3] / 1e6, hp[4] / 1e6, hp[5] / 1e6);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(gp);
    }
    if (ctx->prof && !chain && !par) RMT_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    // the chain after the sweep: both read the fallback flag the chain prep settled
    if (chain) RMT_TRY(extrap_chain_run(ctx, ws, X1o, X2o, max_layers, call));
    if (par) {
        if (ctx->prof) RMT_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        // the caller's work beside the extrapolation may start now (its combine pass is one
        // workgroup, as the chain)
        if (call.chain_event) RMT_HIP(hipEventRecord(call.chain_event, ctx->stream));
        RMT_TRY(extrap_par_values(ctx, ws, X1o, X2o, max_layers));
        if (ctx->prof) RMT_HIP(hipEventRecord(ctx->ev[3], ctx->stream));
    }
    if (force == 3) {   // diagnostic: report an abort (tests of the callers' error paths)
        const int one = 1;
        RMT_HIP(hipMemcpyAsync(ws.status + 1, &one, sizeof(int), hipMemcpyHostToDevice,
                               ctx->stream));
        RMT_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (dev_status)
        RMT_HIP(hipMemcpyAsync(dev_status, ws.status, 2 * sizeof(int), hipMemcpyDeviceToDevice,
                               ctx->stream));
    if (call.chain_event && !chain && !par)
        RMT_HIP(hipEventRecord(call.chain_event, ctx->stream));
    return RMT_OK;
}

int extrap_sweep(rmt_ctx *ctx, double dx, double dy, int max_layers, double *X1o, double *X2o,
                 hipStream_t s) {
    const int ny = ctx->ny, nx = ctx->nx, W = (nx + 63) / 64;
    RMT_CHECK(ctx->ex_chain && !ctx->ex_par && ctx->ex_layers == max_layers, RMT_EINVAL,
              "extrap_sweep: follows an exact-chain extrap_finish of the same layers");
    const ExWs ws = extrap_layout(ctx->bytes, ny, nx, max_layers, nullptr, false,
                                  ctx->opt.ex_arena_bump);
    ExSweep A{X1o, X2o, ws.kbits, ws.cbits, ws.Kold, ws.rowcand, ws.jrange, ny, nx, W,
              max_layers, dx, dy, ws.status, ws.ctl};
    k_ex_sweep<false><<<1, EXW * 64, 0, s>>>(A, nullptr);
    RMT_LAUNCHED();
    return RMT_OK;
}

const int *extrap_status(rmt_ctx *ctx, int max_layers) {
    return extrap_layout(ctx->bytes, ctx->ny, ctx->nx, max_layers, nullptr, ctx->ex_par,
                         ctx->opt.ex_arena_bump).status;
}

int extrapolate(rmt_ctx *ctx, const double *X1, const double *X2, const double *phi, double dx,
                double dy, int max_layers, double *X1o, double *X2o, int *dev_status,
                const u64 *kin, const ExtrapCall &call) {
    const long n = (long)ctx->ny * ctx->nx;
    if (max_layers <= 0) {
        if (X1o != X1) RMT_HIP(hipMemcpyAsync(X1o, X1, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (X2o != X2) RMT_HIP(hipMemcpyAsync(X2o, X2, n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (dev_status) RMT_HIP(hipMemsetAsync(dev_status, 0, 2 * sizeof(int), ctx->stream));
        return RMT_OK;
    }
    RMT_TRY(extrap_geometry(ctx, X1, X2, phi, dx, dy, max_layers, X1o, X2o, kin, call));
    return extrap_finish(ctx, dx, dy, max_layers, X1o, X2o, dev_status, call);
}

}  // namespace rmt

extern "C" int rmt_extrapolate_reference_map(rmt_ctx *ctx, const double *X1, const double *X2,
                                             const double *phi, double dx, double dy,
                                             int max_layers, double *X1_out, double *X2_out) {
    RMT_CHECK(ctx, RMT_EINVAL, "null ctx");
    // the status words (fitted count, abort) land in the shared scratch; read them back so an
    // aborted chain / sweep is an error, not a partly extrapolated map returned with RMT_OK
    RMT_TRY(rmt::ensure_scratch(ctx, 2 * sizeof(int)));
    int *dst = (int *)ctx->scratch;
    RMT_TRY(rmt::extrapolate(ctx, X1, X2, phi, dx, dy, max_layers, X1_out, X2_out, dst));
    int hs[2] = {0, 0};
    RMT_HIP(hipMemcpyAsync(hs, dst, sizeof(hs), hipMemcpyDeviceToHost, ctx->stream));
    RMT_HIP(hipStreamSynchronize(ctx->stream));
    RMT_CHECK(!hs[1], RMT_EDEVICE, rmt::extrap_abort_detail(hs[1]));
    return RMT_OK;
}

std::string rmt::extrap_abort_detail(int code) {
    std::string m = "extrapolation aborted (progress wait timed out)";
    if (!(code & rmt::EXA_TAG)) return m;   // (a test's forced abort, or an older word)
    static const char *kinds[] = {"?", "chain", "?", "?", "?", "?", "?", "relink order",
                                  "fallback sweep", "parallel combine"};
    const int kind = (code >> 26) & 15, part = (code >> 22) & 15, id = code & 0x3fffff;
    m += ": ";
    m += kind < 10 ? kinds[kind] : "?";
    m += " part " + std::to_string(part) + ", fit ordinal " + std::to_string(id);
    return m;
}

namespace rmt {
int extrap_fix_tiles(rmt_ctx *ctx, int max_layers, int margin, int *list, int *count) {
    const int ny = ctx->ny, nx = ctx->nx, W = (nx + 63) / 64;
    const int tiles_x = (nx + MOM_TX - 1) / MOM_TX, ntiles = tiles_x * ((ny + MOM_TY - 1) / MOM_TY);
    RMT_CHECK(margin + max_layers <= 24 && margin >= 0, RMT_EINVAL, "fix-tile reach");
    const ExWs ws = extrap_layout(ctx->bytes, ny, nx, max_layers, nullptr, false,
                                  ctx->opt.ex_arena_bump);
    // fix_all (RMT_FIX_ALL=1, tests only): list every tile.  The fix-up then re-runs phi, the prep and
    // the four stages on the whole grid from the same inputs: bit-identical to the default if
    // the tile-list kernels are right on interior, edge and domain-boundary tiles alike
    const int all = ctx->opt.fix_all != 0;
    RMT_HIP(hipMemsetAsync(count, 0, sizeof(int), ctx->stream));
    k_fix_tiles<<<grid1d(ntiles, 4), 256, 0, ctx->stream>>>(ws.kbits, ny, nx, W, margin + max_layers,
                                                             margin, tiles_x, ntiles, list, count,
                                                             all);
    RMT_LAUNCHED();
    return RMT_OK;
}
}  // namespace rmt

extern "C" int rmt_extrap_last_path(rmt_ctx *ctx, int *path) {
    RMT_CHECK(ctx && path, RMT_EINVAL, "null argument");
    RMT_CHECK(ctx->bytes, RMT_EINVAL, "no extrapolation has run on this context");
    const rmt::ExWs ws = rmt::extrap_layout(ctx->bytes, ctx->ny, ctx->nx, ctx->ex_layers, nullptr,
                                            false, ctx->opt.ex_arena_bump);
    int fb[2] = {1, 0};   // EXC_FALLBACK, EXC_NOOP
    if (ctx->ex_chain) {
        RMT_HIP(hipMemcpyAsync(&fb[0], ws.ctl + rmt::EXC_FALLBACK, sizeof(int),
                               hipMemcpyDeviceToHost, ctx->stream));
        RMT_HIP(hipMemcpyAsync(&fb[1], ws.ctl + rmt::EXC_NOOP, sizeof(int),
                               hipMemcpyDeviceToHost, ctx->stream));
        RMT_HIP(hipStreamSynchronize(ctx->stream));
    }
    *path = fb[1] ? 2 : fb[0] ? 1 : 0;
    return RMT_OK;
}
