// cg.hip -- kernels and launches of the device conjugate-gradient solver (cg.hpp).
#include "cg.hpp"

namespace rmt {

__global__ void __launch_bounds__(CG_T) k_cg_dot(const double *__restrict__ x,
                                                 const double *__restrict__ y, long n,
                                                 double *__restrict__ part) {
    double acc = 0.0;
    for (long k = blockIdx.x * (long)CG_T + threadIdx.x; k < n; k += (long)gridDim.x * CG_T)
        acc += x[k] * y[k];
    cg_block_sum(acc, part);
}

// the sum of the partials into sc[slot] and the CG scalar that stage derives (scipy 1.15
// cg: beta = rho_cur / rho_prev, alpha = rho_cur / p.q, rho_prev = rho_cur)
__global__ void __launch_bounds__(CG_T) k_cg_final(const double *__restrict__ part, int slot,
                                                   int it, double *__restrict__ sc) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < CG_BLOCKS; k += CG_T) acc += part[k];
    __shared__ double sh[CG_T];
    sh[threadIdx.x] = acc;
    __syncthreads();
    tree_fold<CG_T>(sh, fold_add());
    if (threadIdx.x) return;
    const double s = sh[0];
    sc[slot] = s;
    if (slot == CS_RZ && it > 0) sc[CS_BETA] = s / sc[CS_RZ_PREV];
    if (slot == CS_PQ) sc[CS_ALPHA] = sc[CS_RZ] / s;
    if (slot == CS_RR) sc[CS_RZ_PREV] = sc[CS_RZ];
}

// p = z (first iteration) or p *= beta; p += z
__global__ void k_cg_pdir(double *__restrict__ p, const double *__restrict__ z, long n,
                          const double *__restrict__ sc, int first) {
    const long k = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (k >= n) return;
    p[k] = first ? z[k] : p[k] * sc[CS_BETA] + z[k];
}

// x += alpha p; r -= alpha q; partials of r.r
__global__ void __launch_bounds__(CG_T) k_cg_xr(double *__restrict__ x, double *__restrict__ r,
                                                const double *__restrict__ p,
                                                const double *__restrict__ q, long n,
                                                const double *__restrict__ sc,
                                                double *__restrict__ part) {
    const double al = sc[CS_ALPHA];
    double acc = 0.0;
    for (long k = blockIdx.x * (long)CG_T + threadIdx.x; k < n; k += (long)gridDim.x * CG_T) {
        x[k] = x[k] + al * p[k];
        const double rv = r[k] - al * q[k];
        r[k] = rv;
        acc += rv * rv;
    }
    cg_block_sum(acc, part);
}

int cg_begin(const CgWork &W) {
    RMT_HIP(hipMemsetAsync(W.part, 0, CG_BLOCKS * sizeof(double), W.st));
    return RMT_OK;
}
void cg_dot(const CgWork &W, const double *x, const double *y) {
    k_cg_dot<<<CG_BLOCKS, CG_T, 0, W.st>>>(x, y, W.n, W.part);
}
void cg_final(const CgWork &W, int slot, int it) {
    k_cg_final<<<1, CG_T, 0, W.st>>>(W.part, slot, it, W.sc());
}
void cg_pdir(const CgWork &W, double *p, const double *z, bool first) {
    k_cg_pdir<<<grid1d(W.n, 256), 256, 0, W.st>>>(p, z, W.n, W.sc(), first);
}
void cg_xr(const CgWork &W, double *x, double *r, const double *p, const double *q) {
    k_cg_xr<<<CG_BLOCKS, CG_T, 0, W.st>>>(x, r, p, q, W.n, W.sc(), W.part);
}
int cg_read_rr(const CgWork &W, double *rr) {
    RMT_HIP(hipMemcpyAsync(rr, W.sc() + CS_RR, sizeof(double), hipMemcpyDeviceToHost, W.st));
    RMT_HIP(hipStreamSynchronize(W.st));
    return RMT_OK;
}
int cg_norm2(const CgWork &W, const double *v, double *rr) {
    cg_dot(W, v, v);
    cg_final(W, CS_RR, 0);
    return cg_read_rr(W, rr);
}

}  // namespace rmt
