// cg.hpp -- the one device conjugate-gradient solver: scipy.sparse.linalg.cg (scipy 1.15's
// algorithm) with its scalars on the device.  varrho.hip (variable-density projection) and
// imex.hip (MAC Helmholtz solves) bring the operator, the preconditioner and the start; the
// kernels are in cg.hip.  The reduction order and the scalar stages are DESIGN.md's
// "Reduction contract".
#pragma once
#include "rmt_internal.hpp"
#include <cmath>

namespace rmt {

// every reduction launch of the solver, the operator's p.q partials included: this grid fixes
// the summation order
constexpr int CG_BLOCKS = 1024, CG_T = 256;
// scalar slots; cg_final(slot) stores the sum of the partials there and derives that stage's
// scalar: CS_RZ -> beta = rz / rz_prev (iteration > 0), CS_PQ -> alpha = rz / pq,
// CS_RR -> rz_prev = rz
enum { CS_RZ = 0, CS_RZ_PREV = 1, CS_PQ = 2, CS_ALPHA = 3, CS_BETA = 4, CS_RR = 5, CS_N = 8 };
constexpr long CG_WORK = CG_BLOCKS + CS_N;   // doubles of workspace: partials, then scalars

// deterministic block partial of a per-thread sum into part[blockIdx.x] (CG_T threads)
__device__ __forceinline__ void cg_block_sum(double acc, double *part) {
    __shared__ double sh[CG_T];
    sh[threadIdx.x] = acc;
    __syncthreads();
    tree_fold<CG_T>(sh, fold_add());
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

struct CgWork {
    hipStream_t st;
    long n;         // unknowns
    double *part;   // CG_WORK doubles
    double *sc() const { return part + CG_BLOCKS; }
};
int cg_begin(const CgWork &W);                              // zero the partials
int cg_norm2(const CgWork &W, const double *v, double *rr); // *rr = v.v, read back (syncs)
void cg_dot(const CgWork &W, const double *x, const double *y);   // partials of x.y
void cg_final(const CgWork &W, int slot, int it);
void cg_pdir(const CgWork &W, double *p, const double *z, bool first);
void cg_xr(const CgWork &W, double *x, double *r, const double *p, const double *q);
int cg_read_rr(const CgWork &W, double *rr);

// The iterations, from "x, r and rr = r.r are set" on: at most maxiter, stopping before the
// preconditioner once sqrt(rr) < atol; *iters = the iterations run (scipy's callback count).
//   precond(r, &z): z = M r, setting z to where it lives (r itself without one); a status
//   apply(d, q, part): q = A d with CG_BLOCKS partials of d.q into part
template <class Precond, class Apply>
int cg_iterate(const CgWork &W, double *x, double *r, double *d, double *q, double rr,
               double atol, int maxiter, Precond precond, Apply apply, int *iters) {
    int status = RMT_OK, &it = *iters;
    for (it = 0; it < maxiter; ++it) {
        if (std::sqrt(rr) < atol) break;
        const double *z = r;
        if ((status = precond(r, &z))) break;
        cg_dot(W, r, z);
        cg_final(W, CS_RZ, it);
        cg_pdir(W, d, z, it == 0);
        apply(d, q, W.part);
        cg_final(W, CS_PQ, it);
        cg_xr(W, x, r, d, q);
        cg_final(W, CS_RR, it);
        RMT_LAUNCHED();
        if ((status = cg_read_rr(W, &rr))) break;
    }
    return status;
}

}  // namespace rmt
