/*
 * rmt.h -- C ABI of librmt, the MI355X-native 2D Reference Map Technique (RMT) time step.
 *
 * This is the drop-in boundary for pyRMT's per-step hot path.  The
 * reference has no native library: its operator surface is the set of module-level
 * Python functions re-exported by pyRMT/__init__.py:1-57, called by the benchmark loop
 * bodies (e.g. benchmarks/soft_disc_in_lid_driven.py:206-235).  Each entry point below
 * replaces one of those functions (cited per entry); pyrmt_amd/functions.py binds them
 * with ctypes under the reference names and signatures.
 *
 * Conventions
 *   - Fields are float64, C-contiguous, shape (ny, nx), element [j*nx + i] (j <-> y).
 *   - Every array argument is a DEVICE pointer (hipMalloc / torch.cuda memory) on the
 *     context's device.  Calls are stream-ordered on the context stream and return once
 *     enqueued, except where a host result is returned (documented per call).
 *   - The caller allocates and frees every I/O buffer.  The context owns scratch space,
 *     FFT plans and the step state of an rmt_sim.
 *   - Errors: every call returns an rmt_status; rmt_last_error() describes the last
 *     failure on the calling thread.  The Python shim maps RMT_ENONFINITE to
 *     FloatingPointError and RMT_EINVAL to ValueError, like the reference
 *     (functions.py:524-526, :539-542).
 *   - Velocity BCs and level-set shapes cross as enums + parameters instead of the
 *     reference's Python callables (functions.py:946-947, :1366-1367).
 *   - Not re-entrant per context.
 */
#ifndef RMT_H
#define RMT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RMT_OK = 0,
    RMT_EINVAL = 1,      /* bad argument (unknown scheme / bc / shape, bad size)   */
    RMT_ENONFINITE = 2,  /* non-finite velocity fed to advection                  */
    RMT_EDEVICE = 3,     /* HIP / rocFFT failure                                   */
    RMT_ENOTSUP = 4,     /* valid in the reference but outside this build's path   */
    RMT_ENOMEM = 5
} rmt_status;

/* Velocity boundary conditions (benchmarks/common.py:27-50). */
typedef enum {
    RMT_BC_NONE = 0,          /* identity                                            */
    RMT_BC_NOSLIP_LID = 1,    /* no_slip_lid_bc: walls 0, top row u = lid, corners 0  */
    RMT_BC_FREESLIP_BOX = 2,  /* free_slip_box_bc: normal 0, tangential copied        */
    RMT_BC_PERIODIC = 3       /* overlap grid: last column / row copy column / row 0  */
} rmt_bc_kind;

/* Reference-map advection schemes (functions.py:501-542). */
typedef enum {
    RMT_SCHEME_SEMILAGRANGIAN = 0,  /* advect_semilagrangian_rk4 (bilinear)            */
    RMT_SCHEME_WENO5 = 1,           /* advect_weno5_rk3                               */
    RMT_SCHEME_CENTRAL2 = 2,        /* advect_central2_rk3                            */
    RMT_SCHEME_CONSERVATIVE = 3,    /* advect_conservative_rk3 (Jain 2019 eq. 26)      */
    RMT_SCHEME_SEMILAGRANGIAN_CUBIC = 4 /* advect_semilagrangian_cubic_rk4 (bicubic)  */
} rmt_scheme;

typedef struct rmt_ctx rmt_ctx;

const char *rmt_last_error(void);
int rmt_version(void);

/* Context: one device, one stream, one grid shape.  stream may be NULL (null stream)
 * or a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  ny, nx >= 2; the
 * collocated operators (5-point-wide stencils) are only defined on ny, nx >= 5 -- a smaller
 * context serves only the DCT-II Neumann solve (rmt_mac_solve_poisson_neumann,
 * rmt_selftest_dct2_rows) and, from 3 x 3, the periodic FFT solve. */
int rmt_ctx_create(int ny, int nx, int device, void *stream, rmt_ctx **out);
int rmt_ctx_set_stream(rmt_ctx *ctx, void *stream);
int rmt_ctx_destroy(rmt_ctx *ctx);
int rmt_ctx_sync(rmt_ctx *ctx);
/* HIP-event kernel timers on the ctx stream: after each momentum / extrapolation call,
 * ms2[0] = the four RK4 stage kernels of the last momentum call, ms2[1] = the last
 * extrapolation chain (0 if none was recorded).  Blocks until the events complete. */
int rmt_ctx_set_profiling(rmt_ctx *ctx, int on);
int rmt_ctx_kernel_ms(rmt_ctx *ctx, double *ms2);
/* Per-context implementation switches (bit-identical alternatives of the schedule and the
 * kernels, for A/B measurements and the regression tests): each starts from its environment
 * variable, read at rmt_ctx_create and nowhere else -- a variable changed after the library
 * was loaded is seen by the contexts created afterwards.  Names: ext_events, ex_arena_bump, ex_profile, fix_all,
 * dct_rocfft, transpose2, sim_hiprio, sim_sync, early_geometry, early_transpose, fused_fluid,
 * no_overlap, side_tail, par_overlap, fused_fixprep, merged_join, test_delay_side,
 * test_delay_main, chain_cols, chain_layer_groups, chain_waves (8 or 16 waves per chain
 * workgroup; any other value: RMT_EINVAL), edge_slots, edge_stream, sl_phi,
 * mac_boxes, skip_marked_rows, tail_stream, diag_first, mac_noop_host, mac_face_sl,
 * mac_m2_bound, diag_seg, sl_zero_flags, macp_fused (rmt_mac_per_steps' explicit step: the
 * predictor and the divergence in one kernel, same bits), dct_sym (read when the context's DCT
 * plan is made, at its first solve; it chooses another FFT of the same DCT-I, equal to
 * rounding, not bit for bit), and the test-only test_delay_geo / test_nowait_drop (a slab's
 * early geometry delayed; a dropped geometry not waited for).
 * Four select a path and not merely a schedule (a value outside the range: RMT_EINVAL):
 *   extrap_mode (no variable) 0: geometry-first chain path, row-ticket sweep when its capacity
 *     limits are exceeded; 1: sweep only; 2: the chain path's pre-passes, then the sweep forced;
 *     3: mode 0, then the abort status is raised (exercises the callers' error paths).
 *   extrap_parallel (0 / 1, RMT_EXTRAP_PARALLEL) every fit of functions.py:95-161 -- the same
 *     targets, acceptance, weights and raster-order known sets -- evaluated as the weighted
 *     least-squares plane in offsets from the target and the layer solved as one sparse
 *     triangular system by segments (extrap_par.hip), instead of the exact raster-order chain.
 *     Not bit-exact: each fit differs from the reference by the reference's own rounding of
 *     Cramer's rule on absolute coordinates (~1e-7 at N = 4096, the size of 1-ulp weight
 *     noise).  A sim or slab schedules its step for the value it finds.
 *   momentum_mode (RMT_MOM_UNFUSED non-zero gives 2) 0: one LDS-tiled kernel per RK4 stage;
 *     2: unfused per-cell passes.  Bit-identical results in both.
 *   list_blocks (>= 1, RMT_LIST_BLOCKS) the most workgroups of a launch over a device-side
 *     tile list; same bits at any value.
 * Set them before creating a sim or slab on the context (sim_hiprio is read at
 * rmt_sim_create); a change ends a carried step state.  Unknown name: RMT_EINVAL. */
int rmt_ctx_set_option(rmt_ctx *ctx, const char *name, int value);
int rmt_ctx_get_option(rmt_ctx *ctx, const char *name, int *value);

/* ---- finite-difference helpers (pyRMT/utils.py) ----------------------------------- */
/* utils.py:4-14 grad_central_x_2nd / utils.py:16-25 grad_central_y_2nd */
int rmt_grad_x_2nd(rmt_ctx *ctx, const double *f, double h, double *out);
int rmt_grad_y_2nd(rmt_ctx *ctx, const double *f, double h, double *out);
/* utils.py:61-114 diff_upwind_3rd (axis 1 = x, 0 = y) */
int rmt_diff_upwind_3rd(rmt_ctx *ctx, const double *f, const double *vel, double h, int axis,
                        double *out);

/* ---- interpolation / reference-map transport (interpolators.py, functions.py) ------ */
/* interpolators.py:4-61 bilinear_interpolate: u is (ny, nx) of the ctx grid, nq queries. */
int rmt_bilinear_interpolate(rmt_ctx *ctx, const double *u, const double *xq, const double *yq,
                             long nq, double dx, double dy, double *out);
/* functions.py:194-227 advect_semilagrangian_rk4 */
int rmt_advect_sl_rk4(rmt_ctx *ctx, const double *q, const double *a, const double *b,
                      const double *X, const double *Y, double dt, double dx, double dy,
                      double *out);
/* functions.py:321-393 _weno5_rhs and functions.py:396-415 advect_weno5_rk3 */
int rmt_weno5_rhs(rmt_ctx *ctx, const double *q, const double *a, const double *b, double dx,
                  double dy, const double *phi, double w_cut, double *rhs);
int rmt_advect_weno5_rk3(rmt_ctx *ctx, const double *q, const double *a, const double *b,
                         double dx, double dy, double dt, const double *phi, double w_cut,
                         double *out);
/* functions.py:524-526 guard: sets *finite (host) to 1 if every a, b is finite.  Blocks. */
/* functions.py:420-495 _central2_rhs / _conservative_rhs and the SSP-RK3 drivers
 * advect_central2_rk3 / advect_conservative_rk3 (conservative = 0 / 1) */
int rmt_central_rhs(rmt_ctx *ctx, const double *q, const double *a, const double *b, double dx,
                    double dy, const double *phi, double w_cut, int conservative, double *rhs);
int rmt_advect_central_rk3(rmt_ctx *ctx, const double *q, const double *a, const double *b,
                           double dx, double dy, double dt, const double *phi, double w_cut,
                           int conservative, double *out);
/* interpolators.py:64-156 bicubic_interpolate; functions.py:228-251 the bicubic SL-RK4 */
int rmt_bicubic_interpolate(rmt_ctx *ctx, const double *u, const double *xq, const double *yq,
                            long nq, double dx, double dy, double *out);
int rmt_advect_sl_cubic_rk4(rmt_ctx *ctx, const double *q, const double *a, const double *b,
                            const double *X, const double *Y, double dt, double dx, double dy,
                            double *out);
int rmt_all_finite2(rmt_ctx *ctx, const double *a, const double *b, int *finite);
/* Test hook (no reference counterpart): q = divk(x, d), the correctly rounded division by a
 * precomputed divisor that the stencil kernels use for x / (2h), x / (6h), xq / dx, ...
 * (pyrmt_amd/csrc/divk.hpp), and q_ieee = x / d, both on the device (device pointers). */
int rmt_selftest_divk(rmt_ctx *ctx, const double *x, long n, double d, double *q,
                      double *q_ieee);

/* functions.py:48-163 extrapolate_reference_map: exact raster-order (Gauss-Seidel)
 * semantics of the reference; outputs may alias the inputs.  Blocks until the result is
 * complete and returns RMT_EDEVICE if the extrapolation aborted (bug guard / spin timeout),
 * so a caller never sees a partly extrapolated map with RMT_OK. */
int rmt_extrapolate_reference_map(rmt_ctx *ctx, const double *X1, const double *X2,
                                  const double *phi, double dx, double dy, int max_layers,
                                  double *X1_out, double *X2_out);
/* librmt diagnostic (no reference counterpart; blocks): what the last extrapolation on ctx
 * ran (the context options extrap_mode, extrap_parallel): 0 chain, 1 sweep. */
int rmt_extrap_last_path(rmt_ctx *ctx, int *path);

/* functions.py:1366-1367 with benchmarks/common.py:55-57: phi = |xi - (x0,y0)| - R */
int rmt_rebuild_phi_disc(rmt_ctx *ctx, const double *X1, const double *X2, double x0, double y0,
                         double R, double *phi);

/* ---- stress / momentum (functions.py:545-944) -------------------------------------- */
/* functions.py:545-658 solid_cauchy_stress */
int rmt_solid_cauchy_stress(rmt_ctx *ctx, const double *X1, const double *X2, double dx,
                            double dy, double mu_s, double kappa, const double *phi,
                            double w_cut, double detg_clamp, int isochoric, double *sxx,
                            double *sxy, double *syy, double *J);
/* functions.py:660-671 smoothed_heaviside; n elements */
int rmt_smoothed_heaviside(rmt_ctx *ctx, const double *x, long n, double w_t, double *H);
/* benchmarks/common.py:27-50, in place */
int rmt_apply_velocity_bc(rmt_ctx *ctx, int bc_kind, double lid, double *u, double *v);

typedef struct {
    int bc_kind;        /* rmt_bc_kind */
    double lid;         /* lid speed for RMT_BC_NOSLIP_LID */
    double mu_s, kappa, eta_s, rho_s, rho_f, mu_f, w_t;
    double dx, dy, dt;
    int stress_band;    /* functions.py:673-674 stress_band */
    double detg_clamp;
} rmt_momentum_params;

/* functions.py:673-762 momentum_step_rk4 at gamma = 0 (the tuned path; surface tension:
 * rmt_momentum_step_rk4_st).  Outputs u*, v* and the elastic sxx, sxy, syy, J it precomputes. */
int rmt_momentum_step_rk4(rmt_ctx *ctx, const rmt_momentum_params *prm, const double *u,
                          const double *v, const double *p, const double *X1, const double *X2,
                          const double *phi, double *u_new, double *v_new, double *sxx,
                          double *sxy, double *syy, double *J);
/* functions.py:837-861 compute_curvature: div(grad phi / (|grad phi| + 1e-12)) */
int rmt_compute_curvature(rmt_ctx *ctx, const double *phi, double dx, double dy, double *kappa);
/* functions.py:864-895 compute_contact_force: the repulsion between two solids around the
 * mid-surface phi12 = (phi1 - phi2) / 2, cosine window of half-width w_c */
int rmt_compute_contact_force(rmt_ctx *ctx, const double *phi1, const double *phi2, double k_rep,
                              double w_c, double dx, double dy, double *fx, double *fy);
/* functions.py:673-762 momentum_step_rk4 with the surface-tension body force
 * -gamma * kappa * grad H (any gamma; the Python surface routes gamma > 1e-12 here) */
int rmt_momentum_step_rk4_st(rmt_ctx *ctx, const rmt_momentum_params *prm, double gamma,
                             const double *u, const double *v, const double *p, const double *X1,
                             const double *X2, const double *phi, double *u_new, double *v_new,
                             double *sxx, double *sxy, double *syy, double *J);
/* functions.py:765-834 momentum_step_rk4_2solids: two reference maps, the n = 2 mixture of
 * the stresses and densities, the contact force as a body force (k_rep <= 0: none).  Of prm,
 * eta_s and stress_band are unused (as in the reference) and detg_clamp bounds both solids'
 * J.  Jmin = min(Ja, Jb). */
int rmt_momentum_step_rk4_2solids(rmt_ctx *ctx, const rmt_momentum_params *prm, double k_rep,
                                  double w_c, const double *u, const double *v, const double *p,
                                  const double *X1a, const double *X2a, const double *X1b,
                                  const double *X2b, const double *phi_a, const double *phi_b,
                                  double *u_new, double *v_new, double *Jmin);

/* The two pieces of the two-disc driver loop (benchmarks/two_disc_contact.py:80-84, :100-104)
 * that are plain array expressions there: out = q * (phi <= 0), and the per-step record
 * out5 = {cxa, cya, cxb, cyb, min Jmin} with disc_centroid of each level set over the node
 * planes X, Y (host result, blocks; NaN centroid when a level set has no cell <= 0). */
int rmt_mask_solid(rmt_ctx *ctx, const double *q, const double *phi, double *out);
/* (Ha + Hb - 1) rho_f + (1 - Ha) rho_s + (1 - Hb) rho_s with H = smoothed_heaviside(phi, w_t)
 * (functions.py:792-795, two_disc_contact.py:94-95) */
int rmt_mixture_density(rmt_ctx *ctx, const double *phi_a, const double *phi_b, double w_t,
                        double rho_s, double rho_f, double *rho);
int rmt_two_solid_diag(rmt_ctx *ctx, const double *phi_a, const double *phi_b, const double *X,
                       const double *Y, const double *Jmin, double *out5);

/* ---- projection (functions.py:1005-1364) ------------------------------------------- */
/* functions.py:1016-1071 _compute_divergence_rc, constant density: d_f = dt / mean(rho) */
int rmt_divergence_rc(rmt_ctx *ctx, const double *a, const double *b, const double *p,
                      double d_f, double dx, double dy, double *divU);
/* functions.py:1005-1014 _compute_divergence */
int rmt_divergence_central(rmt_ctx *ctx, const double *a, const double *b, double dx,
                           double dy, double *divU);
/* functions.py:1073-1089 _compute_pressure_gradient */
int rmt_pressure_gradient(rmt_ctx *ctx, const double *p, double dx, double dy, double *gx,
                          double *gy);
/* functions.py:1107-1119 _solve_poisson_dct: idctn(dctn(rhs,1)/eig,1) - mean, with eig
 * the DCT-I symbol of functions.py:1091-1104 for this grid (dx, dy). */
int rmt_solve_poisson_dct(rmt_ctx *ctx, const double *rhs, double dx, double dy, double *p);
/* Test hook (no reference counterpart): the solve's plain row pass alone, on the LDS path
 * (RMT_ENOTSUP otherwise): dst = scale * DCT-I of every row of src (device pointers, (ny, nx)).
 * rowmark (nullable, ny bytes): only the rows marked (unmarked != 0: only the others), the rest
 * of dst is left as it is.  rs (nullable, ny doubles, not with rowmark): the row sums the pass
 * takes itself; rs_ref (nullable): the row sums of dst in the order of the projection's mean. */
int rmt_selftest_dct_rows(rmt_ctx *ctx, const double *src, double dx, double dy, double scale,
                          double *dst, double *rs, double *rs_ref,
                          const unsigned char *rowmark, int unmarked);
/* Test hook (no reference counterpart): one row pass of the DCT-II Neumann solve (mac.py:118-123)
 * under the plan of this context's (ny, nx) and (dx, dy).  axis 0: rows of length nx, 1: rows
 * of length ny; src, dst (device, nrows rows of that length; may alias).  mode 0: dst = the
 * unnormalised DCT-II 2 sum x cos of every row (mroot nullable: of x - mroot[0] / mcount);
 * mode 2: its inverse; mode 1 (axis 1): forward, row r / (lamx[row0 + r] + lamy[k]) with the
 * (row0 + r = 0, k = 0) entry zeroed, inverse.  Rows >= nrows of dst are left as they are. */
int rmt_selftest_dct2_rows(rmt_ctx *ctx, int mode, int axis, const double *src, int nrows,
                           int row0, const double *mroot, double mcount, double dx, double dy,
                           double *dst);
/* functions.py:1255-1364 pressure_projection_amg, Neumann branch, constant density rho
 * (variable density: rmt_pressure_projection_variable).  p_prev may be NULL. */
int rmt_pressure_projection(rmt_ctx *ctx, const double *a_star, const double *b_star,
                            double dx, double dy, double dt, double rho, int bc_kind,
                            double lid, const double *p_prev, double *a, double *b, double *p);
/* The same branch with rho a device (ny, nx) array that is constant only to rounding
 * (0 < ptp <= 1e-10, e.g. the two-solid mixture density at rho_s == rho_f), taken pointwise
 * as the reference does: d_f = dt / mean(rho), rhs = rho * divU / dt, a = a* - (dt / rho)
 * grad p_c.  p_prev may be NULL. */
int rmt_pressure_projection_rho_field(rmt_ctx *ctx, const double *a_star, const double *b_star,
                                      double dx, double dy, double dt, const double *rho,
                                      int bc_kind, double lid, const double *p_prev, double *a,
                                      double *b, double *p);
/* The variable-density branch (rho a device (ny, nx) array with ptp > 1e-10),
 * functions.py:1296-1328 + :1350-1364: Rhie-Chow divergence with per-face dt/rho, rhs =
 * divU/dt - mean, preconditioned CG (scipy.sparse.linalg.cg semantics: x0 = 0, stop when
 * ||r|| < rtol ||rhs||, at most maxiter iterations; the reference passes tol = 1e-6,
 * maxiter = 200) on the matrix-free div((1/rho) grad) operator with the DCT-I solve as the
 * preconditioner, then a = a* - (dt/rho) grad p_c, BC, p = p_prev + p_c - mean.
 * *iters receives the iteration count (maxiter: not converged, as scipy's info > 0). */
int rmt_pressure_projection_variable(rmt_ctx *ctx, const double *a_star, const double *b_star,
                                     double dx, double dy, double dt, const double *rho,
                                     int bc_kind, double lid, const double *p_prev, double rtol,
                                     int maxiter, double *a, double *b, double *p, int *iters);
/* functions.py:1122-1168 _apply_variable_poisson: div((1/rho) grad p), face-averaged 1/rho,
 * mirror ghosts. */
int rmt_apply_variable_poisson(rmt_ctx *ctx, const double *p, double dx, double dy,
                               const double *inv_rho, double *out);
/* functions.py:1016-1070 _compute_divergence_rc with a variable rho array (per-face
 * d_f = dt * 0.5 * (1/rho_l + 1/rho_r)). */
int rmt_divergence_rc_variable(rmt_ctx *ctx, const double *a, const double *b, const double *p,
                               double dt, const double *rho, double dx, double dy,
                               double *divU);

/* functions.py:165-192 compute_timestep; host result, blocks. */
int rmt_compute_timestep(rmt_ctx *ctx, const double *a, const double *b, double dx, double dy,
                         double CFL, double dt_min_cap, double mu_s, double rho_s, double gamma,
                         double rho_f, double mu_f, double eta_s, double kappa, double *dt);

/* ---- standalone diagnostics and the blended RHS (pyRMT/__init__.py:16, :28-31) --------
 * Energies return a host scalar and block; the sum runs in np.sum's own order (pairwise over
 * 8192-element chunks), so a bit-exact density gives a bit-exact energy. */
/* output.py:6-39: sum(0.5 rho (a^2 + b^2)) dx dy, rho = (1-H) rho_s + H rho_f */
int rmt_compute_kinetic_energy(rmt_ctx *ctx, const double *a, const double *b, double rho_f,
                               double rho_s, const double *phi, double w_t, double dx, double dy,
                               double *ke);
/* output.py:41-134: neo-Hookean + volumetric strain energy over phi <= 0 (edge-padded grads) */
int rmt_compute_strain_energy(rmt_ctx *ctx, const double *X1, const double *X2, const double *phi,
                              double mu_s, double dx, double dy, double kappa, double *se);
/* output.py:136-193: viscous dissipation rate, mu = H mu_f + (1-H) eta_s */
int rmt_compute_viscous_dissipation(rmt_ctx *ctx, const double *a, const double *b, double mu_f,
                                    const double *phi, double w_t, double dx, double dy,
                                    double eta_s, double *diss);
/* output.py:195-211 divergence_2d_interior (the div_vel dataset of output_simulation_data,
 * pad = 4 there): central differences on the cells >= pad from every edge, 0 elsewhere */
int rmt_divergence_2d_interior(rmt_ctx *ctx, const double *u, const double *v, double dx,
                               double dy, int pad, double *div);
/* functions.py:897-944 velocity_rhs_blended_optimized: H, rho_local device arrays; the
 * surface-tension force fx, fy device arrays or both NULL (the scalar 0.0 of the gamma = 0
 * path).  (phi, dH_dx, dH_dy of the reference signature are unused by its body.) */
int rmt_velocity_rhs_blended(rmt_ctx *ctx, const double *u, const double *v, const double *p,
                             const double *sxx, const double *sxy, const double *syy, double dx,
                             double dy, double mu_f, const double *H, const double *rho,
                             const double *fx, const double *fy, double *rhs_u, double *rhs_v);

/* ---- fused, device-resident time step (the loop body of the benchmark drivers) ----- */
typedef enum {
    RMT_SHAPE_NONE = 0,   /* pure fluid (lid_driven_cavity.py): phi = 1, no solid       */
    RMT_SHAPE_DISC = 1    /* one disc: phi = |xi - (x0,y0)| - R                         */
} rmt_shape_kind;

typedef struct {
    int ny, nx;
    double dx, dy;
    const double *xs, *ys;   /* HOST node coordinates, length nx and ny (create_grid) */
    int scheme;              /* rmt_scheme                                            */
    int bc_kind;             /* rmt_bc_kind                                           */
    double lid;
    int shape;               /* rmt_shape_kind                                        */
    double x0, y0, R;
    double mu_s, kappa, rho_s, eta_s, mu_f, rho_f, w_t;
    int layers;              /* extrapolation layers                                  */
    double cfl, dt_cap;      /* compute_timestep CFL and dt_min_cap                   */
    int stress_band;
    double detg_clamp;
    int energies;            /* per-step KE / SE / dissipation (disc_in_taylor_green) */
} rmt_sim_params;

typedef struct rmt_sim rmt_sim;

/* Per-step diagnostics, one record per completed step (soft_disc_in_lid_driven.py:233
 * traj tuple, disc_in_taylor_green.py:243 hist tuple). */
typedef struct {
    double t, dt, cx, cy, minJ, maxJ, umax;
    double ke, se, diss, integ, ry;
} rmt_diag;

int rmt_sim_create(rmt_ctx *ctx, const rmt_sim_params *prm, rmt_sim **out);
int rmt_sim_destroy(rmt_sim *sim);
/* how often (steps, 1 .. 64) rmt_sim_step reads the device diagnostics back (see below) */
int rmt_sim_set_sync_every(rmt_sim *sim, int k);
/* field ids: 0 u (a), 1 v (b), 2 p, 3 X1, 4 X2, 5 phi (last rebuilt), 6 J, 7 sigma_xx,
 * 8 sigma_xy, 9 sigma_yy (the solid stress of the last momentum step) */
int rmt_sim_field(rmt_sim *sim, int field, double **dev_ptr);
/* Run nsteps loop bodies.  dt comes from compute_timestep on device and is clipped to
 * t_end - t as the drivers do; steps after t >= t_end are no-ops.  Blocks: the diagnostics
 * and flags of the enqueued steps are read back every rmt_sim_set_sync_every steps (64 by
 * default) and at the end of the call, and errors (non-finite velocity, extrapolation abort)
 * are returned then: the diagnostics and t stop at the last good step, while the fields are
 * those after the last ENQUEUED step (up to sync_every - 1 steps past the failing one; with
 * sync_every = 1, or a finite t_end, they are the failing step's).  The call returns once the
 * last step has finished on the stream. */
int rmt_sim_step(rmt_sim *sim, int nsteps, double t_end);
/* Carry (off by default): with on != 0, a call's last step also prepares what the next
 * step needs from the final state alone (the extrapolation geometry of its known plane, the
 * prep planes' constant-segment marks, max |u|^2 from the projection), and the next
 * rmt_sim_step starts from it -- its first step then costs what every later step costs.
 * The caller promises to call rmt_sim_invalidate after writing any field between calls; any
 * other use of the context's workspace between calls ends the carry by itself.  Results
 * are bit-identical either way. */
int rmt_sim_set_carry(rmt_sim *sim, int on);
int rmt_sim_invalidate(rmt_sim *sim);
/* Phase timers (HIP events on the context stream, accumulated over steps while on):
 * ms[0] dt reduction, [1] advection, [2] extrapolation, [3] momentum (prep + 4 stages +
 * BC), [4] projection, [5] diagnostics, [6] the four RK4 stage kernels alone,
 * [7] the extrapolation sweep kernel alone; calls[k] = number of timed intervals. */
int rmt_sim_set_profiling(rmt_sim *sim, int on);
int rmt_sim_phase_times(rmt_sim *sim, double *ms8, long *calls8);
/* Copy the diagnostics of all completed steps since creation (blocks). */
int rmt_sim_diagnostics(rmt_sim *sim, rmt_diag *out, int max_records, int *n_records);

/* ---- periodic branch (functions.py:1177-1290; tests/test_poisson.py:24-78) -----------
 * Overlap grid (x[-1] == x[0]): operators on the reduced (ny-1) x (nx-1) sub-grid, tiled
 * back; ny, nx >= 3, rectangular grids allowed.
 * lamx / lamy: HOST per-axis symbols -(sin(2 pi k / m) / h)^2, length m = nx - 1 / ny - 1. */
int rmt_divergence_periodic(rmt_ctx *ctx, const double *a, const double *b, double dx, double dy,
                            double *divU);                           /* functions.py:1236 */
int rmt_pressure_gradient_periodic(rmt_ctx *ctx, const double *p, double dx, double dy,
                                   double *gx, double *gy);          /* functions.py:1246 */
int rmt_solve_poisson_fft(rmt_ctx *ctx, const double *rhs, const double *lamx,
                          const double *lamy, double *p);            /* functions.py:1216 */
/* pressure_projection_amg(bc_type='periodic') (functions.py:1277-1290): rho_bar = mean rho
 * in the Poisson rhs; rho_cells (device, nullable) the local density of the correction */
int rmt_pressure_projection_periodic(rmt_ctx *ctx, const double *a_star, const double *b_star,
                                     double dx, double dy, double dt, double rho_bar,
                                     const double *rho_cells, int bc_kind, double lid,
                                     const double *lamx, const double *lamy,
                                     const double *p_prev, double *a, double *b, double *p);

/* ---- slab-decomposed step (the fused step over G GPUs, 1D row slabs) ----
 * One rmt_slab = rows [r0, r1) of the global ny x nx grid (row_splits[rank] ..
 * row_splits[rank+1]) plus RMT_SLAB_HALO resident rows on each side, and the column block
 * [col_splits[rank], col_splits[rank+1]) of the transposed DCT pass.  The caller
 * (pyrmt_amd/distributed.py) runs the phases below on every slab, in this order, and
 * performs the collectives named between them (torch.distributed over RCCL, or in-process
 * copies); the result is bit-identical to rmt_sim_step when every slab holds 2^m rows at a
 * multiple of 2^m (the row-tree means), and equal to rounding otherwise.
 * The ctx must be created for the GLOBAL grid; splits must be even and slabs >= HALO rows.
 * Replaces the loop body of soft_disc_in_lid_driven.py:206-235 (semi-Lagrangian, one disc).
 *   buffers: 0-6 u v p X1 X2 phi J (resident (hi-lo) x nx planes), 7 p_c plane,
 *            8 known bits (ny x W u64), 9 rim entries (3 doubles each), 10 DCT slab buffer
 *            (owned x nx), 11 DCT column buffer (ny x nc), 12 scalars (16 doubles:
 *            [0] max|u|^2 owned, [1..10] diag partials, [11] flags (1 non-finite velocity,
 *            2 halo overrun, 4 extrapolation abort), [12] rim count, [13] row-tree root,
 *            [14] cells fitted)
 *   info: r0, r1, lo, hi, c0, c1, W (64-cell words per row), HALO; and the constant dt. */
#define RMT_SLAB_HALO 12
typedef struct rmt_slab rmt_slab;
int rmt_slab_create(rmt_ctx *ctx, const rmt_sim_params *prm, int G, int rank,
                    const int *row_splits, const int *col_splits, rmt_slab **out);
int rmt_slab_destroy(rmt_slab *slab);
int rmt_slab_info(rmt_slab *slab, int *ints8, double *dt_const);
int rmt_slab_buffer(rmt_slab *slab, int id, void **dev_ptr);
int rmt_slab_begin(rmt_slab *slab);                      /* scal[0] of the initial state  */
/* optional, while the halo exchange is in flight: the advection of the rows that read no
 * halo row; rmt_slab_advect (after the halo) then does the remaining rows */
int rmt_slab_advect_interior(rmt_slab *slab, double dt);
int rmt_slab_advect(rmt_slab *slab, double dt);          /* then: allgather known bit rows */
int rmt_slab_rim_pack(rmt_slab *slab);                   /* then: allgather rim entries    */
int rmt_slab_extrapolate(rmt_slab *slab, const double *gathered, const long long *counts,
                         long long cap);                 /* gathered: G x cap x 3 (device) */
int rmt_slab_momentum(rmt_slab *slab, double dt);
int rmt_slab_project_rows(rmt_slab *slab, double dt);    /* then: all_to_all 10 -> 11      */
int rmt_slab_project_cols(rmt_slab *slab);               /* then: all_to_all 11 -> 10      */
int rmt_slab_project_unrows(rmt_slab *slab);             /* then: allgather scal[13]       */
int rmt_slab_sub_mean(rmt_slab *slab, int which, const double *roots_dev);  /* 0 p_c, 1 p */
int rmt_slab_project_correct(rmt_slab *slab, double dt); /* after halo(p_c); then roots   */
int rmt_slab_finish(rmt_slab *slab);                     /* then: allgather scal          */
/* Device-dt step (no host round trip inside the step; distributed.py's asynchronous path):
 * with on != 0 every phase reads dt from the slab's device scalar instead of its dt argument.
 * rmt_slab_next_dt: after the scalar allgather (G x 16 doubles, device), record
 * {dt, max|u|^2, the gathered blocks} into ring_slot (nullable, 2 + 16 G doubles) and set the
 * next dt from the gathered max|u|^2 -- the host's expression, NaN-propagating max.
 * rmt_slab_rim_pack + rmt_slab_rim_cap: the rim allgather moves a fixed `cap` entries per slab
 * (flag 8 in the scalar block's flags when a slab's rim is larger; the host raises);
 * rmt_slab_extrapolate_dev reads the counts from the gathered scalar blocks. */
int rmt_slab_set_device_dt(rmt_slab *slab, int on);
int rmt_slab_next_dt(rmt_slab *slab, const double *gathered_scal, int G, double *ring_slot);
int rmt_slab_rim_cap(rmt_slab *slab, long long cap);
/* The next step's extrapolation geometry beside this step's projection (as rmt_sim_step's
 * early geometry): after rmt_slab_momentum, rmt_slab_next_bits writes the owned rows of the
 * next known plane into buffer 13 (bits_next); the caller allgathers its rows; then
 * rmt_slab_geometry runs the value-independent extrapolation passes on the slab's second
 * stream, and the next step's rmt_slab_advect / rmt_slab_extrapolate* use them (no bits
 * allgather, no geometry on the critical path).  rmt_slab_drop_geometry forgets it (a step
 * that will not run).  Replaces the geometry half of extrapolate_reference_map
 * (functions.py:78-99: targets, acceptance, weights depend on the known set only). */
int rmt_slab_next_bits(rmt_slab *slab);
int rmt_slab_geometry(rmt_slab *slab);
int rmt_slab_drop_geometry(rmt_slab *slab);
int rmt_slab_extrapolate_dev(rmt_slab *slab, const double *gathered, const double *gathered_scal,
                             long long cap);

/* ---- MAC path (config 5): pyRMT/mac.py operators on an N x N cell grid -----------
 * ctx created for (N, N) cells; u is (N, N+1) x-faces, v (N+1, N) y-faces, p / phi (N, N). */
int rmt_mac_divergence(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy,
                       double *out);                                       /* mac.py:81-84  */
int rmt_mac_gradient_p(rmt_ctx *ctx, const double *p, double dx, double dy, double *gu,
                       double *gv);                                        /* mac.py:87-101 */
/* lamx (nx) / lamy (ny): HOST per-axis eigenvalues (eig = lamx[None,:] + lamy[:,None], the
 * (0,0) mode zeroed), or both NULL for poisson_eigs_neumann's own (mac.py:104-115) */
int rmt_mac_solve_poisson_neumann(rmt_ctx *ctx, const double *rhs, double dx, double dy,
                                  const double *lamx, const double *lamy,
                                  double *out);                           /* mac.py:118-123 */
int rmt_mac_project(rmt_ctx *ctx, const double *u_star, const double *v_star, double dx,
                    double dy, double dt, double rho, const double *lamx, const double *lamy,
                    double *u, double *v, double *phi);                   /* mac.py:126-139 */
/* fu / fv: face forces or both NULL                                       mac.py:196-232 */
int rmt_mac_momentum_predictor(rmt_ctx *ctx, const double *u, const double *v, double nu,
                               double dx, double dy, double dt, double U_lid, const double *fu,
                               const double *fv, double rho, double *u_star, double *v_star);
int rmt_mac_contact_stress(rmt_ctx *ctx, const double *phi_a, const double *phi_b, double eta,
                           double Gsum, double eps, double dx, double dy, double *txx,
                           double *txy, double *tyy);                     /* mac.py:729-749 */
/* The free-slip box (mac.py:653-689): rmt_mac_momentum_predictor's arithmetic with mirrored
 * tangential ghosts (u below row 0 / above row N-1 and v beside columns 0 / N-1 are the
 * face's own value); wall-normal faces of u_star / v_star are written as 0.  fu / fv: face
 * forces or both NULL. */
int rmt_mac_momentum_predictor_freeslip(rmt_ctx *ctx, const double *u, const double *v, double nu,
                                        double dx, double dy, double dt, const double *fu,
                                        const double *fv, double rho, double *u_star,
                                        double *v_star);
/* mac.py:179-193: fu (N, N+1), fv (N+1, N) = -gamma * (kappa averaged to the face) * the
 * compact face gradient of H; every face is written, the wall faces as 0. */
int rmt_mac_interfacial_force_faces(rmt_ctx *ctx, const double *kappa, const double *H,
                                    double gamma, double dx, double dy, double *fu, double *fv);
/* MAC IMEX tier (imex.hip), square N x N cell grid (ctx ny = nx = N).  kind 0: u faces, full
 * (N, N+1), interior (N, N-1); kind 1: v faces, full (N+1, N), interior (N-1, N).
 * rmt_mac_lap_lid_hom: the homogeneous-BC Laplacian of a full field on the interior faces,
 *   mac.py:243-250 _lap_u_lid_hom (kind 0) / :253-260 _lap_v_lid_hom (kind 1).
 * rmt_mac_helmholtz: (I - coef Lap_hom) x = rhs on the interior faces by scipy's cg
 *   (x0 = rhs, atol = rtol ||rhs||), precond 0: mac.py:263-275 _cg_helmholtz, precond 1:
 *   mac.py:287-316 _pcg_helmholtz (DST-II preconditioner); *iters = iterations run.
 * rmt_mac_momentum_predictor_lid_imex: mac.py:319-369; fu / fv full face forces or NULL;
 *   iters[2] (optional): the u and v PCG iteration counts. */
int rmt_mac_lap_lid_hom(rmt_ctx *ctx, int kind, const double *f, double dx, double dy,
                        double *out);
int rmt_mac_helmholtz(rmt_ctx *ctx, int kind, const double *rhs, double coef, double dx,
                      double dy, double rtol, int maxiter, int precond, double *x, int *iters);
int rmt_mac_momentum_predictor_lid_imex(rmt_ctx *ctx, const double *u, const double *v,
                                        double nu, double dx, double dy, double dt,
                                        double U_lid, const double *fu, const double *fv,
                                        double rho, double rtol, double cs2, double *u_star,
                                        double *v_star, int *iters);
/* mac.py:381-442 momentum_predictor_lid_semilag, its semi-Lagrangian branch (the caller
 * checked CFL > cfl_switch, mac.py:387-390): midpoint backtrace through cubic-spline
 * interpolation (scipy.ndimage.map_coordinates order 3, mode 'nearest', mac.py:374-378),
 * then the implicit viscosity by PCG; iters as above. */
int rmt_mac_momentum_predictor_lid_semilag(rmt_ctx *ctx, const double *u, const double *v,
                                           double nu, double dx, double dy, double dt,
                                           double U_lid, const double *fu, const double *fv,
                                           double rho, double cs2, double rtol, double *u_star,
                                           double *v_star, int *iters);

/* The loop body of benchmarks/mac_multi_disc_lid.py:62-98 (K soft discs with contact, lid
 * U_lid, fixed dt), device-resident.  Fields: 0 u, 1 v, 2 p (disc ignored); 3 X1, 4 X2,
 * 5 phi of disc `disc`. */
#define RMT_MAC_MAXD 8
typedef struct {
    int N;                   /* cells per side, dx = 1 / N                               */
    double dx;
    int n_discs;
    double R[RMT_MAC_MAXD], cx[RMT_MAC_MAXD], cy[RMT_MAC_MAXD];
    double U_lid, mu_s, mu_f, rho, eta;
    int layers;              /* extrapolation layers (3 in the driver)                   */
    double dt;               /* the driver's fixed step (mac_multi_disc_lid.py:58)        */
} rmt_mac_params;
typedef struct {
    double t, dt, minJ, maxJ, umax;
    int n_discs;
    double cx[RMT_MAC_MAXD], cy[RMT_MAC_MAXD];   /* centroid of phi_k <= 0 (:104)        */
    int diverged;   /* mac_multi_disc_lid.py:100-103: u non-finite, min J < 0, max J > 20 or a
                       disc with no phi <= 0 cell after this step; the sim stops stepping     */
} rmt_mac_diag;
typedef struct rmt_mac_sim rmt_mac_sim;
/* rmt_mac_sim_step stops after a step whose record has diverged set (the reference driver
 * breaks out of its loop there); later calls are no-ops.  RMT_EDEVICE on an extrapolation
 * abort, RMT_ENONFINITE on a non-finite velocity fed to the advection. */
int rmt_mac_sim_create(rmt_ctx *ctx, const rmt_mac_params *prm, rmt_mac_sim **out);
/* The same loop in the free-slip box, the loop body of benchmarks/mac_disc_in_tg_convergence.py
 * :53-82 (one disc) and mac_two_disc_contact.py:50-81 (two): wall = RMT_MAC_WALL_FREESLIP
 * takes the predictor's ghosts of rmt_mac_momentum_predictor_freeslip (U_lid is not read).
 * stop_on_divergence = 0: a step's record still carries diverged and the loop goes on, as
 * those two drivers do (the two error returns of rmt_mac_sim_step stay).  Defaults: lid,
 * stop.  Legal only before the first step (t == 0 and no record); afterwards, or with an
 * unknown wall kind, RMT_EINVAL.  The slab path (rmt_mac_slab_*) is lid-only. */
#define RMT_MAC_WALL_LID 0
#define RMT_MAC_WALL_FREESLIP 1
int rmt_mac_sim_set_mode(rmt_mac_sim *sim, int wall, int stop_on_divergence);
int rmt_mac_sim_destroy(rmt_mac_sim *sim);
int rmt_mac_sim_field(rmt_mac_sim *sim, int field, int disc, double **dev_ptr);
int rmt_mac_sim_step(rmt_mac_sim *sim, int nsteps, double t_end);
int rmt_mac_sim_diagnostics(rmt_mac_sim *sim, rmt_mac_diag *out, int max_records,
                            int *n_records);

/* ---- periodic MAC tier (macper.hip): mac.py:445-540, 636-650 -----------------------
 * ctx created for (ny, nx); u (x-faces), v (y-faces) and p (centres) are all (ny, nx) planes
 * and every index wraps (np.roll); ny, nx >= 2, rectangular and odd extents allowed.
 * The scalars a caller of the reference forms in Python come in formed: dx2 = dx**2,
 * dy2 = dy**2, twodx = 2*dx, twody = 2*dy, coef = dt*nu, rho_dt = rho/dt, dt_rho = dt/rho.
 * lx (nx) / ly (ny): HOST per-axis eigenvalues, symbol = lx[None,:] + ly[:,None] (one
 * rounded add), applied on the ny x (nx/2+1) half-spectrum of a rocFFT D2Z / Z2D pair. */
int rmt_mac_per_divergence(rmt_ctx *ctx, const double *u, const double *v, double dx, double dy,
                           double *out);                                  /* mac.py:449-450 */
/* gu or gv may be NULL */
int rmt_mac_per_gradient_p(rmt_ctx *ctx, const double *p, double dx, double dy, double *gu,
                           double *gv);                                   /* mac.py:453-458 */
int rmt_mac_per_predictor(rmt_ctx *ctx, const double *u, const double *v, double nu, double dx2,
                          double dy2, double twodx, double twody, double dt, double *u_star,
                          double *v_star);                                /* mac.py:636-650 */
int rmt_mac_per_predictor_imex(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                               double twody, double dt, double coef, const double *lx,
                               const double *ly, double *u_star,
                               double *v_star);                           /* mac.py:521-540 */
/* mode 0: out = ifft(fft(rhs) / symbol), (0,0) zeroed (solve_poisson_periodic, mac.py:470-473);
 * mode 1: out = ifft(fft(rhs) / (1 - coef * symbol)) (solve_helmholtz_periodic, :512-518).
 * out may be rhs. */
int rmt_mac_per_solve(rmt_ctx *ctx, const double *rhs, int mode, double coef, const double *lx,
                      const double *ly, double *out);
int rmt_mac_per_project(rmt_ctx *ctx, const double *u_star, const double *v_star, double dx,
                        double dy, double rho_dt, double dt_rho, const double *lx,
                        const double *ly, double *u, double *v,
                        double *phi);                                     /* mac.py:476-480 */
/* nsteps of predictor (imex 0: rmt_mac_per_predictor, 1: rmt_mac_per_predictor_imex) +
 * projection on the device planes u, v in place, the loop of
 * benchmarks/mac_taylor_green_convergence.py:59-66; no host round trip inside, workspace
 * from the context.  p (may be NULL): the last projection's phi.  Option macp_fused
 * (RMT_MACP_FUSED) picks the explicit step's fused predictor + divergence kernel; the
 * results are the same bits as the separate entry points composed. */
int rmt_mac_per_steps(rmt_ctx *ctx, double *u, double *v, double nu, double dx, double dy,
                      double dx2, double dy2, double twodx, double twody, double dt, double coef,
                      double rho_dt, double dt_rho, const double *lx, const double *ly, int imex,
                      int nsteps, double *p);

/* ---- periodic MAC tier, semi-Lagrangian predictor (macper_sl.hip): mac.py:587-633 ----
 * Cubic B-spline interpolation on a periodic plane, scipy.ndimage's order 3, mode
 * "grid-wrap": the prefilter wraps and pads nothing, every tap wraps by an integer modulo.
 * Equal to rounding against scipy (the prefilter runs as windowed two-sided sums, 48 terms
 * a side, parallel within a line), never bit for bit.  Workspace from the context. */
/* the coefficient plane of f, axis 0 then axis 1 (what map_coordinates' prefilter=True makes
 * inside mac.py:597-598); out may be f */
int rmt_mac_per_spline_prefilter(rmt_ctx *ctx, const double *f, double *out);
/* _interp_per(f, iq, jq) at nq points, f[j, i] at index (i, j): iq, jq, out device arrays of
 * nq doubles, any finite coordinate */
int rmt_mac_per_interp(rmt_ctx *ctx, const double *f, const double *iq, const double *jq,
                       int nq, double *out);                              /* mac.py:593-598 */
/* _sl_advect_per: f at offset (ox, oy) advected by the face velocities uf (offset (0, 1/2))
 * and vf ((1/2, 0)), RK2 midpoint backtrace, five interpolations a point; out may be f */
int rmt_mac_per_sl_advect(rmt_ctx *ctx, const double *f, const double *uf, const double *vf,
                          double ox, double oy, double dx, double dy, double dt,
                          double *out);                                   /* mac.py:601-614 */
/* cfl = dt * max(max|u| / dx, max|v| / dy) is formed on the device (Python's max, NaN as
 * np.max); cfl <= cfl_switch: rmt_mac_per_predictor_imex, the same bits; else u, v advected by
 * themselves and two Helmholtz solves.  took_sl (may be NULL): 1 for the SL branch.
 * u_star, v_star distinct from u, v and from each other. */
int rmt_mac_per_predictor_semilag(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                                  double twody, double dx, double dy, double dt, double coef,
                                  double cfl_switch, const double *lx, const double *ly,
                                  double *u_star, double *v_star,
                                  int *took_sl);                          /* mac.py:617-633 */
/* rmt_mac_per_steps with that predictor (integrator "imex-sl" of
 * benchmarks/mac_taylor_green_convergence.py:47-66): the branch of every step is decided and
 * taken on the device, no host read inside the loop.  sl_steps (may be NULL): the number of
 * the nsteps steps that took the SL branch, read once after the last one. */
int rmt_mac_per_steps_sl(rmt_ctx *ctx, double *u, double *v, double nu, double dx, double dy,
                         double dx2, double dy2, double twodx, double twody, double dt,
                         double coef, double rho_dt, double dt_rho, const double *lx,
                         const double *ly, double cfl_switch, int nsteps, double *p,
                         int *sl_steps);

/* ---- reference-map reinitialisation with stored deformation (mac_reinit.hip):
 * benchmarks/mac_reinit_test.py:23-113 (Rycroft 2018) ----
 * All planes (ny, nx) of the context unless stated; arrays of plane pointers (q, out, Fs, Ftot)
 * are host arrays of device pointers.  Bit-exact against the reference but for H's sine. */
/* functions.py:194-227 for np (1..8) planes on one RK4 backtrace: out[k] = the bits of
 * rmt_advect_sl_rk4(q[k]) and, phi non-NULL, of rmt_mask_solid on top (q * 0.0 keeps -0.0 and
 * NaN).  No out[k] may be one of the q planes. */
int rmt_advect_sl_rk4_multi(rmt_ctx *ctx, int np, const double *const *q, const double *a,
                            const double *b, const double *X, const double *Y, double dt,
                            double dx, double dy, const double *phi, double *const *out);
/* :23-33, :74-81: F_current from the map (grad_central_*_2nd, |detG| < 1e-9 -> 1e-9),
 * J_ep = 1 / detG, Ftot = F_current . Fs (components 11, 12, 21, 22),
 * S = (1 - smoothed_heaviside(phi, w_t)) * mu_s * b.  Ftot: NULL, or four planes. */
int rmt_mac_total_stress(rmt_ctx *ctx, const double *X1, const double *X2,
                         const double *const *Fs, const double *phi, double dx, double dy,
                         double w_t, double mu_s, double *Sxx, double *Sxy, double *Syy,
                         double *J_ep, double *const *Ftot);
/* :74-85 in one launch: that stress, its central divergence averaged to the interior faces,
 * wall faces 0: fu (ny, nx+1), fv (ny+1, nx), J_ep.  The same bits as rmt_mac_total_stress,
 * rmt_grad_x_2nd / rmt_grad_y_2nd and the face average composed; S stays in LDS. */
int rmt_mac_total_force(rmt_ctx *ctx, const double *X1, const double *X2,
                        const double *const *Fs, const double *phi, double dx, double dy,
                        double w_t, double mu_s, double *fu, double *fv, double *J_ep);
/* :91-94: out3 (device, 3 doubles) = max J_ep, min J_ep (NaN propagates) and the number of
 * cells over phi <= 0 (-inf, +inf, 0 when there is none). */
int rmt_mac_epoch_distortion(rmt_ctx *ctx, const double *J_ep, const double *phi, double *out3);

/* ---- soft disc under the integrator ladder (benchmarks/mac_soft_disc_lid.py:79-150,
 * mac_soft.hip).  Planes are (ny, nx) of the context, u / fu (ny, nx+1), v / fv (ny+1, nx);
 * dx, dy are arguments: nothing assumes a square grid or box. ---- */
/* :103-110 in one launch: solid_cauchy_stress (w_cut = 0) and its J, the blend with
 * 1 - smoothed_heaviside(phi, w_t), the central divergence (rmt_grad_x_2nd / rmt_grad_y_2nd),
 * the average to the interior faces, wall faces 0.  The same bits as those operators composed;
 * the blended stress stays in LDS. */
int rmt_mac_solid_force(rmt_ctx *ctx, const double *X1, const double *X2, const double *phi,
                        double dx, double dy, double w_t, double mu_s, double kappa,
                        double detg_clamp, int isochoric, double *fu, double *fv, double *J);
/* :133-134: um = 0.5 (u0 + u1), uc = 0.5 (um[:, :-1] + um[:, 1:]), likewise v; with u0 == u1
 * and v0 == v1 the plain face-to-centre average of :82-83 (0.5 (u + u) is u). */
int rmt_mac_midpoint_centres(rmt_ctx *ctx, const double *u0, const double *v0, const double *u1,
                             const double *v1, double *uc, double *vc);
/* :139-150: out8 (device, 8 doubles) = the number of phi <= 0 cells, the sums of Xc and Yc over
 * them (cell centres (i + 0.5) dx, (j + 0.5) dy), min J and max J over the plane, max|u|,
 * max|v| (NaN propagates in all four) and 1.0 if u or v holds a non-finite value, else 0.0. */
int rmt_mac_soft_diag(rmt_ctx *ctx, const double *phi, const double *J, const double *u,
                      const double *v, double dx, double dy, double *out8);
/* mac.py:698-721: SSP-RK3 of -H div(u xi) with the face velocity, H = (phi <= w_cut); three
 * launches over two scratch planes of the context.  out must not be xi. */
int rmt_mac_advect_xi_conservative(rmt_ctx *ctx, const double *xi, const double *u,
                                   const double *v, double dx, double dy, double dt,
                                   const double *phi, double w_cut, double *out);

/* ---- viscoelastic constitutive layer (pyRMT/viscoelastic.py, viscoelastic.hip).  Elementwise
 * over n >= 1 cells of equally long device planes, whatever the context's grid: a symmetric
 * tensor is three planes (11, 12, 22), a velocity gradient L four (11, 12, 21, 22), each passed
 * as a host array of device pointers.  An output plane may be its own input plane.  tau = inf
 * gives 1 / tau = 0 exactly (:38, :107).  The arithmetic entries (ucm, stress) give the
 * reference's bits; the others evaluate exp, log, sin, cos and atan2 exactly where the
 * reference does and differ from it only through them. ---- */
/* The elementwise launch of the entries below for n cells: workgroups and threads per
 * workgroup; a thread walks k, k + blocks * threads, ... (host only, for the tests). */
int rmt_ve_launch_shape(long n, int *blocks, int *threads);
/* :27-42 ucm_local_rhs. */
int rmt_ve_ucm_rhs(rmt_ctx *ctx, long n, const double *const *b, const double *const *L,
                   double tau, double *const *out);
/* :45-54 ucm_local_step applied nsteps >= 1 times, the state in registers between steps.
 * track / out_err (both or neither): track is three host-array entries, each null or nsteps
 * device doubles; out_err (n doubles) gets per cell the largest |component - track[step]| over
 * the steps and the tracked components, as the running max(err, abs(..)) of
 * benchmarks/viscoelastic_relaxation_test.py:32-36, :81 keeps it. */
int rmt_ve_ucm_steps(rmt_ctx *ctx, long n, const double *const *b, const double *const *L,
                     double tau, double dt, int nsteps, const double *const *track,
                     double *const *out, double *out_err);
/* :167-179 viscoelastic_stress: G b, plus G_inf bref where bref is given and G_inf != 0.0 (the
 * branch of :175; not taken, the result is G * b with nothing added). */
int rmt_ve_stress(rmt_ctx *ctx, long n, const double *const *b, double G,
                  const double *const *bref, double G_inf, double *const *out);
/* :71-76 sym_log and :79-84 sym_exp through _sym_eig2 (:63-68); np.maximum's NaN rule. */
int rmt_ve_sym_log(rmt_ctx *ctx, long n, const double *const *a, double *const *out);
int rmt_ve_sym_exp(rmt_ctx *ctx, long n, const double *const *a, double *const *out);
/* :87-116 logconf_local_rhs (|lam2 - lam1| < 1e-10 selects exp(-l1), :104-106). */
int rmt_ve_logconf_rhs(rmt_ctx *ctx, long n, const double *const *psi, const double *const *L,
                       double tau, double *const *out);
/* :133-147 relax_exact; tau = inf or dt == 0.0 copies the input bits (:140-141). */
int rmt_ve_relax_exact(rmt_ctx *ctx, long n, const double *const *psi, double tau, double dt,
                       double *const *out);
/* :119-125 logconf_local_step (strang = 0) or :150-164 logconf_local_step_strang (strang = 1)
 * applied nsteps >= 1 times in one launch: the bits of nsteps calls with nsteps = 1. */
int rmt_ve_logconf_steps(rmt_ctx *ctx, long n, const double *const *psi, const double *const *L,
                         double tau, double dt, int nsteps, int strang, double *const *out);
/* benchmarks/mac_viscoelastic_uniform.py:30-32, :90-92: out3 (device, 3 doubles) = the largest
 * eigenvalue of b over the cells with phi <= 0 (NaN propagates; -inf when there is none), the
 * number of those cells, and b11 at the flat index `at`. */
int rmt_ve_lam_max(rmt_ctx *ctx, long n, const double *const *b, const double *phi, long at,
                   double *out3);

/* ---- the viscoelastic blob in the four-roll mill (benchmarks/mac_viscoelastic_extension.py,
 * mac_ve.hip): what couples the constitutive layer above to the periodic staggered tier.  Planes
 * are the context's (ny, nx) with ny, nx >= 3; face averages wrap, the gradients are the
 * collocated utils.py:5-14 (one-sided at the first and last column / row).  Arithmetic entries
 * give the reference's bits; H (sin), the exact lock (exp) and the FFT solves differ from it to
 * rounding. ---- */
/* :106, :119-120: u_c = 0.5 (u + roll(u, -1, 1)), v_c = 0.5 (v + roll(v, -1, 0)) and
 * L = (d u_c / dx, d u_c / dy, d v_c / dx, d v_c / dy) in one launch.  Six output planes of
 * their own. */
int rmt_mac_ve_centre_kinematics(rmt_ctx *ctx, const double *u, const double *v, double dx,
                                 double dy, double *u_c, double *v_c, double *const *L);
/* :125-131: H = smoothed_heaviside(phi, w_t), S = (1 - H) G be, f_su / f_sv = div S averaged
 * onto the x / y faces, Hu / Hv = H there, chi = 1 - H.  be: three planes (11, 12, 22).  Five
 * output planes of their own. */
int rmt_mac_ve_face_force(rmt_ctx *ctx, const double *const *be, const double *phi, double G,
                          double w_t, double dx, double dy, double *f_su, double *f_sv, double *Hu,
                          double *Hv, double *chi);
/* mac.py:566-579: rhs = u - dt adv + dt f / rho + c_el (1 - chi_face) lap(u), both components
 * (twodx = 2 dx, dx2 = dx^2, ... formed by the caller as the reference forms them). */
int rmt_mac_per_imex_elastic_rhs(rmt_ctx *ctx, const double *u, const double *v, double twodx,
                                 double twody, double dx2, double dy2, double dt, double c_el,
                                 double rho, const double *chi, const double *fu,
                                 const double *fv, double *rhs_u, double *rhs_v);
/* mac.py:560-584 momentum_predictor_periodic_imex_elastic: that right-hand side, then
 * (I - coef Lap) x = rhs per component (coef = dt nu + c_el; lx, ly: host, the per-axis
 * symbol as for rmt_mac_per_solve).  Not in place. */
int rmt_mac_per_predictor_imex_elastic(rmt_ctx *ctx, const double *u, const double *v,
                                       double twodx, double twody, double dx2, double dy2,
                                       double dt, double c_el, double coef, double rho,
                                       const double *chi, const double *fu, const double *fv,
                                       const double *lx, const double *ly, double *u_star,
                                       double *v_star);
/* :139-155 on one component of n faces.  mode 0 (explicit): star + dt (f_s + Hf beta
 * (mill - u)) / rho; mode 1 (imex): mill + (star + dt f_s / rho - mill) exp(-dt beta Hf / rho);
 * mode 2 (imex-elastic): the same without the force (u, f_s may be null where unused).  out
 * may be star. */
int rmt_mac_ve_lock(rmt_ctx *ctx, int mode, long n, const double *star, const double *u,
                    const double *f_s, const double *Hf, const double *mill, double dt,
                    double beta, double rho, double *out);
/* :159-171 as one reduction over n cells: out5 (device, 5 doubles) = the largest eigenvalue
 * of be over phi <= 0 (NaN propagates; -inf when there is none), the number of those cells,
 * be11 at the flat index `at`, max |u| (NaN propagates) and 1.0 if u is all finite, else 0.0. */
int rmt_mac_ve_record(rmt_ctx *ctx, long n, const double *const *be, const double *phi,
                      const double *u, long at, double *out5);

/* The MAC step decomposed into row slabs (config 5 on several GPUs).
 * No reference interface: pyRMT runs mac_multi_disc_lid.py:62-98 in one process.  Slab
 * `rank` of G owns cell rows [row_splits[rank], row_splits[rank+1]) (even, > RMT_SLAB_HALO
 * rows each) and column block [col_splits[rank], col_splits[rank+1]) of the transposed
 * Poisson solve; ctx is the global N x N context.  The caller drives the phases and the
 * collectives between them (order in mac.hip; pyrmt_amd/distributed.py MacDistributedSim).
 * Buffers (rmt_mac_slab_buffer ids): 0 u ((hi-lo) x (N+1)), 1 v ((hi-lo+1) x N, face rows
 * lo..hi), 2 p, 3 X1[disc], 4 X2[disc], 5 phi[disc] ((hi-lo) x N), 6 known bits[disc]
 * (N x W words), 7 rim[disc] (owned cells x 3), 8 A, 9 B (transpose blocks), 10 scalars
 * (RMT_MAC_SLAB_SCALARS doubles: [0] flags 1 non-finite / 2 halo / 4 extrapolation abort,
 * [1] min J, [2] max J, [3] max|u|, [4 + 3k ..] disc k centroid sums (x, y, count),
 * [28 + k] rim count of disc k, [36] row-tree root, [37] cells fitted, [38 + k] 1 if
 * an extrapolation target of disc k in the owned rows fits (0 on every slab: the disc's
 * extrapolation is the identity, rmt_mac_slab_extrapolate_identity replaces the rim
 * allgather + rmt_mac_slab_extrapolate)). */
#define RMT_MAC_SLAB_SCALARS 48
typedef struct rmt_mac_slab rmt_mac_slab;
int rmt_mac_slab_create(rmt_ctx *ctx, const rmt_mac_params *prm, int G, int rank,
                        const int *row_splits, const int *col_splits, rmt_mac_slab **out);
int rmt_mac_slab_destroy(rmt_mac_slab *slab);
int rmt_mac_slab_info(rmt_mac_slab *slab, int *ints8);   /* r0 r1 lo hi c0 c1 W halo */
int rmt_mac_slab_buffer(rmt_mac_slab *slab, int id, int disc, void **dev_ptr);
int rmt_mac_slab_advect(rmt_mac_slab *slab, double dt);
int rmt_mac_slab_rim_pack(rmt_mac_slab *slab);
int rmt_mac_slab_extrapolate(rmt_mac_slab *slab, int disc, const double *gathered_rims,
                             const long long *counts, long long cap);
int rmt_mac_slab_extrapolate_identity(rmt_mac_slab *slab, int disc);
int rmt_mac_slab_predict(rmt_mac_slab *slab, double dt);
int rmt_mac_slab_project_rows(rmt_mac_slab *slab, const double *dev_roots);
int rmt_mac_slab_project_cols(rmt_mac_slab *slab);
int rmt_mac_slab_project_unrows(rmt_mac_slab *slab);
int rmt_mac_slab_correct(rmt_mac_slab *slab, double dt);

#ifdef __cplusplus
}
#endif
#endif /* RMT_H */
