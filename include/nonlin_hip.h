/*
 * nonlin_hip.h -- C ABI of libnonlin_hip.so: the MI355X (gfx950) implementation of
 * nonlin's Jacobian-evaluate + linear-solve inner loop.
 *
 * This is the drop-in boundary.  The reference (jchristopherson/nonlin v2.2.0) is
 * pure Fortran with no C interface; each entry point below replaces one
 * type-bound procedure of the reference and is what a Fortran `bind(C)`
 * interface (nonlin_amd/fortran/) or any other FFI binds to.
 * Signatures use plain pointers, int32_t sizes and doubles only.
 *
 * Conventions
 *   - all matrices are column-major (Fortran order), fp64; integers are int32;
 *     Fortran LOGICALs cross the boundary as int32 0/1;
 *   - "host" entry points take HOST pointers and host callbacks, block until
 *     the result is back in the caller's arrays, and return 0 or the NL_* code
 *     the reference would `error stop` with (the Fortran shim performs the stop);
 *   - "dq" (device-model) entry points take DEVICE pointers (inputs already
 *     resident in HBM), run on the handle's HIP stream and are batched over
 *     independent problems;
 *   - nothing here falls back to a CPU implementation: without a GPU every
 *     compute entry point returns NLH_ERR_NO_DEVICE.
 */
#ifndef NONLIN_HIP_H
#define NONLIN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: src/nonlin_error_handling.f90:10-38 --------------------- */
#define NLH_NO_ERROR                     0
#define NLH_INVALID_INPUT_ERROR        201   /* NL_INVALID_INPUT_ERROR  (:12) */
#define NLH_ARRAY_SIZE_ERROR           202   /* NL_ARRAY_SIZE_ERROR     (:14) */
#define NLH_OUT_OF_MEMORY_ERROR        105   /* = LA_OUT_OF_MEMORY_ERROR (:16), linalg_errors un-vendored */
#define NLH_INVALID_OPERATION_ERROR    104   /* = LA_INVALID_OPERATION_ERROR (:18) */
#define NLH_CONVERGENCE_ERROR          106   /* = LA_CONVERGENCE_ERROR  (:21) */
#define NLH_DIVERGENT_BEHAVIOR_ERROR   206   /* (:23) */
#define NLH_SPURIOUS_CONVERGENCE_ERROR 207   /* (:25) */
#define NLH_TOLERANCE_TOO_SMALL_ERROR  208   /* (:27) */
#define NLH_DIVIDE_BY_ZERO_ERROR       210   /* (:32) */
#define NLH_UNDEFINED_FUNCTION_ERROR   211   /* (:34) */
#define NLH_UNDERDEFINED_PROBLEM_ERROR 212   /* (:37) */
/* Size limits of this implementation (the reference has none); an entry point given a larger problem returns
 * NLH_ARRAY_SIZE_ERROR and touches nothing: quasi-Newton and BFGS n <= 8192 (columns per thread of the single-workgroup
 * rotation kernels); least squares under the opt-in NLH_FACTOR_AUTO / NLH_FACTOR_QR policies n <= 3000 (n-vectors in LDS);
 * the stage-level nlh_lmpar n <= 3358 (its n-vectors in LDS).  Dynamic LDS is capped at 160 KiB - 2 KiB = 161,792 bytes
 * per workgroup; no kernel is launched with more.  Least squares under the default NLH_FACTOR_EXACT policy takes any n <= m
 * (beyond 2902 columns lmpar's n-vectors live in global memory; verified at n = 2903 - 3008), and Newton's LU solve
 * (nlh_newton_solve*, nlh_lu_solve) any n (beyond 13137 its permuted right-hand side and pivots live in global memory;
 * verified at n = 13138 - 13312) -- the solvers' own kernels have no bound in n, but the BUILT-IN
 * dense-quadratic family (the bench / test residual of nlh_dq_*, not part of the reference) keeps a point's x in LDS and
 * stops at n = 20000 (NLH_ARRAY_SIZE_ERROR from its launcher); a user's device function has whatever bound its own kernels
 * have.  Row counts are not limited: polynomial fits and bounded least squares beyond 18000 rows keep the
 * Householder reflector in global memory instead of LDS.  Polynomial roots: order <= 256 (one wave per polynomial on a
 * dense window; the unblocked double-shift QR is not the method for larger orders).
 * The number of problems of a batch is NOT limited: the lock-step drivers carry the problem index in a grid dimension
 * that holds 65535, and a larger batch is solved in slices of 65535 problems, one after the other, inside the entry point
 * (independent problems: the same bits).  The one-variable solvers' batches (brent_solver, newton_1var_solver) carry
 * the problem index in the x dimension and are sliced at 2^28 problems, for their int32 point offsets. */
/* library-level failures (not reference codes) */
#define NLH_ERR_NO_DEVICE             -1
#define NLH_ERR_HIP                   -2
#define NLH_ERR_BAD_HANDLE            -3

/* ---- iteration_behavior: src/nonlin_types.f90:8-29 ------------------------ */
typedef struct nlh_iteration_behavior {
    int32_t iter_count;
    int32_t fcn_count;
    int32_t jacobian_count;
    int32_t gradient_count;
    int32_t converge_on_fcn;        /* logical */
    int32_t converge_on_chng;       /* logical */
    int32_t converge_on_zero_diff;  /* logical */
} nlh_iteration_behavior;

/* ---- solver configuration -------------------------------------------------
 * equation_solver   src/nonlin_multi_eqn_mult_var.f90:67-91 (defaults :69-77)
 * least_squares_solver%m_factor   src/nonlin_least_squares.f90:25, clamp :108-114
 * line_search_solver%m_useLineSearch   src/nonlin_solve.f90:30
 * line_search   src/nonlin_linesearch.f90:35-53                              */
#define NLH_FACTOR_AUTO 0  /* J^T J + pivoted Cholesky; Householder QR when the Gauss-Newton
                              step is rejected or the Gram matrix is ill-conditioned.  Opt-in: within 1e-10 of the
                              reference with exact counts on zero-residual problems (tests/test_gpu_auto_policy.py),
                              at the forward-difference noise level (~1e-7) where a residual remains */
#define NLH_FACTOR_QR   1  /* always the reference's pivoted Householder QR (lmfactor), parallel reductions */
#define NLH_FACTOR_EXACT 2 /* lmfactor/lmpar with every reduction in the reference's operation order
                              (sequential dot products, flang NORM2): bit-identical to the CPU path */
typedef struct nlh_options {
    int32_t max_evals;        /* 100   */
    double  ftol;             /* 1e-8  */
    double  xtol;             /* 1e-12 */
    double  gtol;             /* 1e-12 */
    int32_t print_status;     /* 0     */
    double  factor;           /* 100; setters clamp to [0.1, 100] */
    int32_t use_line_search;  /* 1     */
    int32_t ls_max_evals;     /* 100   */
    double  ls_alpha;         /* 1e-4  */
    double  ls_factor;        /* 0.1   */
    int32_t factor_policy;    /* NLH_FACTOR_EXACT */
    double  ne_pivot_tol;     /* 1e-4: Cholesky pivot / column-norm^2 below this => QR */
    int32_t fuse_fd;          /* 1.  Device-model solves only: 1 = the kernel that evaluates the n perturbed
                                 residuals also forms jac(:,j) = (f_j - f0)/h_j (:274) in its epilogue and the
                                 residual panel is never written; same operations per element, same bits */
    int32_t sub_batches;      /* 0.  Batched device-model LM solves: number of sub-batches kept in flight on private
                                 streams (0 = automatic: nprob / 128, at most 3, and two halves for 32 to 255 problems of
                                 m n >= 65536 elements -- smaller problems have no latency-bound pass to hide and stay one
                                 batch; measurements in nlh_lm.hip, lm_sub_batches; 1 = one lock-step batch).  Results do
                                 not depend on it */
} nlh_options;

void nlh_default_options(nlh_options *opts);

/* print_status (src/nonlin_helper.f90:17-33) as text: the block the solvers print between outer iterations when
 * print_status is set -- a blank line, "Iteration: <I0>", "Function Evaluations: <I0>", "Jacobian Evaluations: <I0>"
 * (only when > 0), "Change in Variable: <E10.3>", "Residual: <E10.3>".  snprintf semantics: returns the length needed. */
int nlh_format_status(int32_t iter, int32_t nfeval, int32_t njaceval, double xnorm, double fnorm, char *buf, int32_t len);

/* ---- user callbacks: vecfcn / jacobianfcn (src/nonlin_multi_eqn_mult_var.f90:14-38)
 * flattened to C.  The Fortran shim passes bind(C) trampolines; ctx carries the
 * vecfcn_helper and the optional class(*) args.  jac is column-major, ld = m. */
/* fcnnvar / gradientfcn (src/nonlin_multi_var.f90:14-27) flattened to C. */
typedef double (*nlh_fcnnvar)(void *ctx, int32_t n, const double *x);
typedef void (*nlh_gradfcn)(void *ctx, int32_t n, const double *x, double *g);
typedef void (*nlh_vecfcn)(void *ctx, int32_t n, const double *x, int32_t m, double *f);
typedef void (*nlh_jacfcn)(void *ctx, int32_t n, const double *x, int32_t m, double *jac);

/* ---- handle: owns a HIP stream reference, device workspaces (cached per shape)
 * and per-kernel HIP-event timers.  Not thread-safe; use one per thread. ---- */
typedef struct nlh_handle nlh_handle;
int  nlh_create(nlh_handle **h, int32_t device, void *hip_stream /* NULL => the default (null) stream */);
void nlh_destroy(nlh_handle *h);
int  nlh_device_count(void);             /* 0 when no GPU is visible */
const char *nlh_last_error(const nlh_handle *h);
const char *nlh_version(void);

/* ===========================================================================
 * Host-callback ("mode H") drop-in entry points: HOST pointers.
 * ======================================================================== */

/* vecfcn_helper%jacobian -- vfh_jac_fcn, src/nonlin_multi_eqn_mult_var.f90:198-277.
 * jacfcn != NULL: forwards to it.  Otherwise evaluates fcn at x + h_j e_j on the
 * host (in the reference's order, x perturbed in place and restored), uploads the
 * m-by-n residual panel and forms jac(:,j) = (f_j - f0)/h_j on the GPU.
 * fv may be NULL (then f0 = fcn(x) is evaluated first, :257-259). */
int nlh_fd_jacobian(nlh_handle *h, int32_t m, int32_t n, nlh_vecfcn fcn, nlh_jacfcn jacfcn,
                    void *ctx, double *x, const double *fv, double *jac);

/* least_squares_solver%solve -- lss_solve, src/nonlin_least_squares.f90:118-391. */
int nlh_lm_solve(nlh_handle *h, const nlh_options *opts, int32_t m, int32_t n,
                 nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx,
                 double *x, double *fvec, nlh_iteration_behavior *ib);

/* newton_solver%solve -- ns_solve, src/nonlin_solve.f90:452-638 (LU step: :570,577). */
int nlh_newton_solve(nlh_handle *h, const nlh_options *opts, int32_t n,
                     nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx,
                     double *x, double *fvec, nlh_iteration_behavior *ib);

/* quasi_newton_solver%solve -- qns_solve, src/nonlin_solve.f90:156-427 (Broyden's method; QR of the
 * Jacobian at :289, rank-one QR update at :307, triangular solve at :327).  jdelta =
 * quasi_newton_solver%m_jDelta (get/set_jacobian_interval, :429-447; default 5, :51). */
int nlh_quasi_newton_solve(nlh_handle *h, const nlh_options *opts, int32_t jdelta, int32_t n,
                           nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx,
                           double *x, double *fvec, nlh_iteration_behavior *ib);

/* constrained_least_squares_solver%solve -- cls_solve, src/nonlin_least_squares.f90:938-1176 (bounded
 * trust-region dog-leg: qr_factor :1047, coleman_li_scaling :1050, dogleg :1053/1301-1403, Armijo
 * fallback :1088-1123).  delta0 = get_trust_region_radius() (default 1, :60), stepscale0 =
 * get_step_scaling_factor() (default 1, :61); xl / xu = get_lower_limits() / get_upper_limits()
 * ([n] host arrays, NULL = unbounded, :999-1009). */
int nlh_cls_solve(nlh_handle *h, const nlh_options *opts, double delta0, double stepscale0,
                  const double *xl, const double *xu, int32_t m, int32_t n,
                  nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx,
                  double *x, double *fvec, nlh_iteration_behavior *ib);

/* fcnnvar_helper%gradient -- fnh_grad_fcn, src/nonlin_multi_var.f90:182-246.  gradfcn != NULL: the user's gradient.
 * Otherwise forward differences: g_j = (f(x + h_j e_j) - f(x)) / h_j, h_j = sqrt(eps) |x_j| (sqrt(eps) when x_j = 0),
 * callbacks in ascending j on the calling thread; x is perturbed and restored; fv = NULL => f(x) is evaluated first.
 * Host arrays; needs no handle (n + 1 calls of a host function and nothing else). */
int nlh_fd_gradient(int32_t n, nlh_fcnnvar fcn, nlh_gradfcn gradfcn, void *ctx, double *x, const double *fv, double *g);

/* bfgs%solve -- bfgs_solve, src/nonlin_optimize.f90:557-770, with fcnnvar_helper%gradient
 * (src/nonlin_multi_var.f90:182-246; gradfcn = NULL => forward differences) and ls_search_miso
 * (src/nonlin_linesearch.f90:329-492).  opts->max_evals = get_max_fcn_evals() (500, :46),
 * opts->gtol = get_tolerance() (1e-12, :47), opts->xtol = get_var_tolerance() (1e-12,
 * src/nonlin_optimize.f90:47), use_line_search / ls_* as for newton.  fout may be NULL.
 * ib->gradient_count is filled, ib->jacobian_count = 0. */
int nlh_bfgs_solve(nlh_handle *h, const nlh_options *opts, int32_t n, nlh_fcnnvar fcn,
                   nlh_gradfcn gradfcn, void *ctx, double *x, double *fout,
                   nlh_iteration_behavior *ib);

/* ===========================================================================
 * Device-model ("mode D") batched entry points: DEVICE pointers.
 * Residual family "dense-quadratic" (SURVEY.md 8(d)), evaluated on the GPU with
 * the exact per-row operation order of the CPU path:
 *   u_i = sum_j A(i,j) x_j  (j ascending, separate multiply and add)
 *   r_i = (u_i + (gamma*u_i)*u_i) - b_i ;   dr_i/dx_j = (1 + 2 gamma u_i) A(i,j)
 * Layout: A [nprob][n][m] (each problem column-major m-by-n), b/fvec [nprob][m],
 * x [nprob][n].  Problems are independent; status[k] receives 0 or an NL_* code.
 * ======================================================================== */
int nlh_dq_lm_solve_batch(nlh_handle *h, const nlh_options *opts, int32_t nprob,
                          int32_t m, int32_t n, const double *dA, const double *db,
                          double gamma, double *dx, double *dfvec,
                          nlh_iteration_behavior *ib /* host, [nprob] */,
                          int32_t *status /* host, [nprob] */);

int nlh_dq_newton_solve_batch(nlh_handle *h, const nlh_options *opts, int32_t nprob,
                              int32_t n, const double *dA, const double *db, double gamma,
                              int32_t analytic_jacobian, double *dx, double *dfvec,
                              nlh_iteration_behavior *ib, int32_t *status);

int nlh_dq_quasi_newton_solve_batch(nlh_handle *h, const nlh_options *opts, int32_t jdelta,
                                    int32_t nprob, int32_t n, const double *dA, const double *db,
                                    double gamma, int32_t analytic, double *dx, double *dfvec,
                                    nlh_iteration_behavior *ib /* host, [nprob] */,
                                    int32_t *status /* host, [nprob] */);

/* xl / xu: [n] host arrays shared by every problem, or NULL. */
int nlh_dq_cls_solve_batch(nlh_handle *h, const nlh_options *opts, double delta0, double stepscale0,
                           const double *xl, const double *xu, int32_t nprob, int32_t m, int32_t n,
                           const double *dA, const double *db, double gamma, double *dx,
                           double *dfvec, nlh_iteration_behavior *ib /* host, [nprob] */,
                           int32_t *status /* host, [nprob] */);

/* bfgs on f(x) = 0.5 * sum_i r_i(x)^2 of the device model, forward-difference gradient on the device.
 * hfout: [nprob] host (may be NULL). */
int nlh_dq_bfgs_solve_batch(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t m,
                            int32_t n, const double *dA, const double *db, double gamma, double *dx,
                            double *hfout, nlh_iteration_behavior *ib /* host, [nprob] */,
                            int32_t *status /* host, [nprob] */);

/* ---- device residual models behind HOST arrays (no reference counterpart: the extension of vecfcn_helper that lets
 * `solver%solve` reach the batched device path -- nonlin_amd/fortran: vecfcn_helper%set_device_model, device_model_batch,
 * least_squares_solver%solve_batch).  A model owns device copies of nprob problems of the dense-quadratic family
 * r = (u + gamma u u) - b, u = A x: A [nprob][n][m] (each problem column-major m x n), b [nprob][m].
 * x [nprob][n] in/out and fvec [nprob][m] out are host arrays; status[p] = 0 or the NL_* code the reference would stop
 * with for problem p (no process abort). ---- */
typedef struct nlh_dq_model nlh_dq_model;
int  nlh_dq_model_create(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *A, const double *b,
                         double gamma, nlh_dq_model **model);

/* ---- several GPUs behind the boundary (SURVEY.md 8(b) `nlx_init(device, comm)`, 8(e); replaces nothing in the
 * reference, whose solvers are single-threaded -- this is how `solver%solve_batch` reaches every GPU of the node from ONE
 * process).  A device set owns one handle (own stream, own workspaces) per entry of its device list.  A model created
 * ON a set is dealt over the entries block-cyclically (problem k -> entry k mod ndev: iteration counts differ per
 * problem), and every nlh_dq_model_* call on it runs one host thread per entry: independent problems, no collective,
 * the same bits as on one device.  devices == NULL or ndev <= 0: every visible device; an id may repeat (two shares
 * on one GPU).  The handle argument of nlh_dq_model_eval / _lm_solve / _newton_solve is ignored (may be NULL) for a
 * model created on a set.  (One process per GPU over RCCL is the other way to use several GPUs: nonlin_amd/sharding.py,
 * bench.py --gpus N.) ---- */
typedef struct nlh_device_set nlh_device_set;
int  nlh_device_set_create(nlh_device_set **set, const int32_t *devices, int32_t ndev);
void nlh_device_set_destroy(nlh_device_set *set);
int32_t nlh_device_set_size(const nlh_device_set *set);
nlh_handle *nlh_device_set_handle(nlh_device_set *set, int32_t i);        /* entry i's handle (owned by the set) */
const char *nlh_device_set_last_error(const nlh_device_set *set);
int  nlh_dq_model_create_on(nlh_device_set *set, int32_t nprob, int32_t m, int32_t n, const double *A, const double *b,
                            double gamma, nlh_dq_model **model);
int32_t nlh_dq_model_device_count(const nlh_dq_model *model);             /* shares the model is dealt into */
void nlh_dq_model_destroy(nlh_dq_model *model);
void nlh_dq_model_shape(const nlh_dq_model *model, int32_t *nprob, int32_t *m, int32_t *n);
/* vecfcn (src/nonlin_multi_eqn_mult_var.f90:14-25) of the model, every problem */
int  nlh_dq_model_eval(nlh_handle *h, const nlh_dq_model *model, const double *x, double *f);
/* lss_solve (src/nonlin_least_squares.f90:118-391) / ns_solve (src/nonlin_solve.f90:452-638) on every problem */
int  nlh_dq_model_lm_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, double *x, double *fvec,
                           nlh_iteration_behavior *ib, int32_t *status);
int  nlh_dq_model_newton_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, int32_t analytic,
                               double *x, double *fvec, nlh_iteration_behavior *ib, int32_t *status);
/* The same for quasi_newton_solver%solve (src/nonlin_solve.f90:156-427; jdelta: iterations between fresh Jacobians),
 * constrained_least_squares_solver%solve (src/nonlin_least_squares.f90:938-1176; xl / xu: n entries or NULL, one box for
 * every problem) and bfgs%solve on 0.5 ||F(x)||^2 (src/nonlin_optimize.f90:557-770; fout [nprob]: the objective at the
 * solution, fvec: F there).  Each runs the lock-step device state machine of its solver on every share of the model. */
int  nlh_dq_model_quasi_newton_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, int32_t jdelta,
                                     int32_t analytic, double *x, double *fvec, nlh_iteration_behavior *ib, int32_t *status);
int  nlh_dq_model_cls_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, double delta0,
                            double stepscale0, const double *xl, const double *xu, double *x, double *fvec,
                            nlh_iteration_behavior *ib, int32_t *status);
int  nlh_dq_model_bfgs_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, double *x, double *fvec,
                             double *fout, nlh_iteration_behavior *ib, int32_t *status);


/* ===========================================================================
 * User-supplied DEVICE residuals: vecfcn / jacobianfcn as LAUNCHERS.
 *
 * The reference's plugin layer is "the user hands in a residual": vecfcn (src/nonlin_multi_eqn_mult_var.f90:14-25),
 * set_fcn (:126-140), and the solvers call it at x, at the n perturbed points of the forward-difference Jacobian
 * (:267-273) and at trial points.  A host procedure cannot run on the GPU, so the device form of the plugin is a
 * launcher: a HOST function that ENQUEUES, on the HIP stream it is handed, device work which evaluates F at `npoints`
 * points, and returns at once (0, or non-zero to abort the solve with NLH_ERR_HIP).  It must not synchronise and may be
 * called from several host threads on different streams (sub-batches, device sets).
 *   point q (0 <= q < npoints) belongs to problem dprob[q] (a DEVICE array: the index the problem has in the caller's
 *   batch -- what the user's kernel selects its data with); its variables are dX[q*n .. q*n + n), its residuals go to
 *   dF[q*m .. q*m + m).  For the Jacobian launcher point q's m-by-n Jacobian goes to dJ + q*m*n, column-major (ld = m).
 * The library builds the points itself, on the device, in the reference's order: for a forward-difference Jacobian of
 * problem p, points p*n + j = x with x(j) replaced by x(j) + h_j (:268-271); k_fd_jacobian then forms
 * jac(:,j) = (F(point j) - F(x)) / h_j with a true division (:274).  Everything downstream is the state machine the
 * dense-quadratic entry points run.  A problem's result does not depend on the batch it is solved in.
 * ======================================================================== */
typedef int (*nlh_device_vecfcn)(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n,
                                 const double *dX, int32_t m, double *dF);
typedef int (*nlh_device_jacfcn)(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n,
                                 const double *dX, int32_t m, double *dJ);

/* vecfcn_helper%jacobian (vfh_jac_fcn, :198-277) of every problem: jacfcn != NULL forwards to it (:241-243), otherwise
 * forward differences.  dx [nprob][n], dfv [nprob][m] = F(x) or NULL (then evaluated first, :257-259), dJ [nprob][n][m]
 * (each problem column-major m x n); DEVICE pointers. */
int nlh_fd_jacobian_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                           nlh_device_jacfcn jacfcn, void *ctx, const double *dx, const double *dfv, double *dJ);
/* least_squares_solver%solve (lss_solve, src/nonlin_least_squares.f90:118-391) on nprob problems of the user's family.
 * dx [nprob][n] in/out, dfvec [nprob][m] out: DEVICE pointers; ib / status: host, [nprob] (NULL allowed). */
int nlh_lm_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t m, int32_t n,
                              nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *dx, double *dfvec,
                              nlh_iteration_behavior *ib, int32_t *status);
/* newton_solver%solve (ns_solve, src/nonlin_solve.f90:452-638) / quasi_newton_solver%solve (qns_solve, :156-427) on
 * nprob square problems of the user's family. */
int nlh_newton_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t n,
                                  nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *dx, double *dfvec,
                                  nlh_iteration_behavior *ib, int32_t *status);
int nlh_quasi_newton_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t jdelta, int32_t nprob, int32_t n,
                                        nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *dx,
                                        double *dfvec, nlh_iteration_behavior *ib, int32_t *status);
/* constrained_least_squares_solver%solve (cls_solve, src/nonlin_least_squares.f90:938-1176) on the user's family; xl / xu:
 * [n] host arrays shared by every problem, or NULL (as nlh_dq_cls_solve_batch). */
int nlh_cls_solve_batch_device(nlh_handle *h, const nlh_options *opts, double delta0, double stepscale0, const double *xl,
                               const double *xu, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                               nlh_device_jacfcn jacfcn, void *ctx, double *dx, double *dfvec, nlh_iteration_behavior *ib,
                               int32_t *status);
int nlh_cls_solve_batch_device_h(nlh_handle *h, const nlh_options *opts, double delta0, double stepscale0, const double *xl,
                                 const double *xu, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                 nlh_device_jacfcn jacfcn, void *ctx, double *x, double *fvec, nlh_iteration_behavior *ib,
                                 int32_t *status);
/* bfgs%solve (src/nonlin_optimize.f90:557-770) on a batch of problems whose objective is the USER'S device fcnnvar
 * (reference plugin: fcnnvar_helper, src/nonlin_multi_var.f90:17-44, 93-104 set_fcn, 182-246 gradient): the launcher is an
 * nlh_device_vecfcn called with m = 1 -- dF[npoints] receives f at each of the npoints points --, gradfcn (NULL: forward
 * differences, n more points per gradient, built on the device in the reference's order :231-243) an nlh_device_jacfcn
 * called with m = 1 -- dJ[npoints][n] receives the gradients (set_gradient_fcn, :126-138).  dx [nprob][n] device, in/out;
 * fout [nprob] host (NULL allowed): f at the solution (:762).  Counts, flags and errors per problem as nlh_bfgs_solve. */
int nlh_bfgs_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t n, nlh_device_vecfcn fcn,
                                nlh_device_jacfcn gradfcn, void *ctx, double *dx, double *fout, nlh_iteration_behavior *ib,
                                int32_t *status);
/* ... with x [nprob][n] a HOST array. */
int nlh_bfgs_solve_batch_device_h(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t n, nlh_device_vecfcn fcn,
                                  nlh_device_jacfcn gradfcn, void *ctx, double *x, double *fout, nlh_iteration_behavior *ib,
                                  int32_t *status);
/* nelder_mead%solve -- nm_solve, src/nonlin_optimize.f90:104-340 (nm_extrapolate :343-399).  opts->max_evals =
 * get_max_fcn_evals() (500, src/nonlin_multi_var.f90:62-66), opts->gtol = get_tolerance() (1e-12), opts->print_status (the
 * block of :306-313 after every iteration); the other options are not read.  init_size: m_initSize (1.0).  simplex: [n+1][n]
 * host (vertex-major: the reference's ndim x npts column-major matrix) or NULL; use_simplex = 1 starts from it (x is
 * ignored), 0 builds it from x and init_size (:183-213); when non-NULL the final simplex is written back, so a second call
 * with use_simplex = 1 continues where the first stopped, as the reference's object state does.  fout may be NULL.
 * Returns 0 (x = the best vertex, :258-266) or NLH_CONVERGENCE_ERROR after max_evals (x untouched, fout = f of the initial
 * vertex 1: :220, :316-337).  ib: iter_count counts the final convergence check (:230); fcn_count grows by n + 1 per shrink
 * although a shrink evaluates n points (:299).  The callback runs on the calling thread; the simplex logic runs on the
 * device (the machine of nlh_nelder_mead_solve_batch_device with one problem). */
int nlh_nelder_mead_solve(nlh_handle *h, const nlh_options *opts, double init_size, int32_t n, nlh_fcnnvar fcn, void *ctx,
                          double *x, double *simplex, int32_t use_simplex, double *fout, nlh_iteration_behavior *ib);
/* ... on nprob problems of the USER'S device fcnnvar (an nlh_device_vecfcn called with m = 1: dF[npoints] = f at each
 * point; a round asks for the points of every problem at once, in ascending problem order).  dx [nprob][n] and dsimplex
 * [nprob][n+1][n] (or NULL: the library's own) DEVICE; fout / ib / status host [nprob] (NULL allowed); status[p] = 0 or
 * NLH_CONVERGENCE_ERROR.  print_status is not honoured.  A problem's bits do not depend on the batch it is solved in. */
int nlh_nelder_mead_solve_batch_device(nlh_handle *h, const nlh_options *opts, double init_size, int32_t nprob, int32_t n,
                                       nlh_device_vecfcn fcn, void *ctx, double *dx, double *dsimplex, int32_t use_simplex,
                                       double *fout, nlh_iteration_behavior *ib, int32_t *status);
/* ... on a model of ONE function made by nlh_device_fcn_model_create (m = 1), host x [nprob][n] in/out, simplex built from
 * x: what the Fortran shim's nelder_mead%solve_batch calls.  A dense-quadratic model or m > 1: NLH_INVALID_OPERATION_ERROR. */
int nlh_dq_model_nelder_mead_solve(nlh_handle *h, const nlh_options *opts, double init_size, const nlh_dq_model *model,
                                   double *x, double *fout, nlh_iteration_behavior *ib, int32_t *status);
/* ---- equations of one variable: nonlin_single_var (src/nonlin_single_var.f90) + brent_solver / newton_1var_solver.
 * fcn1var (:10-22) is an nlh_fcnnvar called with n = 1; fcn1var_helper%diff's user derivative (:154-200) likewise.
 * equation_solver_1var's defaults (:45-54) are nlh_options' own: max_evals = get_max_fcn_evals() (100), ftol =
 * get_fcn_tolerance() (1e-8), xtol = get_var_tolerance() (1e-12), gtol = get_diff_tolerance() (1e-12), print_status =
 * get_print_status() (0); the other options are not read.  x1, x2: value_pair lim (src/nonlin_types.f90:31-36), in
 * either order (both solvers sort them).  Returns 0, NLH_CONVERGENCE_ERROR (max_evals reached), NLH_INVALID_INPUT_ERROR
 * (|x1 - x2| < epsilon, absolute: nothing is evaluated) or NLH_UNDEFINED_FUNCTION_ERROR (fcn NULL) -- the codes the
 * reference error-stops with.  The callbacks run in list order on the calling thread; the solver's statements run on the
 * device (the machine of the batch forms with one problem).  print_status prints the reference's blocks to stdout. */
/* brent_solver%solve -- brent_solve, src/nonlin_solve.f90:643-835.  x is set to 0 before the input check (:691) and
 * written only on convergence (:746, :751): a max-evaluations stop returns x = 0, f = fb and NLH_CONVERGENCE_ERROR.  f
 * (NULL allowed) = fb (:820), 0 on invalid input.  ib: jacobian_count 0.  The a == c test is |a - c| < epsilon (:761);
 * sign(tol1, xm) follows the sign of a negative zero (:802); status is printed after every evaluation, the last included
 * (:808-810).  The first pass reads c, d and e unset when both sign tests of :726-727 fail -- fb == 0 exactly (reachable
 * only with ftol <= 0) or fb NaN: they are 0. */
int nlh_brent_solve(nlh_handle *h, const nlh_options *opts, nlh_fcnnvar fcn, void *ctx, double x1, double x2, double *x,
                    double *f, nlh_iteration_behavior *ib);
/* newton_1var_solver%solve -- newt1var_solve, src/nonlin_solve.f90:840-1032.  diff: the user's derivative, or NULL for
 * f1h_diff_fcn's forward difference (h = sqrt(eps)|x|, sqrt(eps) when h < eps; f at x + h is evaluated and NOT counted;
 * f' = (f(x + h) - f(x)) / h).  Every f + f' pair counts one evaluation and one derivative (ib->jacobian_count).  An
 * endpoint with |f| < ftol returns at once: x = it, f = its value, fcn_count = 2, iter_count = 0, converge_on_fcn
 * (:906-923).  The bisection / Newton-step exits (:953, :964) leave without evaluating at the new x.  f != NULL is the
 * reference's "f present": one more evaluation at the final x, counted, its value discarded, f = the last ff
 * (:1011-1017); f == NULL skips it.  Status is printed only on iterations that pass every test (:999-1001).  On invalid
 * input x is left untouched. */
int nlh_newton_1var_solve(nlh_handle *h, const nlh_options *opts, nlh_fcnnvar fcn, nlh_fcnnvar diff, void *ctx, double x1,
                          double x2, double *x, double *f, nlh_iteration_behavior *ib);
/* ... on nprob problems of the USER'S device fcn1var: an nlh_device_vecfcn called with n = 1, m = 1 (dF[q] = f at point
 * dX[q]); newton's diff (NULL: forward differences, x and x + h in one round) an nlh_device_jacfcn with n = m = 1 (dJ[q]
 * = f' at dX[q]), called once per round after fcn on the same list (entries of points that need no derivative -- a
 * final evaluation -- are ignored).  A round asks every live problem for its points at once, in ascending problem
 * order: brent 2 (a, b) then 1; newton 2 (x1, x2), then 2 per iteration (x, x + h) or 1 with diff, and 1 for the final
 * evaluation when fout != NULL.  dlim [nprob][2], dx [nprob]: DEVICE; fout / ib / status: host [nprob], NULL allowed;
 * fout != NULL is newton's "f present".  status[p] = 0, NLH_CONVERGENCE_ERROR or NLH_INVALID_INPUT_ERROR (a bad bracket
 * in the batch: that problem evaluates nothing; the others are solved).  Any nprob (slices of 2^28 problems: int32
 * point offsets); print_status is not honoured.  A problem's bits do not depend on the batch it is solved in. */
int nlh_brent_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t nprob, nlh_device_vecfcn fcn, void *ctx,
                                 const double *dlim, double *dx, double *fout, nlh_iteration_behavior *ib, int32_t *status);
int nlh_newton_1var_solve_batch_device(nlh_handle *h, const nlh_options *opts, int32_t nprob, nlh_device_vecfcn fcn,
                                       nlh_device_jacfcn diff, void *ctx, const double *dlim, double *dx, double *fout,
                                       nlh_iteration_behavior *ib, int32_t *status);
/* ... on a model made by nlh_device_fcn_model_create with n = m = 1 (its jacfcn, if any, is newton's derivative), host
 * lim [nprob][2] and x [nprob]: what the Fortran shim's solve_batch calls.  n != 1, m != 1 or a dense-quadratic model:
 * NLH_INVALID_OPERATION_ERROR. */
int nlh_dq_model_brent_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, const double *lim, double *x,
                             double *fout, nlh_iteration_behavior *ib, int32_t *status);
int nlh_dq_model_newton_1var_solve(nlh_handle *h, const nlh_options *opts, const nlh_dq_model *model, const double *lim,
                                   double *x, double *fout, nlh_iteration_behavior *ib, int32_t *status);
/* fcn1var_helper%diff -- f1h_diff_fcn, src/nonlin_single_var.f90:154-200: diff != NULL returns diff(x); otherwise the
 * forward difference: f at x + h first, then f at x unless fv (f(x)) is given, df = (f(x + h) - f0) / h.  Host
 * callbacks; needs no handle (like nlh_fd_gradient). */
int nlh_fd_derivative(nlh_fcnnvar fcn, nlh_fcnnvar diff, void *ctx, double x, const double *fv, double *df);
/* The same three behind HOST arrays x [nprob][n] in/out, fvec [nprob][m] out (what the Fortran shim's
 * vecfcn_helper%set_device_fcn + solver%solve / solve_batch call): staged through the handle's buffers. */
int nlh_lm_solve_batch_device_h(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t m, int32_t n,
                                nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *x, double *fvec,
                                nlh_iteration_behavior *ib, int32_t *status);
int nlh_newton_solve_batch_device_h(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t n,
                                    nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *x, double *fvec,
                                    nlh_iteration_behavior *ib, int32_t *status);
int nlh_quasi_newton_solve_batch_device_h(nlh_handle *h, const nlh_options *opts, int32_t jdelta, int32_t nprob, int32_t n,
                                          nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *x,
                                          double *fvec, nlh_iteration_behavior *ib, int32_t *status);
/* The built-in dense-quadratic family expressed as such launchers (ctx = nlh_dq_device_ctx): the same residual bits as
 * the nlh_dq_* entry points, through the open path. */
typedef struct nlh_dq_device_ctx {
    const double *dA;     /* [nprob][n][m], device */
    const double *db;     /* [nprob][m], device */
    double gamma;
} nlh_dq_device_ctx;
int nlh_dq_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                      int32_t m, double *dF);
int nlh_dq_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                      int32_t m, double *dJ);

/* A user's device residual as a MODEL object (what the Fortran shim's vecfcn_helper%set_device_fcn and
 * device_model_batch%create_from_device_fcn hold): nprob problems of m equations in n unknowns each, evaluated by the
 * launchers; nlh_dq_model_eval / _lm_solve / _newton_solve / _quasi_newton_solve accept it (host arrays, the caller's
 * handle; `analytic` selects the jacobianfcn launcher) and so does nlh_dq_model_cls_solve; the bfgs form takes a model of
 * ONE function (m = 1: the launcher is the user's fcnnvar, the jacobianfcn launcher its gradient -- nlh_bfgs_solve_batch_device)
 * and returns NLH_INVALID_OPERATION_ERROR for m > 1 (bfgs minimises a scalar fcnnvar, not a vecfcn).  Lives on the handle's device (not dealt over a device set: the user's data is wherever the
 * user put it).  Freed with nlh_dq_model_destroy; ctx stays the caller's. */
int nlh_device_fcn_model_create(int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx,
                                nlh_dq_model **model);

/* Synthetic problem generator of SURVEY.md 8(d) (bench/test inputs, not part of the
 * reference): counter-based splitmix64, U_k = mix(seed + (k+1)*0x9E3779B97F4A7C15),
 * draw order A (column-major), x_true, noise, x0; problem p uses seed0 + p*seed_stride.
 * A = (2U-1)/sqrt(n) (+2I when square_shift), b = model(x_true) + sigma(2U-1),
 * x0 = x_true + spread(2U-1).  All pointers are DEVICE pointers. */
int nlh_dq_generate(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, uint64_t seed0,
                    uint64_t seed_stride, double gamma, double sigma, double spread, int32_t square_shift,
                    double *dA, double *db, double *dxtrue, double *dx0);

/* ---- stage-level entry points (each is one kernel family of the path; used by
 * the parity tests and the roofline measurement).  DEVICE pointers. ---------- */

/* vecfcn for the dense-quadratic model: f = F(x) for every problem. */
int nlh_dq_residual(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dA,
                    const double *db, double gamma, const double *dx, double *df);
/* The n perturbed evaluations of vfh_jac_fcn (:267-273): P(:,j) = F(x + h_j e_j). */
int nlh_dq_fd_panel(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dA,
                    const double *db, double gamma, const double *dx, double *dP);
/* The forward-difference column write (:274): J(:,j) = (P(:,j) - f0)/h_j,
 * h_j = sqrt(eps)*|x_j| (sqrt(eps) if zero).  HBM-bound streaming kernel. */
int nlh_fd_jacobian_panel(nlh_handle *h, int32_t nprob, int32_t m, int32_t n,
                          const double *dP, const double *df0, const double *dx, double *dJ);
/* Analytic jacobianfcn of the dense-quadratic model. */
int nlh_dq_jacobian(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dA,
                    double gamma, const double *dx, double *dJ);
/* J^T J (fp64 MFMA, deterministic split-K) and J^T f.  dG [nprob][n][n], dg [nprob][n]. */
int nlh_gram(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dJ,
             const double *df, double *dG, double *dg);
/* Which kernel form nlh_gram (and the normal-equations policy) takes for an m-by-n problem, and its K-split count:
 * host code only -- no handle, no device -- the very function the launch dispatches through, under the process's
 * NLH_GRAM512 / NLH_GRAM_TRI environment as it is at the call.  Form and split count depend on the
 * shape only, never on the batch; forms never change a bit of G.  Returns the form; *nsplit (may be NULL) = K-splits;
 * *direct (may be NULL) = 1 when the kernel writes G and g in place and no reduce is launched (a triangle form with one
 * split).  -NLH_INVALID_INPUT_ERROR for m < 1 or n < 1. */
enum { NLH_GRAM_FORM_BLOCK = 0,    /* k_gram_mfma: a workgroup per 64 x 64 block of the lower block triangle */
       NLH_GRAM_FORM_TRI8 = 1,     /* k_gram_tri<8>: 96 < n <= 128, the whole lower triangle in one workgroup */
       NLH_GRAM_FORM_TRI16 = 2,    /* k_gram_tri<16>: 224 < n <= 256 */
       NLH_GRAM_FORM_512 = 3 };    /* k_gram_512: 256 < n <= 512, four workgroups per (problem, K-split) */
int32_t nlh_gram_plan(int32_t m, int32_t n, int32_t *nsplit, int32_t *direct);
/* lmfactor replacement on the Gram matrix: pivoted Cholesky P^T G P = R^T R with
 * MINPACK's pivot rule, acnorm = sqrt(diag G), qtf = R^-T P^T g.  dG is overwritten
 * by R (upper triangle).  ipvt is 0-based.  info[k] != 0 => ill-conditioned/rank-deficient. */
int nlh_chol_factor(nlh_handle *h, int32_t nprob, int32_t n, double *dG, const double *dg,
                    int32_t *dipvt, double *dacnorm, double *dqtf, int32_t *dinfo);
/* The natural-order (unpivoted) blocked Cholesky of the NLH_FACTOR_AUTO policy on caller-supplied G [nprob][n][n] and
 * g [nprob][n] (a test entry point: the solver's own launches).  form 0: one workgroup per problem, n <= 1109; form 1: the
 * multi-CU launches, 192 <= n <= 1109; other sizes return NLH_ARRAY_SIZE_ERROR and launch nothing.  dR [nprob][n][n]
 * receives G with its upper triangle overwritten by R (G = R^T R), dqtf = R^-T g, dacnorm = sqrt(diag G), dipvt the
 * identity (0-based).  dinfo[k] = 0, or the 1-based index of the first pivot d with !(d > pivot_tol * acnorm^2) or
 * !(d > 0); R and qtf of such a problem are unfinished. */
int nlh_chol_natural(nlh_handle *h, int32_t nprob, int32_t n, const double *dG, const double *dg, double pivot_tol,
                     int32_t form, double *dR, int32_t *dipvt, double *dacnorm, double *dqtf, int32_t *dinfo);
/* Row signs of lmfactor for pivoted Cholesky factors (a test entry point: the solver's sign recovery before lmpar's
 * iteration).  dJ [nprob][n][m] column-major (m >= n, not modified), dipvt 0-based as nlh_chol_factor leaves it, dR
 * [nprob][n][n] and dqtf [nprob][n] the factors: on return R = S R~, qtf = S qtf~, dsign [nprob][n] = diag S (+-1). */
int nlh_ne_signs(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dJ, const int32_t *dipvt,
                 double *dR, double *dqtf, double *dsign);
/* lmfactor itself (pivoted Householder QR, src/nonlin_least_squares.f90:569-667) plus
 * Q^T f (:241-253).  dJ is overwritten as in the reference (R strict upper, reflectors
 * below, diagonal restored to rdiag after Q^T f); dqtf [nprob][n]; dwa4 [nprob][m]. */
int nlh_qr_factor(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, double *dJ,
                  const double *df, int32_t *dipvt, double *drdiag, double *dacnorm,
                  double *dqtf, double *dwa4);
/* The same factorisation in the reference's OPERATION ORDER (what NLH_FACTOR_EXACT runs inside the LM solve:
 * streaming lock-step Householder steps, nlh_qrx.hip): bit-identical to the CPU path.  dJ [nprob][n][m] is not
 * modified; dR [nprob][n][n] column-major receives R (strict upper triangle + diagonal = rdiag); requires m >= n. */
int nlh_lmfactor_exact(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *dJ,
                       const double *df, double *dR, int32_t *dipvt, double *drdiag, double *dacnorm,
                       double *dqtf, double *dwa4);
/* The launch plan of that factorisation: which kernels run at each of its n Householder steps for a batch of nprob
 * m-by-n problems of which nact are expected to need factoring (<= 0: all; the LM solve passes its count, with
 * have_stages = 1 for its per-problem stages).  Host code only -- no handle, no device -- walking the very stepper the
 * factorisation walks, under the process's NLH_QRX_* environment.  Forms never change a result bit. */
enum { NLH_QRX_SWEEP_COLUMN = 0,   /* a workgroup per trailing column, the update one step behind (a handful of problems) */
       NLH_QRX_SWEEP_LANE = 1 };   /* a lane per trailing column, updates deferred to a flush every few steps */
enum { NLH_QRX_INIT_SPLIT = 0,     /* initial column norms by a workgroup per column, in a launch of their own */
       NLH_QRX_INIT_FUSED = 1 };   /* ... by a thread per column inside the init kernel */
enum { NLH_QRX_PIVOT_FEW32 = 0,        /* k_qrx_pivot<32, false, true>: m <= 2048, a workgroup has its CU to itself */
       NLH_QRX_PIVOT_BATCH32 = 1,      /* k_qrx_pivot<32>: four workgroups per CU */
       NLH_QRX_PIVOT_FEW64 = 2,        /* k_qrx_pivot<64, false, true>: 4096-row NORM2 chunks, CU to itself */
       NLH_QRX_PIVOT_BATCH64 = 3,      /* k_qrx_pivot<64> */
       NLH_QRX_PIVOT_LONG = 4,         /* k_qrx_pivot<64, true>: columns of several chunks, pipelined NORM2, one launch */
       NLH_QRX_PIVOT_LONG_SCALED = 5,  /* ... with the scaling of the reflector as a chip-wide launch of its own */
       NLH_QRX_PIVOT_LONG_SPLIT = 6 }; /* ... and the gather too: search, gather, NORM2, scaling as four launches */
enum { NLH_QRX_PASS_COLUMN = 0,        /* k_qrx_pass_col (the column sweep) */
       NLH_QRX_PASS_WIDE = 1,          /* k_qrx_pass_rpw: sixteen waves per 64-column window, row-parallel */
       NLH_QRX_PASS_WIDE_HALF = 2,     /* ... per 32-column half window */
       NLH_QRX_PASS_FOUR_WAVE = 3,     /* k_qrx_pass_rp: four waves per window, row-parallel */
       NLH_QRX_PASS_WAVE = 4,          /* k_qrx_pass: one wave per window, a workgroup each */
       NLH_QRX_PASS_WAVE_SHARED = 5 }; /* ... the windows of a problem as the waves of one workgroup */
typedef struct nlh_qrx_plan_head {
    int32_t sweep, init;      /* NLH_QRX_SWEEP_*, NLH_QRX_INIT_* */
    int32_t use_list, ny;     /* (problem, column) grids cover a compacted list of the ny problems that work, not the batch */
    int32_t nact;             /* the count the plan was made for */
} nlh_qrx_plan_head;
typedef struct nlh_qrx_plan_step {
    int32_t j, cur, np;       /* step, reflector bank, pending reflectors when the step starts */
    int32_t lo;               /* lane sweep: first slot that can still hold live data (moves at a flush); column sweep: 0 */
    int32_t flush, pf;        /* the pass writes the columns back and switches banks; the pivot kernel's flags
                                 (1: this step's pass flushes, 2: the pass before did) */
    int32_t pivot, pass;      /* NLH_QRX_PIVOT_*, NLH_QRX_PASS_*: the forms that are launched */
    int32_t gwin;             /* what the pass's grid is built from, per problem: 64-column windows (wide_half: 32-column
                                 half windows, column: trailing columns) */
    int32_t lds, lds_max;     /* dynamic LDS bytes of the pass launch, and what its kernel is allowed */
    int32_t tcur, oop;        /* the copy of the working matrix (0 / 1) the step's kernels read; 1: the flush writes the OTHER
                                 copy, which the next step reads (wave / wave_shared under NLH_QRX_OOP != 0; a factorisation
                                 whose second copy could not be allocated flushes in place instead, same results) */
} nlh_qrx_plan_step;
/* Fills *head and steps[0 .. min(n, cap)) (either may be NULL); returns n, -NLH_INVALID_INPUT_ERROR for nprob < 1,
 * n < 1 or m < n, -NLH_INVALID_OPERATION_ERROR for a plan no kernel instance exists for (a defect of the library). */
int32_t nlh_qrx_plan(int32_t nprob, int32_t m, int32_t n, int32_t nact, int32_t have_stages,
                     nlh_qrx_plan_head *head, nlh_qrx_plan_step *steps, int32_t cap);
/* The exact factorisation keeps its working matrix (8 bytes per element of the padded Jacobians) and, for batches large
 * enough to take the lane-per-column passes, a SECOND copy that their flush writes instead of rewriting the first in place
 * (memory of the exact policy, NLH_QRX_OOP).  Bytes the handle and its sub-batch workers hold for second
 * copies right now: 0 until a factorisation asked for one, and when the device had no room for it. */
int64_t nlh_qrx_second_matrix_bytes(nlh_handle *h);
/* lmpar (:394-566, including its two deviations from MINPACK) on an n-by-n R
 * (leading dimension ldr) for every problem.  dtailsq[k] = sum of squares of the
 * caller's wa4(n+1:m).  Outputs: dpar (in/out), dxstep [nprob][n], dsdiag [nprob][n]. */
int nlh_lmpar(nlh_handle *h, int32_t nprob, int32_t n, double *dR, int32_t ldr,
              const int32_t *dipvt, const double *ddiag, const double *dqtf,
              const double *ddelta, const double *dtailsq, double *dpar,
              double *dxstep, double *dsdiag);
/* lu_factor / solve_lu stand-ins (call sites src/nonlin_solve.f90:570,577):
 * partial-pivoting LU of [nprob][n][n] in place, 0-based ipvt, then one RHS each. */
int nlh_lu_factor(nlh_handle *h, int32_t nprob, int32_t n, double *dA, int32_t *dipvt,
                  int32_t *dinfo);
int nlh_lu_solve(nlh_handle *h, int32_t nprob, int32_t n, const double *dLU,
                 const int32_t *dipvt, double *db);
/* qr_factor(b, q = q, r = r), qr_rank1_update(q, r, u, v) and solve_triangular_system stand-ins
 * (call sites src/nonlin_solve.f90:289, 307, 327; third-party linalg in the reference).
 * dB, dQ: [nprob][n][n] column-major.  dRt: R stored ROW-major.  Q1 R1 = Q R + u v^T. */
int nlh_qr_factor_full(nlh_handle *h, int32_t nprob, int32_t n, const double *dB, double *dQ,
                       double *dRt);
int nlh_qr_rank1_update(nlh_handle *h, int32_t nprob, int32_t n, double *dQ, double *dRt,
                        const double *du, const double *dv);
int nlh_solve_upper(nlh_handle *h, int32_t nprob, int32_t n, const double *dRt, double *dx);
/* Sizes: nlh_qr_factor_full and nlh_qr_rank1_update return NLH_ARRAY_SIZE_ERROR beyond n = 8192 (the largest system the
 * quasi-Newton solver takes), nlh_solve_upper where x (8 n bytes) and the kernel's own 4 KiB no longer fit the 158 KiB of
 * LDS a workgroup may have (n = 19711 is the last that fits; 8192 works) -- each before anything is launched or written. */
/* The Householder steps behind all of the above -- nlh_qr_factor_full, every constrained least-squares iteration, every
 * polynomial fit -- as a stage of their own, for nprob work arrays [A | E]: dA [nprob][rows][ncA] and dE [nprob][rows][ncE],
 * both ROW-major, transformed in place on the handle's stream.  On return A holds R in its upper triangle (exact zeros
 * below the diagonal) and E = Q^T E: E = I (ncE = rows) gives Q^T, E = a right-hand side f gives Q^T f.  min(ncA, rows - 1)
 * steps; a step whose squares below the diagonal sum to exactly zero is skipped (H = I) -- zeros, or entries below
 * 1.5e-162, whose squares underflow -- and leaves (its diagonal entry, zeros).  Every sum runs in ascending row order, so
 * A and E are bit-identical to the CPU restatement (nlo_qr_factor_cols) in every kernel form.  ncE = 0 is allowed (dE may
 * then be NULL).  NLH_INVALID_INPUT_ERROR for nprob < 1, rows < 1, ncA < 1, ncE < 0, ncA > rows or a NULL array;
 * NLH_ARRAY_SIZE_ERROR beyond 65535 problems, 1,048,560 rows or 2^20 columns (the kernels' grids); either way nothing is
 * touched.  Scratch: nprob (2 rows + 2 (ncA + ncE) + 8) doubles of the handle's workspace. */
int nlh_house_steps(nlh_handle *h, int32_t nprob, int32_t rows, int32_t ncA, int32_t ncE, double *dA, double *dE);
/* Which kernel form those steps take for a shape: host code only -- no handle, no device -- the very function the launch
 * dispatches through.  The shape and the batch size decide, never the data; forms never change a bit of the result.
 * Returns the form; *tiles (may be NULL) = product tiles the form keeps in LDS (what distinguishes the two variants of
 * NLH_HOUSE_FORM_FUSED16).  -NLH_INVALID_INPUT_ERROR / -NLH_ARRAY_SIZE_ERROR as nlh_house_steps.  nc = ncA + ncE: */
enum { NLH_HOUSE_FORM_FUSED4 = 0,      /* k_qn_house_fused<4>: rows <= 4096 and nc nprob < 1536; 4 columns a workgroup, 2 tiles */
       NLH_HOUSE_FORM_FUSED16 = 1,     /* k_qn_house_fused<16>: rows <= 4096 otherwise; 16 columns a workgroup; 2 tiles while
                                          ceil(nc / 16) nprob <= 256, 1 beyond (two workgroups share a compute unit) */
       NLH_HOUSE_FORM_DOT2 = 2,        /* k_qn_house_dot2: 4096 < rows <= 8192; 16 columns a workgroup, 2 tiles */
       NLH_HOUSE_FORM_DOT_LDS = 3,     /* k_qn_house_dot<false>: 8192 < rows <= 18000; a thread per column, reflector in LDS, 0 tiles */
       NLH_HOUSE_FORM_DOT_GLOBAL = 4 };/* k_qn_house_dot<true>: rows > 18000; the reflector stays in global memory */
int32_t nlh_house_plan(int32_t nprob, int32_t rows, int32_t ncA, int32_t ncE, int32_t *tiles);
/* cholesky_rank1_update (downdate = 0) / cholesky_rank1_downdate (1) stand-ins (call sites
 * src/nonlin_optimize.f90:721-722): R1^T R1 = R^T R +- u u^T in place on the ROW-major upper factor dRt;
 * du is consumed; *hinfo = 1 if the downdate would lose positive definiteness. */
int nlh_chol_rank1(nlh_handle *h, int32_t n, int32_t downdate, double *dRt, double *du, int32_t *hinfo);
/* cholesky_factor(b, .true.) and solve_cholesky(.true., r, x) stand-ins (call sites src/nonlin_optimize.f90:724, 727),
 * through the launches of bfgs%solve.  dB [nprob][n][n] symmetric; dRt [nprob][n][n] the ROW-major upper factors, zeros
 * below the diagonal; hinfo [nprob] (host): 0, or the 1-based row of a non-positive pivot (the rows above it are
 * factored, the others hold B).  dx [nprob][n] in place.  nlh_bf_chol_form(n): the form the factorisation takes --
 * G = 4, 2, 1: the blocked kernel with G thread groups per column (while its LDS fits: n <= 608); -4, -8: the column
 * form with that many columns per thread; 0 for an n no form exists for.  It asks the runtime for the kernel's static
 * LDS: call it on a thread whose device is set (any handle created), or it reports the column form. */
int nlh_bf_chol_factor(nlh_handle *h, int32_t nprob, int32_t n, const double *dB, double *dRt, int32_t *hinfo);
int nlh_bf_solve_cholesky(nlh_handle *h, int32_t nprob, int32_t n, const double *dRt, double *dx);
int32_t nlh_bf_chol_form(int32_t n);

/* polynomial%fit / polynomial%fit_thru_zero (src/nonlin_polynomials.f90:146-238): least-squares polynomial of
 * the given order through npts points; coef = c0 .. c_order (c0 = 0 for thru_zero).  Returns 4 where the
 * reference stops with 4 (order >= npts or order < 1).  solve_least_squares (third-party linalg) is the
 * Householder QR + back substitution of nlh_cls_solve.  The batch form takes device arrays
 * dx, dy [nprob][npts], dcoef [nprob][order + 1]. */
int nlh_poly_fit(nlh_handle *h, int32_t npts, int32_t order, int32_t thru_zero, const double *x,
                 const double *y, double *coef);
int nlh_poly_fit_batch(nlh_handle *h, int32_t nprob, int32_t npts, int32_t order, int32_t thru_zero,
                       const double *dx, const double *dy, double *dcoef);

/* polynomial%roots (:357-381) for real polynomials of one order: the eigenvalues of the companion matrix of :346-353 by
 * DGEBAL-style balancing and DLAHQR's double-shift QR (see DESIGN "Polynomial roots"); coef = c0 .. c_order.  Roots are
 * interleaved (re, im), z [order][2] = complex(real64) / complex128, in the order DGEEV's WR / WI have: a complex pair as
 * (re, +im), (re, -im), the exact zero roots of zero low coefficients last.  info (per polynomial): 0;
 * NLH_CONVERGENCE_ERROR (the sweep limit: the roots that deflated are valid, the others NaN); NLH_DIVIDE_BY_ZERO_ERROR
 * (leading coefficient exactly 0; roots NaN); NLH_INVALID_INPUT_ERROR (a coefficient, or a quotient -c_i / c_order, that
 * is not finite; roots NaN).  The return value is non-zero only for bad arguments (order < 0: NLH_INVALID_INPUT_ERROR;
 * order > 256: NLH_ARRAY_SIZE_ERROR, nothing launched) or a HIP error.  order == 0 returns 0 and writes nothing (:373).
 * The batch form takes device arrays dcoef [nprob][order + 1], dz [nprob][order][2], dinfo [nprob].
 * NLH_POLYROOTS_FORM = lane | wave | global (environment, read at each call) moves a call to a later form than the one
 * its order selects (lane per polynomial: order <= 8; wave per polynomial on an LDS window: <= 128; on a global-memory
 * window: <= 256); every form gives the same bits. */
int nlh_poly_roots(nlh_handle *h, int32_t order, const double *coef, double *z, int32_t *info);
int nlh_poly_roots_batch(nlh_handle *h, int32_t nprob, int32_t order, const double *dcoef, double *dz,
                         int32_t *dinfo);
/* polynomial%evaluate (:241-321), Horner from the top, for device arrays: dcoef [nprob][order + 1]; real points dx, dy
 * [nprob][npts]; complex points dz, dy [nprob][npts][2] (the product y x is the four-multiply form, the real
 * coefficient is added to the real part only). */
int nlh_poly_eval_batch(nlh_handle *h, int32_t nprob, int32_t order, int32_t npts, const double *dcoef,
                        const double *dx, double *dy);
int nlh_poly_eval_complex_batch(nlh_handle *h, int32_t nprob, int32_t order, int32_t npts, const double *dcoef,
                                const double *dz, double *dy);

/* ---- parameter covariance of a least-squares fit (no counterpart in nonlin v2.2.0; MINPACK, whose lmder lss_solve
 * modernises, ships it as `covar`).  For the problem min ||F(x)||^2 with Jacobian J at x:  cov = s^2 (J^T J)^-1, the
 * standard errors sigma_i = sqrt(cov(i,i)) and the reduced chi-square s^2 = ||F(x)||^2 / (m - n). ----
 * nlh_covar: MINPACK's covar, statement order kept, on the pivoted factor nlh_lmfactor_exact writes -- dR [nprob][n][n]
 * column-major (upper triangle, diagonal = rdiag; the lower triangle is not read; dR is not modified), dipvt [nprob][n]
 * 0-based.  tolr = tol |r(0,0)|; rank = number of leading k with |r(k,k)| > tolr (the first failure ends the count);
 * the leading rank x rank block is inverted, (R^T R)^-1 formed and scattered to cov(ipvt(i), ipvt(j)), symmetric (exactly);
 * rows and columns of the n - rank variables pivoted last are exactly 0 (they are not determined by the data to within
 * tol).  tol <= 0 means machine epsilon.  dcov [nprob][n][n], drank [nprob].  Any n >= 1 and any nprob.  Three forms give
 * the same bits (the plain sequential loops, -ffp-contract=off): a lane per problem (n <= 8), a workgroup per problem
 * with the packed inverse in LDS (while nlh_covar_lds_bytes(n) fits the 161,792-byte cap: n <= 200), the same on a
 * global-memory window of the handle (any n).  NLH_COVAR_FORM = lane | lds | global (environment, read at each call)
 * forces a form for the sizes it can hold.  Switch points and rates: profiles/covar_rate.txt. */
int nlh_covar(nlh_handle *h, int32_t nprob, int32_t n, const double *dR, const int32_t *dipvt, double tol,
              double *dcov, int32_t *drank);
/* Dynamic LDS bytes the workgroup form of nlh_covar asks for at n columns (host code, no device): the count the library
 * compares with the cap before launching. */
int64_t nlh_covar_lds_bytes(int32_t n);
/* The covariance of nprob problems of the user's device family AT THE GIVEN x (dx [nprob][n], device, not modified):
 * fvec = F(x) (one launcher call), J by vfh_jac_fcn's rule exactly as nlh_fd_jacobian_device (jacfcn, or forward
 * differences), nlh_lmfactor_exact, nlh_covar with tol.  chi2 = (sum of f_i^2, i ascending, sequential) / (m - n);
 * scaled = 1 multiplies every entry of cov once by chi2; sigma_i = sqrt(cov(i,i)) (after the scaling).  dcov [nprob][n][n];
 * dsigma [nprob][n], drank [nprob], dchi2 [nprob] may be NULL.  scaled = 1 with m <= n: NLH_INVALID_INPUT_ERROR; m < n:
 * NLH_UNDERDEFINED_PROBLEM_ERROR -- both before anything is evaluated (m == n with scaled = 0 is accepted; chi2 is then
 * the IEEE quotient by zero).  A problem's bits do not depend on the batch it sits in; batches beyond 65535 problems
 * run in slices.  Uses workspaces of the handle that no solver uses. */
int nlh_lm_covariance_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                   nlh_device_jacfcn jacfcn, void *ctx, const double *dx, int32_t scaled, double tol,
                                   double *dcov, double *dsigma, int32_t *drank, double *dchi2);
/* ... behind HOST arrays x, cov, sigma, rank, chi2. */
int nlh_lm_covariance_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                     nlh_device_jacfcn jacfcn, void *ctx, const double *x, int32_t scaled, double tol,
                                     double *cov, double *sigma, int32_t *rank, double *chi2);
/* ... for ONE problem with HOST callbacks: fcn at x, then vfh_jac_fcn's calls (jacfcn, or the n perturbed evaluations in
 * ascending j; x is perturbed in place and restored), on the calling thread; the linear algebra runs on the device.
 * cov [n][n], sigma [n] / rank / chi2 (NULL allowed): host. */
int nlh_lm_covariance(nlh_handle *h, int32_t m, int32_t n, nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx, double *x,
                      int32_t scaled, double tol, double *cov, double *sigma, int32_t *rank, double *chi2);
/* ... for every problem of a model object (built-in family: forward differences, as its LM solve; a user-launcher model:
 * its jacfcn if it has one), host arrays; a model on a device set is served share by share (handle may be NULL).  What
 * the Fortran shim's least_squares_solver%covariance / covariance_batch call. */
int nlh_dq_model_lm_covariance(nlh_handle *h, const nlh_dq_model *model, const double *x, int32_t scaled, double tol,
                               double *cov, double *sigma, int32_t *rank, double *chi2);

/* ---- built-in curve models (no counterpart in nonlin v2.2.0, which ships no model): sums of peaks or decays on a
 * polynomial baseline, as library-owned launchers of the open device-residual path above, so that a curve fitter needs no
 * device code of their own.  A model is a kind, ncomp = K >= 1 components and nbase = B in {-1, 0, .., 8}: the degree of a
 * polynomial baseline, -1 for none.  It is fitted to data t, y [nprob][m] with optional weights w [nprob][m]; with
 * shared_t != 0, t is one [m] array for every problem.  Parameters: the K components in order, then c_0 .. c_B, so
 * n = P K + B + 1 with P = 3 for the peaks and 2 for the decay (n <= 8192).
 * THE OPERATION ORDER IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation, the device library's
 * exp -- so that a restatement in any IEEE language reproduces the exp-free kind bit for bit:
 *   kind                        component k at abscissa t                              its partials, in parameter order
 *   NLH_CURVE_GAUSS (a,mu,s)    d = (t - mu)/s; e = exp(-0.5*(d*d)); term = a*e        e;  g = ((a*e)*d)/s;  g*d
 *   NLH_CURVE_LORENTZ (a,mu,w)  d = (t - mu)/w; q = 1.0 + d*d; term = a/q              1.0/q;  g = ((2.0*a)*d)/((w*q)*q);  g*d
 *   NLH_CURVE_EXPDECAY (a,k)    e = exp(-(k*t)); term = a*e                            e;  -((a*t)*e)
 *   model sum   s = 0;  s = s + term_k for k ascending
 *   baseline    b = c_B;  b = b*t + c_j for j = B-1 .. 0;  s = s + b;      partials: p = 1; column = p; p = p*t, j ascending
 *   residual    r = s - y;  then r = w*r when weights are given; every Jacobian entry is multiplied once by w then
 * No sum crosses a row: a row's bits do not depend on the launch it is computed in.  Two workgroup forms give the same
 * bits: a workgroup per (point, 256 rows), and -- while two points or more fit 256 threads, m <= 128 -- several points per
 * workgroup; NLH_CURVE_FORM = row | flat (environment, read at each call) forces one for the sizes it can hold (flat:
 * m <= 256).
 * Weights and ragged data: rows with w = 0 are the way to pad spectra of different lengths to a common m (such a row's
 * residual and Jacobian row are exactly 0).  When weights are given the degrees of freedom of a problem are
 * dof = (number of rows with w != 0) - n, and nlh_curve_fit_batch reports chi2 = (sum of f_i^2, i ascending, sequential)
 * / dof and multiplies every entry of cov once by (m - n) / dof before sigma_i = sqrt(cov(i,i)) is taken (with no zero
 * weight both are what nlh_lm_covariance_batch_device returns, bit for bit).  A problem with dof <= 0 gets
 * NLH_INVALID_INPUT_ERROR in status[p] before anything is evaluated for it; the others are solved. ---- */
#define NLH_CURVE_GAUSS     0
#define NLH_CURVE_LORENTZ   1
#define NLH_CURVE_EXPDECAY  2
#define NLH_CURVE_MAX_BASE  8
#define NLH_CURVE_MAX_N  8192
typedef struct nlh_curve_ctx {
    int32_t kind, ncomp, nbase;
    int32_t shared_t;     /* dt is [m], the same abscissae for every problem */
    int32_t m;
    const double *dt;     /* [nprob][m] (shared_t: [m]), device; the caller's */
    const double *dy;     /* [nprob][m], device */
    const double *dw;     /* [nprob][m], device, or NULL: no weights */
} nlh_curve_ctx;
/* The launchers (nlh_device_vecfcn / nlh_device_jacfcn, ctx = nlh_curve_ctx): they enqueue on the stream handed in, never
 * synchronise and may be called from several host threads.  A malformed ctx -- unknown kind, K < 1, B outside -1 .. 8,
 * n != P K + B + 1, m != ctx->m, a NULL array -- returns NLH_INVALID_INPUT_ERROR before any launch. */
int nlh_curve_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                         int32_t m, double *dF);
int nlh_curve_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                         int32_t m, double *dJ);
/* n of a model (host code only); -1 for an unknown kind, ncomp < 1, nbase outside -1 .. 8 or n > 8192. */
int32_t nlh_curve_nparams(int32_t kind, int32_t ncomp, int32_t nbase);
/* A curve model as a MODEL object of the device-function kind, from HOST arrays t [nprob][m] (shared_t: [m]), y, w (NULL:
 * no weights): the model owns its context and device copies, nlh_dq_model_destroy frees them.  analytic selects the
 * Jacobian launcher; 0: forward differences, the reference's default.  nlh_dq_model_eval / _lm_solve / _cls_solve /
 * _lm_covariance accept it as they accept any device-function model.  Errors (every nlh_curve_* entry point, in this
 * order): NLH_ERR_BAD_HANDLE (NULL handle), NLH_INVALID_INPUT_ERROR (bad kind or counts, a NULL array),
 * NLH_UNDERDEFINED_PROBLEM_ERROR (m < n). */
int nlh_curve_model_create(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                           const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                           nlh_dq_model **model);
/* Model values -- no data term, no weights, the arithmetic above -- at arbitrary abscissae dt [nprob][npts] (shared_t:
 * [npts]) for parameters dx [nprob][n]: dy [nprob][npts].  DEVICE pointers. */
int nlh_curve_eval_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t npts,
                         const double *dt, int32_t shared_t, const double *dx, double *dy);
/* Fit + errors in one call, exactly this composition: nlh_lm_solve_batch_device (or, when xl or xu is given -- [n] host
 * arrays, one box for every problem --, nlh_cls_solve_batch_device with delta0 = stepscale0 = 1) with the curve launchers;
 * then, if any of dsigma, dcov, dchi2 is non-NULL, nlh_lm_covariance_batch_device at the solution with scaled = 1 and the
 * default tol, and the degrees-of-freedom rule above when dw is given.  A problem whose status is not 0 gets NaN in
 * sigma, cov and chi2 and rank -1.  dt, dy, dw (NULL: none), dx [nprob][n] in/out, dfvec [nprob][m], dsigma [nprob][n],
 * dcov [nprob][n][n], dchi2 [nprob], drank [nprob]: DEVICE; ib, status: host [nprob], NULL allowed.  Asking for errors
 * with m <= n: NLH_INVALID_INPUT_ERROR before anything is evaluated. */
int nlh_curve_fit_batch(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                        int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                        const double *xl, const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov,
                        double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
/* ... behind HOST arrays t, y, w, x, fvec, sigma, cov, chi2, rank. */
int nlh_curve_fit_batch_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                          int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                          const double *xl, const double *xu, double *x, double *fvec, double *sigma, double *cov,
                          double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);

/* ---- formula models (no counterpart in nonlin v2.2.0): the model is an expression the user writes as a string, e.g.
 * "a*exp(-((t-mu)/s)^2/2)+c" with vars "t" and params "a,mu,s,c".  nlh_expr_compile (pure host code, needs no GPU) turns it
 * into a small postfix program; the kernels behind nlh_expr_device_fcn / _jac interpret it, a thread per (point, row), so a
 * curve fitter needs neither hipcc nor device code.
 * GRAMMAR (blanks and newlines are ignored; operators are left-associative; -a^2 is -(a^2); a^2^3 is an error):
 *   formula := (name '=' expr ';')* expr
 *   expr  := term (('+'|'-') term)*            term  := unary (('*'|'/') unary)*
 *   unary := ('-'|'+') unary | power           power := atom ('^' ['-'] number)?
 *   atom  := number | name | func '(' expr (',' expr)* ')' | '(' expr ')'
 * number: what strtod reads in the C locale from a digit or '.'; name: a variable, a parameter or pi (the only named
 * constant); func: exp log sqrt sin cos tanh atan abs erf erfc erfcx voigt pow atan2 min max where j0 j1 i0e i1e lgamma expm1
 * log1p.  voigt takes exactly
 * three arguments (x, sigma, gamma), where three (c, a, b: a where c >= 0, else b), pow(a, b), atan2(y, x), min(a, b) and
 * max(a, b) two, every other function one; another count is an error that names its column.  '^' takes a literal only: an
 * exponent that is a parameter or an expression is pow's second argument.  vars: 1 .. 4 comma-separated names; params: 1 .. 32, their order is
 * the order of x.  A name is [A-Za-z_][A-Za-z0-9_]*, not pi and not a function.
 * DEFINITIONS: name = expr; in front of the formula names a value that is computed once, e.g. with vars "x,y" and params
 * "a,x0,y0,sx,sy,th,b" the rotated elliptical Gaussian
 *   dx = x-x0; dy = y-y0; c = cos(th); s = sin(th);  u = dx*c + dy*s;  v = dy*c - dx*s;
 *   b + a*exp(-(u^2/(2*sx^2) + v^2/(2*sy^2)))
 * A definition's name follows the name rule and is not a variable, a parameter, a function, pi or an earlier definition
 * (single assignment); it may be used in every later statement, any number of times, also never.  The last statement is
 * the model value and has no name; a trailing ';' or an empty statement is an error.  A formula without ';' compiles to
 * the program it always did.
 * THE PROGRAM IS THE POSTFIX OF THE PARSE TREE: no constant folding, no reassociation, no sharing the user did not write
 * (a unary '+' emits nothing; every literal and every pi is a constant of its own; a definition is written once however
 * often it is used, and counts once toward the 256 instructions and 64 constants).  THE FRAME: statement k is compiled with
 * k slots of the stack in use, so its root lands in slot k and stays there -- no instruction stores --, the next statement
 * evaluates on top of it, and the model value ends in slot ndef, the number of definitions.  depth (nlh_expr_shape) is
 * that frame: the most slots in use, definitions included, 16 at most.  Instructions (op, arg):
 *   CONST i (consts[i])   VAR v   PARAM k   NEG   ADD   SUB   MUL   DIV   (b on top of the stack, a below it)
 *   IPOW k   an integer literal exponent, 2 <= |k| <= 16          POWC i   any other literal exponent c = consts[i]
 *   EXP LOG SQRT SIN COS TANH ATAN ABS   ERF ERFC ERFCX   VOIGT (pops x, sigma, gamma -- gamma on top -- and pushes one)
 *   POW ATAN2 MIN MAX (b on top, a below it)   WHERE (pops c, a, b -- b on top -- and pushes one)
 *   LOAD k   pushes a copy of slot k, the value of definition k
 *   J0 J1 (the Bessel functions of the first kind)   I0E I1E (exp(-|a|) I0(a), exp(-|a|) I1(a): the scaled modified Bessel
 *   functions; I0 itself overflows at 713)   LGAMMA (log |Gamma(a)|)   EXPM1 (exp(a) - 1)   LOG1P (log(1 + a)): one operand each
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation, the device library's
 * functions -- so that a restatement in any IEEE language reproduces bit for bit an exp-free formula: one without a
 * library function (POWC EXP LOG SIN COS TANH ATAN ERF ERFC ERFCX POW ATAN2 J0 J1 LGAMMA EXPM1 LOG1P; a formula that uses
 * them is within the running bound of the restatement, not bit for bit).  VOIGT is not one: a formula whose only
 * function is voigt stays in the bit-exact class (the Faddeeva function below is stated arithmetic, not a library call).
 * MIN, MAX and WHERE are selections and stay in it too.  I0E and I1E are stated arithmetic as well (+ - * / and sqrt): a
 * formula whose only functions are i0e and i1e stays in the bit-exact class.
 *   values     the obvious operation per instruction;  POWC: pow(a, c);  NEG, ABS: sign operations;
 *              IPOW k: v = a; v = v*a (|k| - 1 times in all); for k < 0 then v = 1.0/v
 *   column j of the Jacobian: forward mode with STRUCTURAL zeros.  A node's tangent is absent (Z) or a double: CONST, VAR,
 *   PARAM k != j are Z, PARAM j is 1.0; a Z operand is dropped, never multiplied (da, db: the tangents of a, b; v: the value)
 *     ADD   da + db | da | db                       SUB   da - db | da | -db
 *     MUL   da*b + a*db | da*b | a*db               DIV   q = a/b:  (da - q*db)/b | da/b | -((q*db)/b)
 *     NEG   -da
 *     IPOW  u = the product before the last multiplication (a itself for |k| = 2):
 *           k > 0: ((double)k*u)*da                 k < 0: -((((double)|k|*u)*da)*(v*v))
 *     POWC  (c*pow(a, c - 1.0))*da
 *     EXP   v*da          LOG  da/a                 SQRT  da/(2.0*v)          SIN  cos(a)*da       COS  -(sin(a)*da)
 *     TANH  (1.0 - v*v)*da                          ATAN  da/(1.0 + a*a)      ABS  a < 0 ? -da : da
 *     with C1 = 2/sqrt(pi) = 1.1283791670955126, SQRT2 = 1.4142135623730951, SQRTPI = 1.772453850905516:
 *     ERF   v = erf(a):    (C1*exp(-(a*a)))*da      ERFC  v = erfc(a):  -((C1*exp(-(a*a)))*da)
 *     ERFCX v = erfcx(a):  ((2.0*a)*v - C1)*da      (the device library's erf, erfc, erfcx, exp)
 *     VOIGT voigt(x, sigma, gamma) = Re w(z)/(|sigma| sqrt(2 pi)), z = (x + i|gamma|)/(|sigma| sqrt(2)): the Gaussian of
 *           standard deviation sigma convolved with the Lorentzian of half width gamma, unit area; defined for sigma != 0
 *           s = |sigma|; g = |gamma|; u = s*SQRT2; zr = x/u; zi = g/u; (wr, wi) = w(zr, zi) (nlh_faddeeva below)
 *           nrm = u*SQRTPI; v = wr/nrm
 *           w' = -2zw + i C1:  dwr = -(2.0*(zr*wr - zi*wi));  dwi = C1 - 2.0*(zr*wi + zi*wr);  un = u*nrm
 *           gx = dwr/un;  gs = -((v + (zr*dwr - zi*dwi)/nrm)/s);  gg = -(dwi/un);
 *           sigma < 0: gs = -gs;  gamma < 0: gg = -gg  (the ABS rule)
 *           tangent, with dx, ds, dg the operands' tangents, the present ones in this order:
 *             gx*dx + gs*ds + gg*dg | gx*dx + gs*ds | gx*dx + gg*dg | gs*ds + gg*dg | gx*dx | gs*ds | gg*dg
 *           (sums left to right).  w is evaluated once per pass over the program and serves the value and every column
 *           the pass carries.  gs is computed through a cancellation in the Lorentzian wings (|x| >> sigma): its error
 *           is small against V(0)/sigma, not against itself.
 *     MAX   s = b > a;  v = s ? b : a               MIN   s = b < a;  v = s ? b : a
 *           a tie keeps a (max(-0.0, 0.0) is -0.0); a NaN b is dropped, a NaN a stays.  Tangent: the selected operand's,
 *           s ? db : da, and +0.0 where the selected operand is Z and the other is not
 *     WHERE s = c >= 0.0;  v = s ? a : b            (-0.0 selects a, NaN selects b)
 *           tangent: the selected branch's, s ? da : db, +0.0 where that one is Z; dc is never read.  Both branches are
 *           evaluated; the selection is a select, never a multiplication, so a NaN or Inf in the branch not taken
 *           reaches neither the value nor the tangent.  A node whose only tangent is c's is present and +0.0.
 *     ATAN2 v = atan2(a, b);  den = a*a + b*b:      (b*da - a*db)/den | (b*da)/den | -((a*db)/den)
 *     POW   v = pow(a, b)
 *           ga = b*pow(a, b - 1.0), computed only where a has a tangent
 *           gb = v == 0.0 ? 0.0 : v*log(a), computed only where b has a tangent
 *           ta = da == 0.0 ? 0.0 : ga*da;  tb = gb*db;        ta + tb | ta | tb
 *           The two guards make a = 0 usable: gb is its limit 0 for b > 0 instead of 0*-inf, and an infinite ga
 *           (b < 1) against a zero da is 0.  a < 0 with a tangent in b is outside the domain (log(a): NaN).
 *           (the device library's pow, atan2, log)
 *     LOAD k  v = the value in slot k;  tangent: the one in slot k, Z where definition k's is (a copy: no operation)
 *     the unary functions below: g is computed only where the operand has a tangent
 *     EXPM1  v = expm1(a)          g = exp(a)                         g*da     (not v + 1.0: it cancels for a << 0)
 *     LOG1P  v = log1p(a)          da/(1.0 + a)
 *     J0     v = j0(a)             g = j1(a)                          -(g*da)
 *     J1     v = j1(a)             g = a == 0.0 ? 0.5 : j0(a) - v/a   g*da
 *     I0E    v = i0e(a)            s = a < 0.0 ? -v : v;  g = i1e(a) - s                                   g*da
 *     I1E    v = i1e(a)            s = a < 0.0 ? -v : v;  g = a == 0.0 ? 0.5 : (i0e(a) - s) - v/a          g*da
 *     LGAMMA v = lgamma(a)         g = digamma(a)                     g*da
 *            (the device library's expm1, log1p, j0, j1, lgamma, exp; i0e, i1e and digamma are stated here)
 *       cheb(y, c[0 .. N-1]), Clenshaw's recurrence, the coefficients highest degree first:
 *            b0 = c[0]; b1 = 0.0; b2 = 0.0;  for k = 1 .. N-1:  b2 = b1;  b1 = b0;  b0 = (y*b1 - b2) + c[k];   0.5*(b0 - b2)
 *       i0e(a):  x = |a|;  x <= 8.0:  cheb(x/2.0 - 2.0, I0E_A[30])         else  cheb(32.0/x - 2.0, I0E_B[25])/sqrt(x)
 *       i1e(a):  x = |a|;  x <= 1.0:  cheb(x*4.0 - 2.0, I1E_A[15])*x       else  x <= 8.0:  cheb((x - 4.5)/1.75, I1E_M[28])
 *                                                                           else  cheb(32.0/x - 2.0, I1E_B[25])/sqrt(x)
 *                then a < 0.0 ? -v : v   (odd; i1e(-0.0) is +0.0).  A NaN a takes the last range and stays NaN.
 *            The five tables are the Chebyshev coefficients, in T_k(y/2) on -2 <= y <= 2, of exp(-x) I0(x) (x = 2(y + 2)),
 *            of exp(-x) I1(x)/x (x = (y + 2)/4) and exp(-x) I1(x) (x = 4.5 + 1.75 y), and of sqrt(x) exp(-x) I0(x) and
 *            sqrt(x) exp(-x) I1(x) (x = 32/(y + 2)): literal constants of the library
 *            (nonlin_amd/csrc/nlh_kernels_specfun2.h), derived at 40 digits by tests/golden/make_specfun2_tables.py.
 *            (i1e has a middle range because the series of exp(-x) I1(x)/x, taken up to 8, cancels to a thirtieth of its
 *            terms there.)  Measured against 40-digit values, a uniform sample of [-8, 8] among them: i0e within
 *            3.5 * 2^-52 of the true value, relatively, i1e within 1.7 * 2^-52.
 *       digamma(a), a > 0 (NaN for a <= 0 and for a NaN a: outside the domain, as POW's log(a)), B[k] = B_2k+2/(2k + 2),
 *            k = 0 .. 6: 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12:
 *            r = 0.0;  while a < 10.0:  r = r + 1.0/a;  a = a + 1.0          (ten steps at most)
 *            z = 1.0/(a*a);  p = B[6];  for k = 5 .. 0:  p = p*z + B[k];   p = p*z
 *            ((log(a) - 0.5/a) - p) - r                                      (the device library's log)
 *     a root that is Z writes +0.0
 *   A program with definitions gives, bit for bit, the value and every Jacobian column of the formula with each definition
 *   substituted in parentheses: the operations on the operands are the same, and each IEEE operation and each library
 *   function is deterministic.  Whether a formula is in the bit-exact class is decided by the functions it uses, as before.
 *   "structural": the compiler records per instruction the 32-bit mask of the parameters its subtree names -- WHERE's
 *   condition included --; the tangent of a node for column j is present exactly when bit j of that mask is set, whatever
 *   the values are.
 *   residual   r = f - y;  then r = w*r when weights are given; every Jacobian entry is multiplied once by w then (the
 *              padding rule of the curve models: a row of weight 0 is a zero -- of either sign, 0 times the value's --
 *              where the value is finite; the product is a multiplication, not a store, so 0 times a non-finite value
 *              is NaN)
 * No sum crosses a row: a row's bits do not depend on the launch shape, the workgroup form (NLH_EXPR_FORM = row | flat,
 * environment, read at each call, as NLH_CURVE_FORM), the number of Jacobian columns a pass carries, or the batch. ---- */
#define NLH_EXPR_MAX_INSTR   256
#define NLH_EXPR_MAX_CONST    64
#define NLH_EXPR_MAX_DEPTH    16
#define NLH_EXPR_MAX_VARS      4
#define NLH_EXPR_MAX_PARAMS   32
#define NLH_EXPR_CONST  0
#define NLH_EXPR_VAR    1
#define NLH_EXPR_PARAM  2
#define NLH_EXPR_NEG    3
#define NLH_EXPR_ADD    4
#define NLH_EXPR_SUB    5
#define NLH_EXPR_MUL    6
#define NLH_EXPR_DIV    7
#define NLH_EXPR_IPOW   8
#define NLH_EXPR_POWC   9
#define NLH_EXPR_EXP   10
#define NLH_EXPR_LOG   11
#define NLH_EXPR_SQRT  12
#define NLH_EXPR_SIN   13
#define NLH_EXPR_COS   14
#define NLH_EXPR_TANH  15
#define NLH_EXPR_ATAN  16
#define NLH_EXPR_ABS   17
#define NLH_EXPR_ERF   18
#define NLH_EXPR_ERFC  19
#define NLH_EXPR_ERFCX 20
#define NLH_EXPR_VOIGT 21
#define NLH_EXPR_POW   22
#define NLH_EXPR_ATAN2 23
#define NLH_EXPR_MIN   24
#define NLH_EXPR_MAX   25
#define NLH_EXPR_WHERE 26
#define NLH_EXPR_LOAD  27
#define NLH_EXPR_J0    28
#define NLH_EXPR_J1    29
#define NLH_EXPR_I0E   30
#define NLH_EXPR_I1E   31
#define NLH_EXPR_LGAMMA 32
#define NLH_EXPR_EXPM1 33
#define NLH_EXPR_LOG1P 34
typedef struct nlh_expr nlh_expr;
/* Compile (host code only, thread-safe).  Errors -- a syntax error, an unknown name, a name in both lists, a duplicate or
 * reserved name ("'erf' is a function", "'lgamma' is a function"), a definition whose name is taken ("'t' is a variable", "'u' is already defined"), a wrong number of arguments, an empty list or item, too many names, more than 256 instructions, 64 constants or a stack deeper than 16
 * -- return NLH_INVALID_INPUT_ERROR, leave *e NULL and set the message nlh_expr_error() returns (thread-local), e.g.
 * "col 17: unknown name 'foo'" (0-based column of the formula; "vars col 2: ..." / "params col 2: ..." for the lists). */
int nlh_expr_compile(const char *formula, const char *vars, const char *params, nlh_expr **e);
const char *nlh_expr_error(void);
void nlh_expr_destroy(nlh_expr *e);
/* Any of the outputs may be NULL.  depth: the deepest the evaluation stack gets, the definitions' slots included. */
void nlh_expr_shape(const nlh_expr *e, int32_t *nvar, int32_t *nparams, int32_t *ninstr, int32_t *nconst, int32_t *depth);
/* Read-back, for restatements: op, arg [ninstr], consts [nconst] (any may be NULL).  The dependency masks: nlh_expr_masks. */
int nlh_expr_program(const nlh_expr *e, int32_t *op, int32_t *arg, double *consts);
int nlh_expr_masks(const nlh_expr *e, uint32_t *mask);
/* Operand roots [ninstr] (either may be NULL): aroot, the instruction that produced the lower operand of a binary
 * instruction (POW, ATAN2, MIN, MAX included), VOIGT's x or WHERE's c; broot, the one that produced VOIGT's sigma or
 * WHERE's a (0 elsewhere).  The top operand's is i - 1.  LOAD k is a leaf for both rules; its own aroot is the instruction
 * that produced definition k, and its mask that instruction's.  The code word is op | (arg & 0xff) << 8 | aroot << 16 |
 * broot << 24, so all of VOIGT's and WHERE's dependency masks are structural. */
int nlh_expr_roots(const nlh_expr *e, int32_t *aroot, int32_t *broot);

/* The Faddeeva function w(z) = exp(-z^2) erfc(-iz), Im z >= 0, in double precision, by Weideman's rational approximation
 * with N = 40 terms -- one formula over the whole half plane, no branch, no library function:
 *   L = sqrt(N/sqrt(2));  Z = (L + iz)/(L - iz);  w = 2 p(Z)/(L - iz)^2 + (1/sqrt(pi))/(L - iz),  p of degree 39.
 * THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, no fused operation), for z = zr + i zi:
 *   dr = L + zi;  di = -zr;  nr = L - zi;  ni = zr;  den = dr*dr + di*di
 *   Zr = (nr*dr + ni*di)/den;  Zi = (ni*dr - nr*di)/den
 *   pr = a[0]; pi = 0;  for k = 1 .. 39:  tr = pr*Zr - pi*Zi;  ti = pr*Zi + pi*Zr;  pr = tr + a[k];  pi = ti
 *   ir = dr/den;  ii = -(di/den);  qr = ir*ir - ii*ii;  qi = 2.0*(ir*ii)
 *   wr = 2.0*(pr*qr - pi*qi) + ISQRTPI*ir;  wi = 2.0*(pr*qi + pi*qr) + ISQRTPI*ii     (ISQRTPI = 0.5641895835477563)
 * L and a[0 .. 39] (highest power first) are literal constants of the library; nlh_faddeeva_table reads them back (either
 * output may be NULL).  Host code and the kernels run the same text, so nlh_faddeeva, nlh_faddeeva_batch and the VOIGT
 * instruction give the same bits, and a restatement in any IEEE language reproduces them.  Accuracy: DESIGN 4e.
 * nlh_faddeeva (host; needs no GPU) refuses Im z < 0 or NaN and NULL outputs with NLH_INVALID_INPUT_ERROR.
 * nlh_faddeeva_batch: DEVICE pointers, a thread per element, on the handle's stream; Im z < 0 is outside its domain (what
 * it writes there is not w).  NLH_ERR_BAD_HANDLE, NLH_INVALID_INPUT_ERROR (count < 0, a NULL array with count > 0). */
int nlh_faddeeva(double re, double im, double *wre, double *wim);
void nlh_faddeeva_table(double *L, double *a40);
int nlh_faddeeva_batch(nlh_handle *h, int64_t count, const double *dre, const double *dim, double *dwre, double *dwim);
typedef struct nlh_expr_ctx {
    const nlh_expr *e;
    int32_t shared_t;     /* dt is [nvar][m], the same abscissae for every problem */
    int32_t m;
    const double *dt;     /* [nvar][nprob][m] (shared_t: [nvar][m]), device; the caller's */
    const double *dy;     /* [nprob][m], device */
    const double *dw;     /* [nprob][m], device, or NULL: no weights */
    int64_t dt_stride;    /* doubles from one variable's block of dt to the next: nprob*m (shared_t: m); 0 means that
                           * value for shared_t and is allowed for one variable (it is never used then) */
} nlh_expr_ctx;
/* The launchers (nlh_device_vecfcn / nlh_device_jacfcn, ctx = nlh_expr_ctx): they enqueue on the stream handed in, never
 * synchronise, allocate nothing (the program travels in the kernel arguments) and may be called from several host threads.
 * A malformed ctx -- NULL e, n != nparams, m != ctx->m, a NULL array, two variables or more without a stride -- returns
 * NLH_INVALID_INPUT_ERROR before any launch. */
int nlh_expr_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                        int32_t m, double *dF);
int nlh_expr_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX,
                        int32_t m, double *dJ);
/* The launch shape of the formula kernels for a program of this depth with n parameters on m rows: host code, needs no GPU;
 * the function the launchers themselves dispatch through.  jac = 0: the residual kernel (chunk = 0).  Reads NLH_EXPR_FORM
 * and NLH_EXPR_CHUNK as the launchers do.  Returns 0, or NLH_INVALID_INPUT_ERROR (depth outside 1 .. 16, n outside 1 .. 32,
 * m < 1, npoints < 0, a NULL output), NLH_ARRAY_SIZE_ERROR as the launchers.
 * flat: 1 the flat form (ppw = 256 / m points per workgroup, nblk = 1), 0 the row form (ppw = 1, nblk = ceil(m / 256) row
 * blocks per point); grid: workgroups, ceil(npoints / ppw) or npoints * nblk; chunk: the Jacobian columns a pass over the
 * program carries, 1 .. min(n, 8) -- the most with which the launch stays within half of the 161,792 bytes of LDS a
 * workgroup may ask for, or 1 where even that does not fit half; lds_bytes: the dynamic LDS of the launch,
 * 8 * (ppw * n + 256 * depth * (1 + chunk)): x of the workgroup's points, the value stack, chunk tangent stacks.  The
 * largest launch is 131,072 bytes (depth 16, n = 32, m = 1, the Jacobian). */
int32_t nlh_expr_plan(int32_t depth, int32_t n, int32_t m, int32_t npoints, int32_t jac,
                      int32_t *flat, int32_t *ppw, int32_t *nblk, int64_t *grid, int32_t *chunk, int64_t *lds_bytes);
/* A formula model as a MODEL object of the device-function kind, from HOST arrays t [nvar][nprob][m] (shared_t: [nvar][m]),
 * y, w (NULL: no weights): the model owns a copy of the program, its context and device copies of the data (the caller may
 * destroy e at once); nlh_dq_model_destroy frees them.  Errors (every entry point below, in this order):
 * NLH_ERR_BAD_HANDLE (NULL handle), NLH_INVALID_INPUT_ERROR (NULL e or array, bad counts), NLH_UNDERDEFINED_PROBLEM_ERROR
 * (m < n). */
int nlh_expr_model_create(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t m, const double *t, int32_t shared_t,
                          const double *y, const double *w, int32_t analytic, nlh_dq_model **model);
/* Model values -- no data term, no weights -- at dt [nvar][nprob][npts] (shared_t: [nvar][npts]) for parameters
 * dx [nprob][n]: dy [nprob][npts].  DEVICE pointers. */
int nlh_expr_eval_batch(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t npts, const double *dt, int32_t shared_t,
                        const double *dx, double *dy);
/* Fit + errors in one call: exactly the composition nlh_curve_fit_batch documents (one helper runs both), with the formula
 * launchers -- solve or bounded solve, covariance with scaled = 1, the zero-weight degrees-of-freedom rule, NaN and rank -1
 * for a problem that did not solve.  The arguments are nlh_curve_fit_batch's, e for (kind, ncomp, nbase). */
int nlh_expr_fit_batch(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                       int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                       const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                       int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                         int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                         const double *xu, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                         nlh_iteration_behavior *ib, int32_t *status);

/* ---- confidence and prediction bands (no counterpart in nonlin v2.2.0): a fit's parameter covariance propagated through
 * any vector function g(x) of the parameters -- the delta method.  With G the Jacobian of g at the solution and C the
 * parameter covariance, var g_i = G_i C G_i^T: the 1-sigma confidence band of the model (g = the model on a plotting grid),
 * the prediction band for a new observation (the same plus a noise variance), the standard error of a derived quantity (g = a
 * formula of the parameters, e.g. a lifetime 1/k, evaluated as a one-row model).
 * nlh_propagate, the kernel: dJ [npoints][n][m], each point's Jacobian column-major exactly as nlh_device_jacfcn writes
 * it; dcov [npoints][n][n]; dnoise [npoints] or NULL; dsd [npoints][m] out.  DEVICE pointers.
 * THE OPERATION ORDER IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  Row i of point p, with
 * J_k = J[p][k][i] and C = cov[p]:
 *   v = 0
 *   for j = 0 .. n-1:   s = 0;  s = s + C[j][k]*J_k for k = 0 .. j-1;  s = 2.0*s;  s = s + C[j][j]*J_j;  v = v + J_j*s
 *   v = v + noise[p] when noise is given;   v < 0.0: v = 0.0 (a NaN passes through);   sd = sqrt(v)
 * A MATRIX IS READ BY ITS LOWER TRIANGLE: only the entries C[j][k] with k <= j (cov[p*n*n + j*n + k]); what nlh_covar and
 * the parameter maps write is exactly symmetric, a caller's own matrix counts as symmetric with that triangle.  No sum
 * crosses a thread -- one thread owns one (point, row) -- so a row's bits depend neither on the workgroup form (row: a
 * workgroup per (point, 256 rows); flat: several points per workgroup while two or more fit, m <= 128;
 * NLH_BAND_FORM = row | flat, environment, read at each call, forces one for the sizes it can hold: flat m <= 256 and
 * n <= 200) nor on where the matrix is kept (packed in LDS while n (n + 1) / 2 doubles fit the 161,792-byte cap, n <= 200;
 * read from global memory beyond) nor on the batch.  Any m, n >= 1.
 * noise is a per-problem VARIANCE added once to every row.  NULL: the confidence band of g.  The fit's chi2 -- with the
 * scaled covariance of an unweighted fit, whose residual variance chi2 estimates -- gives the prediction band of a new
 * observation.  sd is ONE standard deviation: the coverage factor (a Student-t quantile at the fit's degrees of freedom,
 * or the normal 1.96) is the caller's to apply.  A problem whose fit failed has NaN in cov and gets NaN in sd.
 * Errors (every entry point of this section, in this order, before anything is evaluated): NLH_ERR_BAD_HANDLE (NULL
 * handle), NLH_UNDEFINED_FUNCTION_ERROR (NULL fcn), NLH_INVALID_INPUT_ERROR (a negative count, m, n or npts < 1, an unknown
 * model; then, for a batch that is not empty, a NULL required array).  An empty batch returns 0. */
int nlh_propagate(nlh_handle *h, int32_t npoints, int32_t m, int32_t n, const double *dJ, const double *dcov,
                  const double *dnoise, double *dsd);
/* The chain for nprob problems of a launcher pair AT THE GIVEN x (dx [nprob][n], device, not modified): dval = F(x), one
 * launcher call, skipped when dval is NULL (and no forward difference needs it); J by vfh_jac_fcn's rule exactly as
 * nlh_fd_jacobian_device (jacfcn, or forward differences when it is NULL); nlh_propagate.  dcov [nprob][n][n], dnoise
 * [nprob] or NULL, dval [nprob][m] or NULL, dsd [nprob][m].  m < n is fine (a derived quantity is a one-row model).  The
 * Jacobian lives in a workspace of the handle that no solver uses, at most 1 GiB of it per call (NLH_BAND_SCRATCH,
 * environment, read at each call: fewer bytes; tests): beyond it the problems go in slices, the launchers seeing dprob, dX
 * and the outputs offset as in every sliced call.  A problem's bits do not depend on the batch it sits in. */
int nlh_propagate_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                               nlh_device_jacfcn jacfcn, void *ctx, const double *dx, const double *dcov,
                               const double *dnoise, double *dval, double *dsd);
/* ... behind HOST arrays x, cov, noise, val, sd. */
int nlh_propagate_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                 nlh_device_jacfcn jacfcn, void *ctx, const double *x, const double *cov,
                                 const double *noise, double *val, double *sd);
/* nlh_curve_eval_batch / nlh_expr_eval_batch plus the band: the model -- no data term, no weights -- at arbitrary abscissae
 * dt (shapes as the eval calls document) with its analytic Jacobian, on a context of the call's own.  dy [nprob][npts] (the
 * bits of the eval call) may be NULL; dsd [nprob][npts].  DEVICE pointers.  After a fit with a parameter map, a separable
 * fit, a loss or Poisson counts the one-call fits return full-size x and cov: these two apply as they are. */
int nlh_curve_band_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t npts,
                         const double *dt, int32_t shared_t, const double *dx, const double *dcov, const double *dnoise,
                         double *dy, double *dsd);
int nlh_expr_band_batch(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t npts, const double *dt, int32_t shared_t,
                        const double *dx, const double *dcov, const double *dnoise, double *dy, double *dsd);
/* ... for every problem of a launcher-backed model object (curve, formula, a user's launchers, any wrapping model): its
 * jacfcn if it has one, forward differences otherwise; host arrays x [nprob][n], cov [nprob][n][n], noise [nprob] or NULL,
 * val [nprob][m] or NULL, sd [nprob][m].  val is the model's F(x): a curve or formula model created with y = 0 and no
 * weights gives the model values.  A dense-quadratic model (the only kind a device set deals over several devices) is
 * refused with NLH_INVALID_INPUT_ERROR, as the wrapping models refuse it.  What the Fortran shim's
 * least_squares_solver%propagate_batch calls. */
int nlh_dq_model_propagate(nlh_handle *h, const nlh_dq_model *model, const double *x, const double *cov,
                           const double *noise, double *val, double *sd);

/* ---- parameter maps (no counterpart in nonlin v2.2.0): fixed and tied parameters for ANY device model.  The model keeps
 * its N FULL parameters; the solver sees n <= N FREE unknowns.  Each full parameter k is free, fixed at a per-problem
 * value, or tied to another parameter: p_k = scale_k*p_src + offset_k.  The map is a pair of wrapping launchers around any
 * inner launcher pair (built-in curve, formula, a user's own), so everything that takes launchers works through it:
 * nlh_lm_solve_batch_device, nlh_cls_solve_batch_device, nlh_lm_covariance_batch_device, nlh_fd_jacobian_device and the
 * model objects.  With forward differences the library then builds n + 1 points per Jacobian instead of N + 1.
 * Free parameters are numbered in ascending full index: free unknown j is the j-th free full parameter.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation:
 *   expand    (free x[n] -> full p[N])  first every free p_k = x[index_k] and every fixed p_k = full_k (full: the caller's
 *             array of full parameters); then, tied k ascending:  u = scale_k*p_src;  p_k = u + offset_k
 *   gather    (full -> free)  x[j] = full[free_to_full[j]]
 *   contract  (inner Jacobian Jf, m x N -> J, m x n)  for each free j:  v = Jf[:, free_to_full[j]];  then, for every tied k
 *             in ascending k whose source is that parameter:  v = v + scale_k*Jf[:, k].  Columns of fixed parameters, and
 *             of parameters tied to fixed ones, are not read.
 *   covariance of the full parameters from the free one: the factor g_k is 1.0 for a free parameter, scale_k for a tie to a
 *             free source and absent otherwise (j_k: the free number of k, or of its source);
 *             cov_full[k][l] = (g_k*cov[j_k][j_l])*g_l;  sigma_full[k] = fabs(g_k)*sigma[j_k];  rows, columns and sigmas of
 *             parameters without a factor are +0.0.  A problem that did not solve has NaN in every entry (and rank -1).
 * No sum crosses a row: a row's bits do not depend on the launch, the batch or the workgroup form. ---- */
#define NLH_PMAP_FREE  0
#define NLH_PMAP_FIXED 1
#define NLH_PMAP_TIED  2
#define NLH_PMAP_MAX_N 8192            /* = NLH_CURVE_MAX_N */
typedef struct nlh_pmap nlh_pmap;
/* The map object (host code, needs no GPU; nlh_pmap_gather_batch, _expand_batch and _cov_batch keep a device copy of its
 * tables in it from their first use, which nlh_pmap_destroy frees).
 * kind [nfull]: NLH_PMAP_*; src, scale, offset [nfull] are read only at tied positions, and all three may be NULL when nothing is tied.  Refused with NLH_INVALID_INPUT_ERROR, *pm left NULL:
 * nfull < 1 or > NLH_PMAP_MAX_N; a kind outside 0 .. 2; a tie whose source is out of range, is itself, or is itself tied
 * (no chains); a scale or offset that is not finite; a tie with scale 0.0 (that is a fixed parameter: say so); no free
 * parameter at all.  A tie to a FIXED source is allowed: a derived constant. */
int  nlh_pmap_create(int32_t nfull, const int32_t *kind, const int32_t *src, const double *scale, const double *offset, nlh_pmap **pm);
void nlh_pmap_destroy(nlh_pmap *pm);
void nlh_pmap_shape(const nlh_pmap *pm, int32_t *nfull, int32_t *nfree, int32_t *ntied);     /* any output may be NULL */
/* Read-back, for restatements (any output may be NULL): kind, index, scale, offset [nfull], free_to_full [nfree].
 * index[k]: the free number for a free k, the source's full index for a tied k, -1 for a fixed k; scale / offset are
 * 1.0 / 0.0 where k is not tied. */
int  nlh_pmap_tables(const nlh_pmap *pm, int32_t *kind, int32_t *index, double *scale, double *offset, int32_t *free_to_full);
/* The wrapping launchers.  nlh_pmap_wrap makes their context on the handle's device: device copies of the tables, scratch,
 * the inner pair (fcn, jac -- NULL: none --, inner_ctx; all stay the caller's and must outlive the context).  dfull is a
 * DEVICE array [nprob][N], or [N] with shared_full != 0, the caller's, read at fixed positions only: point q reads row
 * dprob[q] (a NULL dprob means q itself).
 *   nlh_pmap_device_fcn  expand into scratch P [npoints][N]; the inner fcn with n = N straight into the caller's dF
 *   nlh_pmap_device_jac  expand; the inner jac into scratch Jf [npoints][N][m]; contract into dJ.  With a NULL inner jac it
 *                        returns an error: pass a NULL jacfcn to the solver instead (forward differences over the n free
 *                        unknowns).
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n != nfree or m < 1 returns non-zero before any launch.  An inner error comes back as it
 * is, with no further launch; the inner launcher is called after the expansion of its points has been enqueued, so by then
 * the context's own scratch has been written, and nothing of the caller's.
 * Scratch belongs to the context: one buffer per stream, grown on demand, reused, kept until nlh_pmap_unwrap, at most
 * 1 GiB per call and so per stream (a context called on s streams -- the handle's and a solver's sub-batch workers -- holds
 * up to s GiB).  A call that needs more runs in slices of points, each calling the inner launcher with offset dprob, dX and
 * dJ -- the same bits.  Growing a buffer frees and allocates device memory, which waits for the device: it happens in the
 * first calls on a stream, not in every call.
 * NLH_PMAP_SCRATCH = bytes (environment, read at each call; tests) lowers the cap.  The contraction runs a thread per
 * (point, row) in the two workgroup forms of the curve kernels -- a workgroup per (point, 256 rows), or several points per
 * workgroup while two or more fit 256 threads; NLH_PMAP_FORM = row | flat forces one for the sizes it can hold (flat:
 * m <= 256) -- and splits the free columns over a second grid dimension while the launch would otherwise be fewer than four
 * workgroups per compute unit (NLH_PMAP_SPLIT = number of column groups overrides; tests). */
typedef struct nlh_pmap_ctx nlh_pmap_ctx;
int  nlh_pmap_wrap(nlh_handle *h, const nlh_pmap *pm, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx,
                   const double *dfull, int32_t shared_full, nlh_pmap_ctx **out);
void nlh_pmap_unwrap(nlh_pmap_ctx *c);
int  nlh_pmap_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_pmap_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The three small steps around a solve made through the launchers by hand, on DEVICE arrays (the handle's stream):
 *   gather   dfull [nprob][N] -> dx [nprob][n]
 *   expand   dx [nprob][n], dfull [nprob][N] (shared_full: [N]) -> dp [nprob][N] (dp may not alias dfull; dfull may be
 *            NULL for a map without a fixed parameter, as for nlh_pmap_wrap)
 *   cov      dcov [nprob][n][n], dsigma [nprob][n] -> dcov_full [nprob][N][N], dsigma_full [nprob][N]; either pair may be
 *            NULL; dfail [nprob] int32 or NULL: a non-zero entry marks a problem that did not solve (NaN in every entry). */
int  nlh_pmap_gather_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dfull, double *dx);
int  nlh_pmap_expand_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dx, const double *dfull,
                           int32_t shared_full, double *dp);
int  nlh_pmap_cov_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dcov, const double *dsigma,
                        const int32_t *dfail, double *dcov_full, double *dsigma_full);
/* One-call fits through a map: nlh_curve_fit_batch / nlh_expr_fit_batch plus pm (NULL: exactly the old entry points, bit
 * for bit).  Everything the caller sees is FULL: dx [nprob][N] in and out, dsigma [nprob][N], dcov [nprob][N][N], host xl / xu
 * [N].  On entry a fixed parameter keeps the value dx holds for that problem (the values may differ per problem; the entry
 * point works on a private copy); tied positions of dx are ignored on entry; on exit dx is the expansion of the solution, for
 * every problem: one that is refused on its degrees of freedom keeps its free and fixed values, and its tied positions
 * hold the ties evaluated at them.
 * Bound entries at fixed and tied positions are not read.  The composition: gather; the solve over the n = nfree free
 * unknowns with the wrapping launchers; the covariance at the solution; expand; the covariance of the full parameters.
 * The degrees of freedom, m >= n (NLH_UNDERDEFINED_PROBLEM_ERROR otherwise), m > n for errors and (m - n) / dof all use
 * n = nfree; everything else is the old composition, zero-weight padding rule included.  Errors, in this order: the old
 * entry point's for the handle and the model; NLH_INVALID_INPUT_ERROR for a map whose nfull is not the model's N;
 * NLH_UNDERDEFINED_PROBLEM_ERROR (m < nfree); NLH_INVALID_INPUT_ERROR (a NULL array; errors asked for with m <= nfree). */
int nlh_curve_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                             int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                             const double *xl, const double *xu, const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma,
                             double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                               int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                               const double *xl, const double *xu, const nlh_pmap *pm, double *x, double *fvec, double *sigma,
                               double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                            const double *xu, const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma, double *dcov,
                            double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                              const double *xu, const nlh_pmap *pm, double *x, double *fvec, double *sigma, double *cov,
                              double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
/* A device-function MODEL of nfree unknowns over a launcher-backed inner model (device-function, curve or formula; a
 * dense-quadratic model: NLH_INVALID_INPUT_ERROR), which must outlive it.  full: HOST [nprob][N], or [N] with shared_full;
 * the model owns its device copy and its wrapping context.  Every nlh_dq_model_* solver and nlh_dq_model_lm_covariance
 * then takes it (x [nprob][nfree]).  Errors: NLH_ERR_BAD_HANDLE, then NLH_INVALID_INPUT_ERROR (a NULL argument, a
 * dense-quadratic inner model, nfull != the inner model's n), NLH_UNDERDEFINED_PROBLEM_ERROR is left to the solvers. */
int nlh_pmap_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_pmap *pm, const double *full, int32_t shared_full,
                          nlh_dq_model **model);

/* ---- robust losses (no counterpart in nonlin v2.2.0): Huber, soft-L1 and Cauchy fits for ANY device model.  A measured
 * spectrum with a cosmic-ray spike or a dead bin pulls a plain least-squares fit; a robust loss rho bounds what one residual
 * can contribute.  Like a parameter map, a loss is a pair of wrapping launchers around any inner launcher pair (built-in
 * curve, formula, a user's own, a map's), so everything that takes launchers works through it unchanged:
 * nlh_lm_solve_batch_device, nlh_cls_solve_batch_device, nlh_lm_covariance_batch_device, nlh_fd_jacobian_device, the model
 * objects and the maps.  The wrapped residual is  rho~(r) = c*sign(r)*sqrt(rho((r/c)^2)),  so ||rho~||^2 = c^2 * sum rho and
 * the unchanged solver minimises the robust cost itself; a forward-difference Jacobian of the wrapped function is the right
 * Jacobian.  c > 0 is the scale: residuals well inside it are treated as least squares treats them.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  r the inner residual,
 * u = r / c, a = fabs(u):
 *   kind                               out                                                      g (row factor of J)      wgt = rho'
 *   NLH_LOSS_LINEAR                    r                                                        1.0                      1.0
 *   NLH_LOSS_HUBER    a <= 1.0         r (bit for bit)                                          1.0                      1.0
 *                     else (NaN too)   v = 2.0*a; v = v - 1.0; s = sqrt(v); c*copysign(s, u)    1.0/s                    1.0/a
 *   NLH_LOSS_SOFT_L1                   z = u*u; s = sqrt(1.0 + z); k = sqrt(2.0/(s + 1.0));
 *                                      c*(u*k)                                                  1.0/(s*k)                1.0/s
 *   NLH_LOSS_CAUCHY   z = u*u == 0.0   r                                                        1.0                      1.0
 *                     else             l = log1p(z); s = sqrt(l); c*copysign(s, u)              q = 1.0 + z; wgt = 1.0/q;
 *                                                                                               g = (wgt*a)/s            wgt
 * The Jacobian rule is J'[i][j] = g_i * J[i][j], one multiply per entry, g_i from the inner residual at the same point.  No
 * sum crosses a row: a row's bits do not depend on the launch, the batch or the workgroup form.  Huber and soft-L1 use only
 * + - * / sqrt and are reproducible bit for bit; Cauchy carries the device library's log1p.  A row with r = +-0 stays +-0
 * under every kind, so zero-weight padding keeps working.  Documented domain: |r| < 1e150 * c.
 * The scale is per problem, dscale [nprob] on the DEVICE -- point q reads dscale[dprob[q]] (a NULL dprob means q itself) --,
 * or one value with shared_scale != 0.  On device arrays a scale that is not finite or not positive makes every residual,
 * g and wgt of that problem NaN (every kind but LINEAR, which reads no scale: dscale may then be NULL); entry points that
 * take HOST scales refuse one with NLH_INVALID_INPUT_ERROR. ---- */
#define NLH_LOSS_LINEAR  0
#define NLH_LOSS_HUBER   1
#define NLH_LOSS_SOFT_L1 2
#define NLH_LOSS_CAUCHY  3
/* The wrapping launchers.  nlh_loss_wrap makes their context on the handle's device; the inner pair (fcn, jac -- NULL: none
 * --, inner_ctx) and dscale stay the caller's and must outlive the context.
 *   nlh_loss_device_fcn  the inner fcn straight into the caller's dF; then the table's out, in place.  Needs no scratch
 *                        beyond a problem list when dprob is NULL.
 *   nlh_loss_device_jac  the inner fcn into scratch R [npoints][m]; the inner jac straight into the caller's dJ; then
 *                        every row of dJ times its g, in place.  With a NULL inner jac it returns an error: pass a NULL
 *                        jacfcn to the solver instead (forward differences of the wrapped residual).
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n < 1 or m < 1 returns non-zero before any launch.  An inner error comes back as it is,
 * with no further launch.  NLH_LOSS_LINEAR launches no kernel of the table and calls no inner fcn for a Jacobian: the inner
 * pair's output is the caller's as it is.  Every kind, LINEAR included, hands the inner launcher a problem list of its own when
 * dprob is NULL (the built-in launchers want one), so a wrapped pair takes the same calls whatever its kind.
 * Scratch belongs to the context, exactly as a parameter map's: one buffer per stream, grown on demand, reused, kept
 * until nlh_loss_unwrap, at most 1 GiB per call and so per stream; a call that needs more runs in slices of points -- the
 * same bits.  NLH_LOSS_SCRATCH = bytes (environment, read at each call; tests) lowers the cap.  The row scaling runs a
 * thread per (point, row) in the two workgroup forms of the curve kernels -- a workgroup per (point, 256 rows), or several
 * points per workgroup while two or more fit 256 threads (m <= 128); NLH_LOSS_FORM = row | flat forces one for the sizes
 * it can hold (flat: m <= 256) -- and splits the columns over a second grid dimension while the launch would otherwise be
 * fewer than four workgroups per compute unit (NLH_LOSS_SPLIT = number of column groups overrides; tests). */
typedef struct nlh_loss_ctx nlh_loss_ctx;
int  nlh_loss_wrap(nlh_handle *h, int32_t kind, const double *dscale, int32_t shared_scale, nlh_device_vecfcn fcn,
                   nlh_device_jacfcn jac, void *inner_ctx, nlh_loss_ctx **out);
void nlh_loss_unwrap(nlh_loss_ctx *c);
int  nlh_loss_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_loss_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The table applied to raw residuals dr [nprob][m] on the DEVICE (the handle's stream): dout, dg, dwgt [nprob][m], each
 * may be NULL; dout may be dr itself.  wgt = rho' is 1.0 for a residual the loss leaves alone and falls towards 0.0 for an
 * outlier: it is what a user thresholds to flag outliers. */
int  nlh_loss_apply_batch(nlh_handle *h, int32_t kind, int32_t nprob, int32_t m, const double *dscale, int32_t shared_scale,
                          const double *dr, double *dout, double *dg, double *dwgt);
/* One-call fits with a loss: the _pmap entry points plus (loss, dscale, shared_scale) after pm.  NLH_LOSS_LINEAR is the
 * _pmap entry point, bit for bit (dscale is not read).  The composition is fixed, and the bits depend on its order: the
 * loss wraps the model's launchers directly, and the map, if any, wraps the result.  What comes back is that of the
 * TRANSFORMED problem: dfvec is rho~ (not the raw residual: nlh_curve_eval_batch / nlh_expr_eval_batch give the model, and
 * nlh_loss_apply_batch the weights), dchi2 is sum rho~^2 / dof = c^2 * sum rho / dof, and dsigma / dcov are the scaled
 * covariance of the transformed problem, (J'^T J')^-1 * chi2.  Errors, in this order: the _pmap entry point's up to
 * NLH_UNDERDEFINED_PROBLEM_ERROR; NLH_INVALID_INPUT_ERROR for a loss outside 0 .. 3; then the _pmap entry point's for NULL
 * arrays (dscale, or scale, included).  The _h forms take HOST scale [nprob] (or [1]) and refuse, with
 * NLH_INVALID_INPUT_ERROR, one that is not finite or not positive. */
int nlh_curve_fit_batch_loss(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                             int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                             const double *xl, const double *xu, const nlh_pmap *pm, int32_t loss, const double *dscale,
                             int32_t shared_scale, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                             int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                               int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                               const double *xl, const double *xu, const nlh_pmap *pm, int32_t loss, const double *scale,
                               int32_t shared_scale, double *x, double *fvec, double *sigma, double *cov, double *chi2,
                               int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_loss(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                            const double *xu, const nlh_pmap *pm, int32_t loss, const double *dscale, int32_t shared_scale,
                            double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                            nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                              const double *xu, const nlh_pmap *pm, int32_t loss, const double *scale, int32_t shared_scale,
                              double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                              nlh_iteration_behavior *ib, int32_t *status);
/* A device-function MODEL with a loss over a launcher-backed inner model (device-function, curve, formula or mapped; a
 * dense-quadratic model: NLH_INVALID_INPUT_ERROR), which must outlive it.  scale: HOST [nprob], or [1] with shared_scale
 * (NULL allowed for NLH_LOSS_LINEAR); the model owns its device copy and its wrapping context.  Every nlh_dq_model_* solver
 * and nlh_dq_model_lm_covariance then takes it.  Errors: NLH_ERR_BAD_HANDLE, then NLH_INVALID_INPUT_ERROR (a NULL
 * argument, a dense-quadratic inner model, a kind outside 0 .. 3, a scale that is not finite or not positive). */
int nlh_loss_model_create(nlh_handle *h, const nlh_dq_model *inner, int32_t kind, const double *scale, int32_t shared_scale,
                          nlh_dq_model **model);

/* ---- Poisson likelihood fits (no counterpart in nonlin v2.2.0): counting data for ANY device model.  For counts -- photon
 * counting decays, histogrammed spectra, low-dose images -- least squares is the wrong estimator: weighting by 1/sqrt(y)
 * biases a decay rate by several per cent at 50 counts, and the unweighted fit wastes information.  The Poisson deviance
 *   sum_i D_i,  D_i = 2 [mu_i - y_i + y_i log(y_i / mu_i)]  ( = -2 log L up to a constant of the data)
 * is a sum of squares of the DEVIANCE RESIDUALS d_i = sign(mu_i - y_i) * sqrt(D_i), so the unchanged LM and bounded solvers
 * minimise -2 log L when they are handed d and its Jacobian.  Like a loss, this is a pair of wrapping launchers around any
 * inner launcher pair (built-in curve, formula, a user's own), so everything that takes launchers works through it:
 * nlh_lm_solve_batch_device, nlh_cls_solve_batch_device, nlh_lm_covariance_batch_device, nlh_fd_jacobian_device, the model
 * objects and the maps (a map wraps the Poisson pair, not the other way round).
 * The inner pair is an ordinary least-squares model bound WITHOUT weights, so that its residual is r = model - y.  The
 * wrapper is given the same counts dy [nprob][m], an optional mask dw [nprob][m] of 0.0 / 1.0 (NULL: every row counts) and a
 * floor mu_floor > 0, all on the DEVICE; point q reads row dprob[q] of dy and dw (a NULL dprob means q itself).
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  Per row, f = mu_floor:
 *   f not finite or not positive          out = g = NaN, every row (the entry points that take a HOST floor refuse it)
 *   masked: dw given and w == 0.0         out = +0.0, g = 0.0; the Jacobian row is STORED as +0.0, not multiplied.  (The mask is
 *                                         the wrapper's, because a real row with y = 0 and mu -> 0 has inner residual 0 too.)
 *   w neither 0.0 nor 1.0, y < 0.0 or y not finite            out = g = NaN
 *   floor       mu = r + y; low = mu < f; rr = low ? f - y : r
 *   y == 0.0    D = 2.0*rr; s = sqrt(D); d = s; g = 1.0/s
 *   y >  0.0    e = rr/y; a = fabs(e); u = (rr + y)/y
 *               a <= 2^-6   q = 1.0/13; q = 1.0/k - e*q for k = 12 .. 2 (the constants 1.0/k); h = (e*e)*q
 *                           -- the series of e - log(1 + e), no library function
 *               otherwise   l = (e < -0.5) ? log(u) : log1p(e); h = e - l
 *               D = (2.0*y)*h; s = sqrt(D); d = copysign(s, e)
 *               g = (e == 0.0) ? 1.0/sqrt(y) : a/(u*s)                     ( = (1 - y/mu) / d )
 *   result      low: out = d + g*(mu - f);  otherwise out = d.             J'[i][j] = g_i * J[i][j]
 * Below the floor out is the C1 linear extension of d: a clamp would leave the solver without a slope, NaN would kill the
 * problem.  No sum crosses a row: a row's bits do not depend on the launch, the batch or the workgroup form.  Rows that reach
 * no library function (masked, y = 0, the series, and floor rows whose base point is one of those) are reproducible bit for
 * bit; the others carry the device library's log1p or log, and d and g stay within 2^-44 relative of the exact values over
 * the documented domain: y in [0.01, 1e6], |e| in [1e-12, 1e6], e + 1 >= 1e-12 (DESIGN.md 4h derives the bound). ---- */
typedef struct nlh_pois_ctx nlh_pois_ctx;
/* The wrapping launchers.  nlh_pois_wrap makes their context on the handle's device; the inner pair (fcn, jac -- NULL: none
 * --, inner_ctx), dy and dw stay the caller's and must outlive the context.  mu_floor is not checked here (the table's NaN).
 *   nlh_pois_device_fcn  the inner fcn straight into the caller's dF; then the table's out, in place.
 *   nlh_pois_device_jac  the inner fcn into scratch R [npoints][m]; the inner jac straight into the caller's dJ; then
 *                        every row of dJ times its g, in place.  With a NULL inner jac it returns
 *                        NLH_UNDEFINED_FUNCTION_ERROR: pass a NULL jacfcn to the solver instead (forward differences of
 *                        the wrapped residual).
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n < 1 or m < 1 returns non-zero before any launch.  An inner error comes back as it is,
 * with no further launch.  When dprob is NULL the launchers build a problem list of their own, for the inner launcher and for
 * the rows of dy and dw.  Scratch belongs to the context, exactly as a loss's: one buffer per stream, grown on demand, kept
 * until nlh_pois_unwrap, at most 1 GiB per call; a call that needs more runs in slices of points -- the same bits.
 * NLH_POIS_SCRATCH = bytes lowers the cap, NLH_POIS_FORM = row | flat forces a workgroup form for the sizes it can hold,
 * NLH_POIS_SPLIT = number of column groups overrides the column split (environment, read at each call; tests). */
int  nlh_pois_wrap(nlh_handle *h, const double *dy, const double *dw, double mu_floor, nlh_device_vecfcn fcn,
                   nlh_device_jacfcn jac, void *inner_ctx, nlh_pois_ctx **out);
void nlh_pois_unwrap(nlh_pois_ctx *c);
int  nlh_pois_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_pois_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The table applied to raw residuals dr [nprob][m] = model - y on the DEVICE (the handle's stream): dout, dg and the row
 * deviances ddev (the table's D: the deviance at max(mu, f); 0.0 on a masked row) [nprob][m], each may be NULL; dout may be
 * dr itself. */
int  nlh_pois_apply_batch(nlh_handle *h, int32_t nprob, int32_t m, const double *dy, const double *dw, double mu_floor,
                          const double *dr, double *dout, double *dg, double *ddev);
/* One-call Poisson fits: the _pmap entry points plus mu_floor after pm; dw (w) now means the 0 / 1 mask, and the model itself
 * is bound without weights.  The composition is fixed: the Poisson pair wraps the model's launchers, and the map, if any,
 * wraps the result.  What comes back: dfvec is the deviance residual d; dchi2 is the deviance / dof = (sum of d_i^2, i
 * ascending, sequential) / dof with dof = unmasked rows - n (a problem with dof <= 0 gets NLH_INVALID_INPUT_ERROR in its
 * status, as with zero weights); dsigma / dcov are UNSCALED, nlh_lm_covariance_batch_device with scaled = 0: (J'^T J')^-1 is the
 * inverse Fisher information at the fit, and Poisson noise has no free variance.  Errors, in this order: the _pmap entry
 * point's; then NLH_INVALID_INPUT_ERROR for a mu_floor that is not finite or not positive.  The _h forms also refuse, with
 * NLH_INVALID_INPUT_ERROR, a w outside {0, 1} and, on a row the mask keeps, a y that is negative or not finite (a masked
 * row may hold anything there too: NaN padding of ragged data is accepted). */
int nlh_curve_fit_batch_pois(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                             int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                             const double *xl, const double *xu, const nlh_pmap *pm, double mu_floor, double *dx,
                             double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                             nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_pois_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                               int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                               const double *xl, const double *xu, const nlh_pmap *pm, double mu_floor, double *x,
                               double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                               nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_pois(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                            const double *xu, const nlh_pmap *pm, double mu_floor, double *dx, double *dfvec, double *dsigma,
                            double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_pois_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                              const double *xu, const nlh_pmap *pm, double mu_floor, double *x, double *fvec, double *sigma,
                              double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
/* A device-function MODEL minimising the Poisson deviance over a launcher-backed inner model (device-function, curve or
 * formula, created WITHOUT weights; a dense-quadratic model: NLH_INVALID_INPUT_ERROR), which must outlive it.  y, w (NULL: no
 * mask): HOST [nprob][m]; the model owns its device copies and its wrapping context.  Every nlh_dq_model_* solver and
 * nlh_dq_model_lm_covariance (pass scaled = 0) then takes it; a mapped model may be made over it.  Errors: NLH_ERR_BAD_HANDLE,
 * then NLH_INVALID_INPUT_ERROR (a NULL argument, a dense-quadratic inner model, a bad mu_floor, a w outside {0, 1}, a y that
 * is negative or not finite on a row the mask keeps). */
int nlh_pois_model_create(nlh_handle *h, const nlh_dq_model *inner, const double *y, const double *w, double mu_floor,
                          nlh_dq_model **model);

/* ---- instrument-response fits (no counterpart in nonlin v2.2.0): ANY device model convolved with a kernel along its rows.
 * A detector does not record the model: it records the model convolved with the instrument's response -- the IRF of a
 * photon-counting set-up for a decay, the line shape of a spectrometer for a spectrum.  Fitting the convolved model
 * ("reconvolution") uses every bin; the alternative, fitting only the tail the response does not touch, is biased or has
 * nothing left to fit when the lifetime is comparable to the response (README, the study table).  Like a loss, this is a
 * pair of wrapping launchers around any inner launcher pair, so everything that takes launchers works through it; a loss, the
 * Poisson pair, a map or a group wrap the convolved pair, not the other way round.
 * The inner pair follows the Poisson convention: an ordinary least-squares model bound WITHOUT weights to the same y, so that
 * its residual is r = model - y.  The wrapper is given dy [nprob][m], optional weights dw [nprob][m] (NULL: none) and the
 * kernel, all on the DEVICE; point q belongs to problem p = dprob ? dprob[q] : q and reads row p of dy and dw and the taps
 * kp = shared_k ? k : k + p L.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  The convolution c of one column
 * v [0 .. m-1] (the model values, or one column of the inner Jacobian), row i:
 *   acc = +0.0
 *   for j = 0 .. L-1 ascending:   s = i + origin - j
 *       NLH_CONV_ZERO: s outside 0 .. m-1 -> the tap is SKIPPED (nothing multiplied, nothing added)
 *       NLH_CONV_HOLD: s = min(max(s, 0), m-1)
 *       t = kp[j] * v[s];  acc = acc + t
 *   c_i = acc
 *   residual    mu_s = r_s + y_s (one add); c over mu; out_i = c_i - y_i; with weights out_i = w_i * out_i
 *   Jacobian    J'[i][j] = c_i over column j of the inner Jacobian; with weights w_i * c_i
 *   weights     a row with w_i == 0.0 is STORED as +0.0 in dF and in every column of dJ, not multiplied
 * No sum crosses threads: every output is one sequential chain, so its bits do not depend on the batch, the workgroup form,
 * the row tile or the slice, and a numpy restatement reproduces them bit for bit.  Two consequences:
 *   - the model is convolved over ALL m rows, whatever their weights: the rows must lie on one uniform grid, and y must be
 *     finite on EVERY row, padded rows included -- a NaN in y_s reaches every row that reads s;
 *   - with NLH_CONV_ZERO a constant baseline ramps up over the first taps of a causal kernel: mask the pre-pulse bins with
 *     w = 0, or use NLH_CONV_HOLD when the window starts on a flat part.
 * The kernel is used as given, not normalised. ---- */
#define NLH_CONV_MAX_L   1024
#define NLH_CONV_ZERO    0      /* rows outside 0 .. m-1 contribute nothing */
#define NLH_CONV_HOLD    1      /* rows outside take the nearest edge row's value */
typedef struct nlh_conv {
    int32_t L;            /* taps, 1 .. NLH_CONV_MAX_L (L > m is allowed) */
    int32_t origin;       /* 0 .. L-1: tap `origin` sits on the output row.  0 = causal (IRF), (L-1)/2 = centred (line shape) */
    int32_t ext;          /* NLH_CONV_ZERO | NLH_CONV_HOLD */
    int32_t shared_k;     /* k is [L], one kernel for every problem; otherwise [nprob][L] */
    const double *k;      /* device pointer; used as given, not normalised */
} nlh_conv;
typedef struct nlh_conv_ctx nlh_conv_ctx;
/* The wrapping launchers.  nlh_conv_wrap makes their context on the handle's device; *cv is copied, while its k, the inner
 * pair (fcn, jac -- NULL: none --, inner_ctx), dy and dw stay the caller's and must outlive the context.
 *   nlh_conv_device_fcn  the inner fcn into scratch R [npoints][m]; then the table's residual into the caller's dF.
 *   nlh_conv_device_jac  the inner jac into scratch Jf [npoints][n][m]; then the table's Jacobian into dJ [npoints][n][m],
 *                        out of place; every entry is written.  With a NULL inner jac it returns
 *                        NLH_UNDEFINED_FUNCTION_ERROR: pass a NULL jacfcn to the solver instead (forward differences of
 *                        the wrapped residual).
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n < 1, m < 1 or a bad L / origin / ext returns non-zero before any launch.  An inner error
 * comes back as it is, with no further launch.  When dprob is NULL the launchers build a problem list of their own.  Scratch
 * belongs to the context, exactly as a loss's: one buffer per stream, grown on demand, kept until nlh_conv_unwrap, at most
 * 1 GiB per call; a call that needs more runs in slices of points -- the same bits.  NLH_CONV_SCRATCH = bytes lowers the cap,
 * NLH_CONV_FORM = row | flat forces a workgroup form for the sizes it can hold (flat: m <= 256), NLH_CONV_SPLIT = number of
 * column groups overrides the column split (environment, read at each call; tests).
 * Errors of nlh_conv_wrap: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a NULL out, dy, cv or cv->k, L outside 1 ..
 * NLH_CONV_MAX_L, origin outside 0 .. L-1, ext outside 0 .. 1); NLH_UNDEFINED_FUNCTION_ERROR (a NULL fcn). */
int  nlh_conv_wrap(nlh_handle *h, const nlh_conv *cv, const double *dy, const double *dw, nlh_device_vecfcn fcn,
                   nlh_device_jacfcn jac, void *inner_ctx, nlh_conv_ctx **out);
void nlh_conv_unwrap(nlh_conv_ctx *c);
int  nlh_conv_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_conv_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The bare convolution c of arbitrary columns dv [nprob][ncol][m] on the DEVICE (the handle's stream) into dout of the same
 * shape, dout != dv; problem p uses the taps of p.  The convolved model for plotting is nlh_curve_eval_batch (or the
 * formula's) followed by this with ncol = 1. */
int  nlh_conv_apply_batch(nlh_handle *h, const nlh_conv *cv, int32_t nprob, int32_t m, int32_t ncol, const double *dv, double *dout);

/* ---- global fits: parameters shared across the data sets of a group, for any device model -------------------------------
 * A GROUP is G = nsets data sets of one inner model with N = nfull parameters, S = nshared of which have one value for the
 * whole group; the other L = N - S are free per data set.  A tie (nlh_pmap) links parameters inside one problem; a group
 * links them across problems.  G consecutive inner problems p G + g of m rows are, as they lie in memory, ONE outer problem
 * p of M = G m rows: y, weights and fvec [ngroup G][m] are [ngroup][M] as they stand.
 * THE ORDER OF THE OUTER UNKNOWNS IS PART OF THE INTERFACE: n = S + G L of them,
 *   the shared parameters first, in ascending inner index;
 *   then, for data set g = 0 .. G - 1, its local parameters in ascending inner index.
 * nlh_group_index(g, set, k) is the outer unknown of inner parameter k of data set `set` (the same for every set when k is
 * shared; -1 out of range).  S may be 0 (nothing shared: a block-diagonal problem) or N (everything shared).
 * The group object is host code and needs no GPU (nlh_group_gather_batch, _expand_batch and _sigma_batch keep a device copy of
 * its tables in it from their first use, which nlh_group_destroy frees).  shared [nshared]: distinct inner indices, in any
 * order.  Refused with NLH_INVALID_INPUT_ERROR, *g left NULL: a NULL argument (shared may be NULL when nshared = 0), nfull
 * < 1 or > NLH_PMAP_MAX_N, nshared outside 0 .. nfull, an index out of range or repeated, nsets < 1, n beyond int32.
 * A group's Jacobian is DENSE to the solver, [n][M], though the local columns of a data set are zero in every other data
 * set's rows: its size and the solve's cost grow as G^2 and G^3.  The practical range is G of tens, not thousands. */
typedef struct nlh_group nlh_group;
int  nlh_group_create(int32_t nfull, int32_t nshared, const int32_t *shared, int32_t nsets, nlh_group **g);
void nlh_group_destroy(nlh_group *g);
void nlh_group_shape(const nlh_group *g, int32_t *nfull, int32_t *nshared, int32_t *nsets,
                     int32_t *nouter);                                                       /* any output may be NULL */
int32_t nlh_group_index(const nlh_group *g, int32_t set, int32_t k);
/* The wrapping launchers.  nlh_group_wrap makes their context on the handle's device around ANY inner launcher pair (a
 * curve's, a formula's, a loss's, a Poisson pair's, a map's, a user's own) whose context indexes its data by inner problem;
 * jac may be NULL.  nlh_group_device_fcn / _jac are then launchers of the outer problem with `out` as their context: outer
 * point q of outer problem p (dprob ? dprob[q] : q) stands for the G inner points q G + g of inner problems p G + g.
 *   nlh_group_device_fcn  expand into scratch P [npoints G][N] and the inner problem list; the inner fcn with npoints G
 *                         points, n = N and m = M / G STRAIGHT INTO the caller's dF (no copy)
 *   nlh_group_device_jac  expand; the inner jac into scratch Jf [npoints G][N][m]; scatter into dJ [npoints][n][M]
 *                         (column-major, ld = M): a shared column takes rows g m + i from every data set, the local column
 *                         (g, l) from its own and is +0.0 in every other row.  Every entry of dJ is written.  With a NULL
 *                         inner jac pass NULL for the outer jac: the solver then takes forward differences over the n
 *                         OUTER unknowns, (n + 1) G inner evaluations per Jacobian where a structured difference would
 *                         need (N + 1) G -- correct, but wasteful at large G.
 * Nothing is computed: values are copied, so the bits are the inner launchers'.  Both return NLH_INVALID_INPUT_ERROR when M
 * is not a multiple of G or n != S + G L, NLH_UNDEFINED_FUNCTION_ERROR for a Jacobian call without an inner jac, and
 * otherwise what the inner launcher returns.  They do not synchronise.
 * Scratch belongs to the context, exactly as a map's: one buffer per stream, grown on demand, kept until
 * nlh_group_unwrap, at most 1 GiB per call; a call that needs more runs in slices of outer points -- the same bits.
 * NLH_GROUP_SCRATCH = bytes lowers the cap, NLH_GROUP_FORM = row | flat forces a workgroup form of the scatter for the sizes it
 * can hold (flat: m <= 256), NLH_GROUP_SPLIT = number of column groups overrides its column split (environment, read at each
 * call; tests).  The scatter moves 8 G m N bytes in and 8 G m (S + G L) out per outer point; it is store-bound and at large G
 * mostly writes zeros, which is what a dense solver costs. */
typedef struct nlh_group_ctx nlh_group_ctx;
int  nlh_group_wrap(nlh_handle *h, const nlh_group *g, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx,
                    nlh_group_ctx **out);
void nlh_group_unwrap(nlh_group_ctx *c);
int  nlh_group_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t M, double *dF);
int  nlh_group_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t M, double *dJ);
/* The batch steps on the DEVICE (the handle's stream; copies, no arithmetic):
 *   gather  dfull [ngroup G][N] -> dx [ngroup][n]; a shared parameter takes the value of the group's data set 0
 *   expand  dx [ngroup][n] -> dfull [ngroup G][N]
 *   sigma   dsigma [ngroup][n] -> dsigma_full [ngroup G][N]; NaN for every data set of a group whose dfail [ngroup] entry is
 *           non-zero (dfail may be NULL) */
int  nlh_group_gather_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dfull, double *dx);
int  nlh_group_expand_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dx, double *dfull);
int  nlh_group_sigma_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dsigma, const int32_t *dfail,
                           double *dsigma_full);
/* One-call global fits: the arguments of nlh_curve_fit_batch / nlh_expr_fit_batch plus, after xu, the group, a loss
 * (loss, dscale [nprob] per DATA SET or one shared; NLH_LOSS_LINEAR: none, dscale not read) and a statistic (stat: 0 least
 * squares, 1 Poisson deviance with mu_floor, dw then the 0 / 1 mask; the loss must then be NLH_LOSS_LINEAR).  They take no
 * parameter map: a map inside a group works through the launchers by hand.  nprob counts DATA SETS and must be a multiple
 * of G; ngroup = nprob / G.  The composition is fixed: the loss (or the Poisson pair) wraps the model's launchers per data
 * set, the group wraps the result.  The caller sees per-data-set arrays:
 *   dx [nprob][N] in and out: on entry a shared parameter starts from the value of the group's data set 0; on exit it is
 *   equal across the group.  dfvec [nprob][m], dsigma [nprob][N] (a shared parameter's sigma repeated per data set).
 *   xl, xu: HOST [N] or NULL, expanded to the n outer unknowns.
 * and per GROUP: dcov [ngroup][n][n] in the outer order (nlh_group_index locates entries), dchi2, drank, ib, status [ngroup].
 * Every rule of the unsuffixed entry point that names m or n holds with M = G m and n = S + G L: M >= n, M > n for errors, and
 * the zero-weight degrees of freedom, counted over the group's G m rows (a group is refused on its own count alone: a data
 * set whose rows all weigh 0 does not refuse its group, but its local columns are then zero and drank reports the
 * shortfall).  Errors, in this order:
 * NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a model that is refused, nprob < 0, m < 1, a NULL group, a group of another
 * parameter count, nprob not a multiple of G); NLH_UNDERDEFINED_PROBLEM_ERROR (M < n); NLH_INVALID_INPUT_ERROR (a loss
 * outside 0 .. 3, a stat outside 0 .. 1, Poisson with a loss); then, unless nprob = 0, NLH_INVALID_INPUT_ERROR for a NULL
 * array, errors asked for with M <= n, a bad mu_floor; the _h forms check scales, masks and counts as the _loss and _pois
 * entry points do. */
int nlh_curve_fit_batch_group(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                              int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                              const double *xl, const double *xu, const nlh_group *g, int32_t loss, const double *dscale,
                              int32_t shared_scale, int32_t stat, double mu_floor, double *dx, double *dfvec, double *dsigma,
                              double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_group_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                                int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                                const double *xl, const double *xu, const nlh_group *g, int32_t loss, const double *scale,
                                int32_t shared_scale, int32_t stat, double mu_floor, double *x, double *fvec, double *sigma,
                                double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_group(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                             int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                             const double *xu, const nlh_group *g, int32_t loss, const double *dscale, int32_t shared_scale,
                             int32_t stat, double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov,
                             double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_group_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                               int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                               const double *xu, const nlh_group *g, int32_t loss, const double *scale, int32_t shared_scale,
                               int32_t stat, double mu_floor, double *x, double *fvec, double *sigma, double *cov,
                               double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status);
/* A device-function MODEL of the outer unknowns of a group over a launcher-backed inner model (device-function, curve,
 * formula, loss, Poisson or mapped; a dense-quadratic model: NLH_INVALID_INPUT_ERROR), which must outlive it: nprob / G
 * problems of G m rows and n unknowns.  The same contract as nlh_pmap_model_create.  Errors: NLH_ERR_BAD_HANDLE, then
 * NLH_INVALID_INPUT_ERROR (a NULL argument, a dense-quadratic inner model, a group of another parameter count, an inner nprob
 * that is no multiple of G). */
int nlh_group_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_group *g, nlh_dq_model **model);

/* A device-function MODEL of a launcher-backed inner model (device-function, curve or formula, created WITHOUT weights; a
 * dense-quadratic model: NLH_INVALID_INPUT_ERROR) convolved with an instrument response; the inner model must outlive it.
 * cv->k, y, w (NULL: no weights): HOST arrays, [L] or [nprob][L], [nprob][m]; the model owns its device copies and its
 * wrapping context.  Every nlh_dq_model_* solver and nlh_dq_model_lm_covariance then takes it; a loss, Poisson, mapped or
 * global model may be made over it.  Errors: NLH_ERR_BAD_HANDLE, then NLH_INVALID_INPUT_ERROR (a NULL argument, a
 * dense-quadratic inner model, a bad L / origin / ext, a tap or a y that is not finite). */
int nlh_conv_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_conv *cv, const double *y, const double *w,
                          nlh_dq_model **model);
/* One-call fits with an instrument response: the arguments of the _group entry points plus, after the group, a parameter map
 * and the transform.  g may be NULL (no group), pm may be NULL (no map); both together: NLH_INVALID_INPUT_ERROR.  cv is
 * required; its k is a DEVICE pointer here and a HOST pointer in the _h forms, which stage it with the other arrays.  The
 * composition is fixed: the convolving pair wraps the model's launchers FIRST, the model bound without weights and dw
 * becoming the convolving pair's weights; the loss or the Poisson pair wraps the result -- under the Poisson pair the
 * convolving pair gets no weights and the Poisson pair keeps dw as its 0 / 1 mask (masked rows are +0.0) --; the map or the
 * group goes outside.  dfvec is the residual of the convolved model; everything else is what the _group (with a group), the
 * _pmap, _loss or _pois entry point of the same arguments returns.  Errors, in this order: the _group entry point's (without
 * its refusal of a NULL group; through its "unless nprob = 0" step); then NLH_INVALID_INPUT_ERROR for a NULL cv or cv->k, L
 * outside 1 .. NLH_CONV_MAX_L, origin outside 0 .. L-1, ext outside 0 .. 1; the _h forms also refuse, with
 * NLH_INVALID_INPUT_ERROR, a tap that is not finite and a y that is not finite on ANY row, whatever its weight; then they
 * check scales, masks and counts as the _loss and _pois entry points do. */
int nlh_curve_fit_batch_conv(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                             int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                             const double *xl, const double *xu, const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv,
                             int32_t loss, const double *dscale, int32_t shared_scale, int32_t stat, double mu_floor, double *dx,
                             double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                             nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_conv_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                               int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                               const double *xl, const double *xu, const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv,
                               int32_t loss, const double *scale, int32_t shared_scale, int32_t stat, double mu_floor, double *x,
                               double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                               nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_conv(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                            const double *xu, const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss,
                            const double *dscale, int32_t shared_scale, int32_t stat, double mu_floor, double *dx, double *dfvec,
                            double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                            int32_t *status);
int nlh_expr_fit_batch_conv_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                              const double *xu, const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss,
                              const double *scale, int32_t shared_scale, int32_t stat, double mu_floor, double *x, double *fvec,
                              double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib,
                              int32_t *status);

/* ---- separable fits (no counterpart in nonlin v2.2.0): variable projection for ANY device model.  Most fit models are linear
 * in many of their parameters -- a curve kind in its amplitudes and baseline coefficients, a formula like vmax*s/(km+s) in one
 * or two.  Variable projection (Golub & Pereyra; Kaufman's Jacobian) solves for those exactly at every trial point, so the
 * solver iterates over the nonlinear ones only and the caller gives no starting values for the linear ones.  Like a parameter
 * map it is a pair of wrapping launchers around any inner launcher pair, so everything that takes launchers works through it.
 * "Linear" is the caller's declaration: the inner model must be affine in those parameters at fixed nonlinear ones.
 * The nonlinear unknowns are the other full parameters in ascending full index: n = N - L.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  Per point, alpha the n
 * nonlinear values handed in:
 *   basis     p0 = (c = +0.0, alpha);  the inner jac at p0: its L linear columns are Phi (m x L);  the inner fcn at p0: f0
 *             (residuals are model - y here, so the residual at (c, alpha) is Phi c + f0)
 *   sum       EVERY sum over rows below has one order: 256 partials; partial j starts at +0.0 and takes the rows i = j (mod
 *             256) in ascending i as s = s + a*b; the partials combine as a 256-thread block sum does: inside each run of 64
 *             the tree  p[l] = p[l] + p[l + off], l < off, for off = 32, 16, 8, 4, 2, 1;  then t = +0.0 and t = t + (the
 *             result of run w) for w = 0, 1, 2, 3
 *   QR        unpivoted Householder on [Phi | f0].  norm0_l = sqrt(sum over all rows of w_i*w_i) of column l before any
 *             reflector.  Column l = 0 .. L-1 in turn, w its current values, r = the live columns so far:
 *               sigma = sum_{i>r} w_i*w_i;  norm = sqrt(w_r*w_r + sigma)
 *               DEAD when norm <= 2^-40 * norm0_l: the column is skipped, makes no reflector and gets c_l = +0.0
 *               else beta = -copysign(norm, w_r);  v_i = w_i / (w_r - beta) for i > r;  tau = (beta - w_r) / beta;  R_rr = beta;
 *               the reflector is applied to every later column of Phi and to f0, and r becomes r + 1
 *   apply     a reflector (v, tau) at position r to a column x:  s = x_r + sum_{i>r} v_i*x_i;  s = tau*s;  x_r = x_r - s;
 *             x_i = x_i - s*v_i for i > r.  R_rk is x_r of column k after the reflector at position r
 *   solve     z_j = -(Q^T f0)_j, the entry of f0 at column j's position.  j descending over the live columns:  s = z_j;  then
 *             s = s - R_jk*c_k for the live k > j in ascending k;  c_j = s / R_jj.  rank = the live columns
 *   fcn       p^ = (c, alpha); the inner fcn at p^ straight into the caller's dF: the residual the solver sees is, bit for
 *             bit, the inner model's residual at the full parameters nlh_sep_solve_batch returns
 *   jac       basis, QR and solve as above; the inner jac at p^; each of its n nonlinear columns d is projected,
 *             d - Q1 Q1^T d, as: the live reflectors in order; the leading rank entries to +0.0; the live reflectors in
 *             reverse order.  This is Kaufman's approximation; its J^T r is the exact gradient, because r is orthogonal to
 *             span Phi.
 * A point's bits do not depend on the launch shape, the slice, the batch or the workgroup form. ---- */
#define NLH_SEP_MAX_L 32
typedef struct nlh_sep nlh_sep;
/* The object (host code, needs no GPU).  lin [nlin]: the full indices of the linear parameters, ascending.  Refused with
 * NLH_INVALID_INPUT_ERROR, *sp left NULL: nlin < 1 or > NLH_SEP_MAX_L; no nonlinear parameter left (nfull - nlin < 1);
 * nfull > NLH_PMAP_MAX_N; a NULL lin; an index out of range, repeated or not ascending. */
int  nlh_sep_create(int32_t nfull, int32_t nlin, const int32_t *lin, nlh_sep **sp);
void nlh_sep_destroy(nlh_sep *sp);
void nlh_sep_shape(const nlh_sep *sp, int32_t *nfull, int32_t *nlin, int32_t *nnonlin);      /* any output may be NULL */
/* Read-back, for restatements (either output may be NULL): lin [nlin], nonlin [nfull - nlin] = the full index of each
 * nonlinear unknown. */
int  nlh_sep_tables(const nlh_sep *sp, int32_t *lin, int32_t *nonlin);
/* The wrapping launchers.  nlh_sep_wrap makes their context on the handle's device: a copy of the tables, scratch, the inner
 * pair (fcn, jac, inner_ctx; all stay the caller's and must outlive the context).  The inner jac is REQUIRED -- its linear
 * columns are the basis --: a NULL fcn or jac is NLH_UNDEFINED_FUNCTION_ERROR (after NLH_ERR_BAD_HANDLE for a NULL handle and
 * NLH_INVALID_INPUT_ERROR for a NULL sp or out).  The outer Jacobian may still be left to forward differences: pass a NULL
 * jacfcn to the solver.
 *   nlh_sep_device_fcn  three inner calls (jac and fcn at p0, fcn at p^) and the QR-and-solve kernel
 *   nlh_sep_device_jac  three inner calls (jac and fcn at p0, jac at p^), the QR-and-solve kernel and the projection kernel
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n != N - L or m < N returns non-zero before any launch.  An inner error comes back as it is,
 * with no further launch; by then only the context's own scratch has been written, nothing of the caller's.
 * Scratch belongs to the context: one buffer per stream, grown on demand, reused, kept until nlh_sep_unwrap, at most 1 GiB
 * per call and so per stream.  A call that needs more runs in slices of points -- the same bits.  NLH_SEP_SCRATCH = bytes
 * (environment, read at each call; tests) lowers the cap.
 * One workgroup of 256 threads works on a point, in one of two forms with the same bits: lds -- the panel [Phi | f0], and then
 * the reflectors and the columns of D (32 per workgroup at most), live in LDS, while m (L + 1 + n) doubles fit a workgroup's
 * LDS --, global -- the panel stays in the context's scratch and is re-read through the cache.  NLH_SEP_FORM = lds | global
 * (environment, read at each call; tests) forces one where it fits (lds is what runs where it fits). */
typedef struct nlh_sep_ctx nlh_sep_ctx;
int  nlh_sep_wrap(nlh_handle *h, const nlh_sep *sp, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, nlh_sep_ctx **out);
void nlh_sep_unwrap(nlh_sep_ctx *c);
int  nlh_sep_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_sep_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The two steps around a solve made through the launchers by hand, on DEVICE arrays (the handle's stream):
 *   gather   dfull [nprob][N] -> dx [nprob][n], the nonlinear values
 *   solve    dalpha [nprob][n] -> dfull [nprob][N] = (c(alpha), alpha), drank [nprob] (may be NULL) = the live columns; basis,
 *            QR and solve of the context's inner pair on problems 0 .. nprob-1 of m rows each (the context does not know m)
 * There is no covariance step: the covariance of a separable fit is the existing chain on the INNER pair at the full
 * solution, N x N with m - N degrees of freedom. */
int  nlh_sep_gather_batch(nlh_handle *h, const nlh_sep *sp, int32_t nprob, const double *dfull, double *dx);
int  nlh_sep_solve_batch(nlh_handle *h, nlh_sep_ctx *c, int32_t nprob, int32_t m, const double *dalpha, double *dfull, int32_t *drank);

/* A device-function MODEL of the n = N - L nonlinear unknowns over a launcher-backed inner model (device-function, curve,
 * formula, convolved; a dense-quadratic model: NLH_INVALID_INPUT_ERROR), which must outlive it; the model owns its projecting
 * context.  The same contract as nlh_pmap_model_create: every nlh_dq_model_* solver then takes it (x [nprob][n]);
 * nlh_dq_model_lm_covariance on it is the covariance of the PROJECTED problem -- for the errors of a separable fit call it on
 * the inner model at the full solution.  Errors: NLH_ERR_BAD_HANDLE, then NLH_INVALID_INPUT_ERROR (a NULL argument, a
 * dense-quadratic inner model, an sp whose N is not the inner model's n), NLH_UNDEFINED_FUNCTION_ERROR (an inner model
 * created without its analytic Jacobian). */
int  nlh_sep_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_sep *sp, nlh_dq_model **model);
/* One-call separable fits: nlh_curve_fit_batch / nlh_expr_fit_batch plus, after xu, a group (may be NULL), an instrument response (may be NULL; its k a
 * DEVICE pointer here, a HOST pointer in the _h forms) and the separable object (required).  They take no map, no loss and
 * no statistic: both are nonlinear in c and do not belong inside the projection.  The composition: the convolving pair, if
 * any, wraps the model's launchers first, the model bound without weights; the projecting pair wraps that; the group goes
 * outside: it is declared over the model's N parameters, its shared ones must all be nonlinear, and the solve runs through the
 * group of the same shared parameters over the n nonlinear ones (shared lifetimes, the amplitudes projected out per data set).
 * With a group dx, dfvec and dsigma stay per data set and dcov, dchi2, drank, ib, status are per group, and the errors are
 * what the _group entry point reports for the unprojected model at dx.
 * What the caller sees is FULL, exactly as from the _conv entry point: dx [nprob][N] -- on entry the linear positions are
 * ignored, on exit it is the full solution (c(alpha), alpha) of every problem that was solved (one that is refused on its
 * degrees of freedom keeps its x) --, dfvec the inner residual at dx, and dsigma, dcov, dchi2, drank what
 * nlh_lm_covariance_batch_device gives for the UNPROJECTED pair at dx: N x N, m - N degrees of freedom, the zero-weight rule
 * with N.  m >= N (NLH_UNDERDEFINED_PROBLEM_ERROR otherwise), m > N for errors.  analytic chooses the outer Jacobian --
 * Kaufman's projected one, or forward differences over the nonlinear unknowns -- and the Jacobian of the errors; the model's
 * analytic Jacobian is used for the basis either way.  xl / xu [N] (host): entries at linear positions must be infinite (or
 * the array NULL): a bound on a projected parameter cannot be honoured.  Errors, in this order: the _conv entry point's
 * (without its refusal of a NULL cv); then NLH_INVALID_INPUT_ERROR for a NULL sp, an sp of another N, a shared linear
 * parameter, a finite bound at a linear position. */
int nlh_curve_fit_batch_sep(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                            int32_t m, const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic,
                            const double *xl, const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp,
                            double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                            nlh_iteration_behavior *ib, int32_t *status);
int nlh_curve_fit_batch_sep_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob,
                              int32_t m, const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic,
                              const double *xl, const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp,
                              double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                              nlh_iteration_behavior *ib, int32_t *status);
int nlh_expr_fit_batch_sep(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                           int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                           const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *dx, double *dfvec,
                           double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                           int32_t *status);
int nlh_expr_fit_batch_sep_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                             int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                             const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *x, double *fvec,
                             double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib,
                             int32_t *status);

/* ---- per-kernel timing (HIP events on the handle's stream) ------------------ */
#define NLH_K_DQ_RESIDUAL   0
#define NLH_K_DQ_PANEL      1
#define NLH_K_FD_JACOBIAN   2
#define NLH_K_GRAM          3
#define NLH_K_GRAM_REDUCE   4
#define NLH_K_JTF           5
#define NLH_K_CHOL          6
#define NLH_K_LMPAR         7
#define NLH_K_QR            8
#define NLH_K_UPDATE        9
#define NLH_K_LU           10
#define NLH_K_DQ_JACOBIAN  11
#define NLH_K_QRX_PASS     12   /* exact lmfactor: trailing pass of a Householder step (nlh_qrx.hip) */
#define NLH_K_QRX_PIVOT    13   /* exact lmfactor: pivot + reflector of a step */
#define NLH_K_POLYROOTS    14   /* polynomial%roots: the one kernel of a nlh_poly_roots_batch call (nlh_polyroots.hip) */
#define NLH_K_COVAR       15   /* covar: the launches of one nlh_covar call, one bracket (nlh_covar.hip) */
#define NLH_K_COUNT        16
/* on: 0 = off, 1 = every kernel group, otherwise a mask with bit (k + 1) set for each group NLH_K_<k> to time
   (two HIP event records per timed launch on the handle's stream). */
void nlh_timing_enable(nlh_handle *h, int32_t on);
void nlh_timing_reset(nlh_handle *h);
/* Synchronises the stream, then returns total milliseconds and launch count. */
int  nlh_timing_get(nlh_handle *h, int32_t kernel_id, double *total_ms, int64_t *launches);
/* Per-launch durations (ms, launch order) of ONE kernel group since the last nlh_timing_reset.  The first call with a
 * new kernel_id selects that group and returns 0; later calls copy up to cap samples and return how many there are. */
int64_t nlh_timing_samples(nlh_handle *h, int32_t kernel_id, float *out_ms, int64_t cap);
const char *nlh_kernel_name(int32_t kernel_id);

#ifdef __cplusplus
}
#endif

/* ---- starting values for the built-in curve models: x0 for the one-call curve fits from the data alone, on the device.  The
 * entry points, their flags and their stated arithmetic are in nonlin_hip_guess.h, a part of this ABI that this header
 * includes: whoever includes nonlin_hip.h has them. ---- */
#include "nonlin_hip_guess.h"

/* ---- starts: starting values for ANY device model from a box -- the cost of a residual launcher at the candidates of the box,
 * for every problem at once, and the best of them per problem.  The entry points and their stated arithmetic are in
 * nonlin_hip_starts.h, a part of this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_starts.h"

/* ---- bootstrap: confidence intervals of ANY fit from refits of resampled data -- the replicas of every data set, made on the
 * device by a counter-based generator, and the reduction of the refits' parameters to intervals.  The entry points and their
 * stated arithmetic are in nonlin_hip_boot.h, a part of this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_boot.h"

/* ---- bin-integrated fits: ANY device model integrated or averaged over the bins of a histogram or the pixels of an image -- a
 * pair of wrapping launchers that evaluate the inner model at the nodes of a quadrature rule and sum them per bin.  The entry
 * points and their stated arithmetic are in nonlin_hip_bin.h, a part of this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_bin.h"

/* ---- Poisson bootstrap: the bootstrap of a fit of COUNTS (stat = Poisson) -- parametric replicas y* ~ Poisson(mu) of the fitted
 * values, drawn on the device by inversion from the mode in stated arithmetic.  The entry points are in
 * nonlin_hip_boot_pois.h, a part of this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_boot_pois.h"

/* ---- profile-likelihood intervals: the third statement of a fit's uncertainty, beside sigma and the bootstrap -- a pair of
 * wrapping launchers that pins one parameter per wrapped problem at its own value on shared data, and the lock-step root
 * finder over the pinned refits of every end.  The entry points and their stated arithmetic are in nonlin_hip_profile.h, a
 * part of this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_profile.h"

/* ---- studentised and BCa intervals of the bootstrap: the two textbook corrections of the percentile interval -- the reduction
 * of the refits and their standard errors to the bootstrap-t interval, the delete-one jackknife weights, the acceleration and
 * the bias-corrected, accelerated levels.  The entry points and their stated arithmetic are in nonlin_hip_boot_ci.h, a part of
 * this ABI that this header includes in the same way. ---- */
#include "nonlin_hip_boot_ci.h"

#endif /* NONLIN_HIP_H */
