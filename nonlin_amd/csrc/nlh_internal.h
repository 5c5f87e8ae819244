// nlh_internal.h -- what the translation units of libnonlin_hip.so share: the handle, the error macro, the event
// brackets of a kernel group, and the helpers one unit defines for the others (nlh_core.hip unless noted).
// Units:
//   nlh_core.hip       handle, options, timing, generator, residual / FD launches, worker handles
//   nlh_lm.hip         least_squares_solver: lss_solve and its stages
//   nlh_square.hip     newton_solver, quasi_newton_solver, LU, the Householder steps
//   nlh_cls.hip        constrained_least_squares_solver
//   nlh_bfgs.hip       bfgs, fcnnvar_helper%gradient
//   nlh_nm.hip         nelder_mead
//   nlh_1var.hip       brent_solver, newton_1var_solver, fcn1var_helper%diff
//   nlh_poly.hip       polynomial%fit
//   nlh_polyroots.hip  polynomial%roots, batched evaluate
//   nlh_covar.hip      parameter covariance
//   nlh_band.hip       confidence and prediction bands: the covariance propagated through any launcher pair
//   nlh_devfcn.hip     user device residuals: the open launcher path, the built-in family as launchers
//   nlh_curve.hip      built-in curve models: launchers, values, the eight nlh_curve_fit_batch* entry points
//   nlh_expr.hip       formula models: compiler, launchers, values, the eight nlh_expr_fit_batch* entry points
//   nlh_fit.hip        the fit + errors pipeline behind those sixteen (nlh_fit_run below)
//   nlh_pmap.hip       parameter maps: the map object, the wrapping launchers, gather / expand / covariance
//   nlh_loss.hip       robust losses: the wrapping launchers, apply, the upload of host scales
//   nlh_pois.hip       Poisson likelihood fits: the wrapping launchers, apply, the check of host counts and masks
//   nlh_conv.hip       instrument-response fits: the wrapping launchers, apply, the check of a transform
//   nlh_group.hip      global fits: the group object, the wrapping launchers, gather / expand / sigma
//   nlh_sep.hip        separable fits: the object, the wrapping launchers (variable projection), gather / solve
//   nlh_guess.hip      starting values for the curve models: the nonlinear stage's kernels, then nlh_sep_solve_batch
//   nlh_starts.hip     starts: the candidates of a box, the batched scan over any residual launcher, cost / pick / take
//   nlh_boot.hip       bootstrap: the generator's draws, the resampling kernels, the summary of the refits
//   nlh_bin.hip        bin-integrated fits: the Gauss-Legendre rules, the wrapping launchers, apply
//   nlh_pin.hip        the pin pair: the wrapping launchers that hold one parameter per wrapped problem at its own value
//   nlh_profile.hip    profile-likelihood intervals: the start and the lock-step step of the root finder over all ends
//   nlh_model.hip      device sets, device residual models behind host arrays
//   nlh_qrx.hip        the exact lmfactor
// Kernels live in the nlh_kernels_*.h headers with internal linkage: a unit compiles the ones it launches.  nlh_launch.h:
// the host side of the (point, row) kernels' two workgroup forms and what the six pairs of wrapping launchers share.
#pragma once
#include "../../include/nonlin_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <atomic>
#include <string>
#include <vector>

#include "nlh_common.h"
#include "nlh_lm_head.h"


// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct nlh_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    uint32_t timing = 0;              // bit k: kernel group k is bracketed by HIP events
    struct Pair { hipEvent_t a, b; int kid; };
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    double ms[NLH_K_COUNT] = {0};
    int64_t launches[NLH_K_COUNT] = {0};
    int sample_kid = -1;              // kernel group whose per-launch durations are kept (nlh_timing_samples)
    std::vector<float> samples;
    std::vector<DevBuf *> bufs;       // every workspace buffer, for destroy
    // named workspace buffers (grown on demand, reused across calls)
    DevBuf J, P, wa4, scratch, G, Gpart, vecs, ipvt, gvec, part, state, info, misc, lu, xdev, fdev, Adev, bdev, W2, R,
           qnQ, qnR, qnV, bfB, bfR, bfV, qxV, lumv, lus,
           P2,                            // second copy of the exact factorisation's working matrix (lazy: qrx_second_matrix)
           dvX, dvF, dvIdx, dvP,          // user device residuals: points, compact residuals, problem lists, panel chunk (nlh_devfcn.hip)
           cvW, cvT, cvH,                 // covariance (nlh_covar.hip): the chain's arrays, the global-memory window, host-array staging
           crv,                           // one-call fits (nlh_fit.hip): status, non-zero-weight counts, a covariance nobody asked to keep
           sepx,                          // one-call separable fits (nlh_fit.hip): the nonlinear unknowns and, of a group, the outer ones
           bdW, bdH,                      // bands (nlh_band.hip): the chain's Jacobian and values, host-array staging
           guessA, guessP, guessH,        // starting values (nlh_guess.hip): alpha / span / flags, the decays' panel, host-array staging
           startsC, startsX, startsF, startsS, startsH,   // starts (nlh_starts.hip): the candidate table, a chunk's points and problems, its
                                          // residuals, its costs, host-array staging
           bootV,                         // bootstrap (nlh_boot.hip): which replicas of which problems are valid
           profW;                         // profile intervals (nlh_profile.hip): the residuals at the fit, the box, the count of running ends
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    DevBuf cholmc;                     // side buffer of the multi-CU Cholesky (solved panels, bad-pivot flags)
    void *staging = nullptr;           // pinned staging of a device-set share's rows of the caller's host arrays
    size_t staging_bytes = 0;
    void *cbstage = nullptr;           // pinned staging of the host-callback launchers (HostCallbacks): a call's points and results
    size_t cbstage_bytes = 0;
    bool cb_failed = false;            // a host-callback launcher failed on its own account: err holds the text, its code is the library's
    bool qrx_open_on = false; hipEvent_t qrx_a{}, qrx_b{}; int qrx_kid = 0;   // open bracket of a nlh_qrx.hip launch
    std::vector<nlh_handle *> workers;   // private handles (own stream + workspace) for the sub-batches of a dealt LM batch
    hipStream_t lu_side = nullptr;       // the blocked LU's look-ahead: the bulk of a step's update runs here, under the next panel
    hipEvent_t lu_panel_done = nullptr, lu_bulk_done[2] = {nullptr, nullptr};
};

#define HIPCHK(h, call)                                                                 \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return NLH_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)


int ensure(nlh_handle *h, DevBuf &b, size_t bytes);              // grow-on-demand device workspace, registered for destroy
// The dynamic LDS nlh_create allows every single-workgroup kernel (hipFuncAttributeMaxDynamicSharedMemorySize).
static const int NLH_LDS_MAX = 160 * 1024 - 2048;
// Does a launch of `kernel` with `dyn` bytes of dynamic LDS fit NLH_LDS_MAX, the kernel's static LDS included?  Asked
// before every launch whose dynamic LDS grows with n: a launch the runtime refuses would leave its problems where they are.
bool lds_fits(const void *kernel, size_t dyn);
int ensure_staging(nlh_handle *h, size_t bytes);
int ensure_pinned(nlh_handle *h, size_t bytes);
void timing_flush(nlh_handle *h);
hipEvent_t ev_get(nlh_handle *h);

struct Timed {
    nlh_handle *h; int kid; hipEvent_t a{}, b{}; bool on;
    Timed(nlh_handle *h_, int kid_) : h(h_), kid(kid_), on((h_->timing >> kid_) & 1u)
    {
        if (on) { a = ev_get(h); b = ev_get(h); hipEventRecord(a, h->stream); }
    }
    ~Timed()
    {
        if (on) {
            hipEventRecord(b, h->stream);
            h->pending.push_back({a, b, kid});
            if (h->pending.size() > 65536) timing_flush(h);
        }
    }
};
int ensure_workers(nlh_handle *h, int T);

// per-unit kernel attributes (dynamic LDS limits), called by nlh_create on the handle's device
void nlh_lm_init_device(int lds_max);
void nlh_square_init_device(int lds_max);

// launches of the residual family (nlh_core.hip)
void launch_dq_residual(nlh_handle *h, int nprob, int m, int n, const double *A, const double *b, double gamma, const double *x,
                        double *f, double *part, const LmState *st, int want);
void launch_dq_panel(nlh_handle *h, int nprob, int m, int n, const double *A, const double *b, double gamma, const double *x,
                     double *P, const LmState *st, int want, const double *f0_fused = nullptr, bool to_qrx = false);
void launch_fd(nlh_handle *h, int nprob, int m, int n, const double *P, const double *f0, const double *x, double *J,
               const LmState *st, int want);
// ---------------------------------------------------------------------------
// The shell of a batch entry point around its lock-step driver (nlh_core.hip): slices, host staging, a silent batch.
// ---------------------------------------------------------------------------
// Several kernels of the lock-step drivers carry the problem index in gridDim.y / .z (at most 65535): a larger batch is
// solved in slices of NLH_MAX_LOCKSTEP problems, one after the other (independent problems: the same bits).
static const int32_t NLH_MAX_LOCKSTEP = 65535;
// The one slice loop: run(first, count) on consecutive runs of at most `slice` problems until one returns non-zero (a
// 64-bit counter: first + slice may pass INT32_MAX).  A template, not a std::function: launch_dq_residual comes here once
// per solver iteration, and its closure would not fit a std::function's own storage.
template <class Run> static inline int lockstep_slices(int32_t nprob, int32_t slice, Run &&run)
{
    for (int64_t p0 = 0; p0 < nprob; p0 += slice) {
        const int rc = run((int32_t)p0, (int32_t)std::min<int64_t>(slice, nprob - p0));
        if (rc) return rc;
    }
    return 0;
}
template <class Run> static inline int lockstep_slices(int32_t nprob, Run &&run) { return lockstep_slices(nprob, NLH_MAX_LOCKSTEP, run); }
// Slice lengths of a user's launcher (the lock-step ones also hold NLH_MAX_LOCKSTEP).
// One Jacobian call asks the launcher for count * n points at once, and its panel is addressed with 31-bit point counts.
static inline int32_t slice_points(int32_t n)
{
    return (int32_t)std::max<int64_t>(1, std::min<int64_t>(NLH_MAX_LOCKSTEP, ((int64_t)1 << 30) / n));
}
// A covariance or FD-Jacobian call keeps the whole panel: count * n points of max(m, n) doubles inside 31 bits.
static inline int32_t slice_panel(int32_t m, int32_t n)
{
    return (int32_t)std::max<size_t>(1, std::min<size_t>((size_t)NLH_MAX_LOCKSTEP, ((size_t)1 << 30) / ((size_t)n * std::max(m, n))));
}
// Nelder-Mead's staging list holds count * (n + 1) points whose offsets are int32.
static inline int32_t slice_simplex(int32_t n) { return (int32_t)std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)n + 1)); }
// A scalar root has at most two points per problem in flight, and the point offsets are int32.
static inline int32_t slice_root1v() { return 1 << 28; }

// Which residual a lock-step driver evaluates (nlh_devfcn.hip): the built-in dense-quadratic family (dA, db, gamma), or a
// user's launchers (include/nonlin_hip.h: nlh_device_vecfcn / nlh_device_jacfcn).  pbase: index, in the caller's batch,
// of the first problem of the range the driver works on (slices, sub-batches) -- what the user's dprob entries count from.
struct ResidualSource {
    const double *dA = nullptr, *db = nullptr;
    double gamma = 0.0;
    nlh_device_vecfcn fcn = nullptr;
    nlh_device_jacfcn jac = nullptr;
    void *ctx = nullptr;
    int32_t pbase = 0;
    static ResidualSource dense_quadratic(const double *dA, const double *db, double gamma)
    {
        ResidualSource r;
        r.dA = dA; r.db = db; r.gamma = gamma;
        return r;
    }
    static ResidualSource launchers(nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *ctx)
    {
        ResidualSource r;
        r.fcn = fcn; r.jac = jac; r.ctx = ctx;
        return r;
    }
    bool user() const { return fcn != nullptr; }
    int32_t slice(int32_t n) const { return user() ? slice_points(n) : NLH_MAX_LOCKSTEP; }   // problems of one lock-step run
    ResidualSource shifted(int32_t p0, int m, int n) const
    {
        ResidualSource r = *this;
        if (user()) r.pbase += p0;
        else { r.dA += (size_t)p0 * m * n; r.db += (size_t)p0 * m; }
        return r;
    }
};
// What a lock-step driver reads and writes per problem: x [n] and fvec [m] on the device, fout, ib and status on the host;
// any but x may be NULL.  at(p0): the same arrays from problem p0 on.
struct BatchIO {
    double *x, *fvec, *fout;
    nlh_iteration_behavior *ib;
    int32_t *status;
    BatchIO at(int32_t p0, int m, int n) const
    {
        return {x + (size_t)p0 * n, fvec ? fvec + (size_t)p0 * m : nullptr, fout ? fout + p0 : nullptr, ib ? ib + p0 : nullptr,
                status ? status + p0 : nullptr};
    }
};
// A batch through a lock-step driver in slices of rs.slice(n): run(count, the slice's residual source, the slice's arrays).
int residual_slices(const ResidualSource &rs, int32_t nprob, int m, int n, const BatchIO &io,
                    const std::function<int(int32_t, const ResidualSource &, const BatchIO &)> &run);
// The host-array twin of a device-pointer entry point: each host array gets a device copy in a buffer of the handle (in:
// uploaded before the call), call(dev) runs the device form on dev[k], the copy of array k, and, when it returns 0, the out
// arrays are downloaded and the stream is synchronised once.  A non-zero return of call copies nothing back.
struct HostArray { void *host; size_t bytes; bool in, out; DevBuf *buf; };
int staged_call(nlh_handle *h, std::initializer_list<HostArray> arrays, const std::function<int(void *const *)> &call);
// A batch stays silent: the status block is a single solve's (the reference prints between the iterations of ONE solve), and a
// slice, a sub-batch or a share of a dealt batch may hold a single problem.
static inline nlh_options silent_in_batch(const nlh_options &o, int32_t nprob)
{
    nlh_options q = o;
    if (nprob > 1) q.print_status = 0;
    return q;
}
// h->err = "<what>: the user's <which> returned <rc>"; returns NLH_ERR_HIP (nlh_devfcn.hip)
int launcher_failed(nlh_handle *h, int rc, const char *what, const char *which = "launcher");
// F(x) for the problems at stage `want` (st == nullptr: every problem): x [nprob][n] -> f [nprob][m]; part (optional):
// the per-block partial sums of squares k_dq_residual leaves (the non-exact policies' norms).
int residual_eval(nlh_handle *h, const ResidualSource &rs, int nprob, int m, int n, const double *x, double *f, double *part,
                  const LmState *st, int want);
// vfh_jac_fcn for the problems at stage `want`: the n perturbed evaluations + jac(:,j) = (f_j - f0) / h_j (or the user's
// jacobianfcn when use_jac and one is set).  out: column-major [nprob][n][m], or -- to_qrx -- the exact factorisation's
// working matrix; panel: scratch of nprob * m * n doubles, distinct from out (the dense-quadratic family's unfused form
// only: a user's panel lives in a chunk buffer of the handle).  fuse: dense-quadratic family only.
int residual_jacobian(nlh_handle *h, const ResidualSource &rs, int nprob, int m, int n, const double *x, const double *f0,
                      double *out, double *panel, const LmState *st, int want, bool to_qrx, bool fuse, bool use_jac, int known_cnt = -1);

void launch_sumsq_part(nlh_handle *h, int nprob, int m, int n, const double *f, double *part);   // nlh_lm.hip

// A user's HOST callbacks as launchers (nlh_devfcn.hip): what lets a lock-step driver with nprob = 1 stand behind the
// single solves of the drop-in path (nlh_lm_solve, nlh_quasi_newton_solve, nlh_cls_solve, nlh_bfgs_solve,
// nlh_fd_jacobian).  A call copies the points to the host, synchronises the stream, calls the user's function once per point
// in ascending point order on the calling thread -- which must be the thread that made the context: a driver that dealt
// the problem to a worker is refused -- and uploads the results (left in flight: their readers are behind them on the
// stream).  A forward-difference Jacobian is n
// such points: the reference's n calls, in its order (src/nonlin_multi_eqn_mult_var.f90:267-273).  Either the vector pair
// (fcn, jac) or the scalar pair (sfcn, grad: fcnnvar / gradientfcn, the m = 1 case with a 1 x n Jacobian) is set.
struct HostCallbacks {
    nlh_handle *h;
    nlh_vecfcn fcn;
    nlh_jacfcn jac;
    nlh_fcnnvar sfcn;
    nlh_gradfcn grad;
    void *ctx;
    std::thread::id caller;
    // armed by residual_eval for one call: the one problem's stage comes down with the point, and the user's function is
    // called only if it is `want` (no separate read-back of the stage before the call)
    const int32_t *stage = nullptr;
    int32_t want = 0;
    static HostCallbacks vector(nlh_handle *h, nlh_vecfcn fcn, nlh_jacfcn jac, void *ctx)
    {
        return {h, fcn, jac, nullptr, nullptr, ctx, std::this_thread::get_id(), nullptr, 0};
    }
    static HostCallbacks scalar(nlh_handle *h, nlh_fcnnvar sfcn, nlh_gradfcn grad, void *ctx)
    {
        return {h, nullptr, nullptr, sfcn, grad, ctx, std::this_thread::get_id(), nullptr, 0};
    }
    // the residual source a driver takes: the Jacobian launcher only when the user gave a Jacobian / gradient
    ResidualSource source();
};
int host_callback_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int host_callback_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);

// nlh_square.hip
void launch_lu_factor(nlh_handle *h, int nprob, int n, double *dA, int32_t *dipvt, int32_t *dinfo, const LmState *st = nullptr,
                      int want = -1);
void launch_house_steps(nlh_handle *h, int nprob, int rows, int ncA, int ncE, double *dA, double *dE, double *vbuf, double *wbuf,
                        double *st, const LmState *gst = nullptr, int gwant = -1);


static const int RB = 256;   // rows per block of the residual kernels

// host-side scalar helpers of nlh_newton_solve's O(n) logic (the reference's operation order)

static inline double h_dot(int n, const double *a, const double *b)
{
    double s = 0.0;
    for (int i = 0; i < n; ++i) s = s + a[i] * b[i];
    return s;
}

// NORM2 as the flang runtime evaluates it (processor-dependent intrinsic); the host-side
// Newton logic uses it only for stpmax and limit_search_vector.
static inline double h_norm2(int n, const double *x)
{
    double mx = 0.0, s = 0.0;
    for (int i = 0; i < n; ++i) {
        const double a = fabs(x[i]);
        if (mx == 0.0) mx = a;
        else if (a > mx) { const double t = mx / a, tsq = t * t; s = s * tsq; s = s + tsq; mx = a; }
        else if (a != 0.0) { const double t = a / mx; s = s + t * t; }
    }
    return mx * sqrt(1.0 + s);
}

// min_backtrack_search, src/nonlin_linesearch.f90:495-551
static inline double min_backtrack_search(int mode, double f0, double f, double f1, double alam, double alam1, double slope)
{
    double lam;
    if (mode == 1) {
        lam = -slope / (2.0 * (f - f0 - slope));
    } else {
        const double rhs1 = f - f0 - alam * slope;
        const double rhs2 = f1 - f0 - alam1 * slope;
        const double a = (rhs1 / (alam * alam) - rhs2 / (alam1 * alam1)) / (alam - alam1);
        const double b = (-alam1 * rhs1 / (alam * alam) + alam * rhs2 / (alam1 * alam1)) / (alam - alam1);
        if (a == 0.0) {
            lam = -slope / (2.0 * b);
        } else {
            const double disc = b * b - 3.0 * a * slope;
            if (disc < 0.0) lam = 0.5 * alam;
            else if (b <= 0.0) lam = (-b + sqrt(disc)) / (3.0 * a);
            else lam = -slope / (b + sqrt(disc));
        }
        if (lam > 0.5 * alam) lam = 0.5 * alam;
    }
    return lam;
}
void format_e10_3(double v, char out[16]);
void nlh_bfgs_init_device(int lds_max);
// nlh_nm.hip: nelder_mead on a batch of the user's device fcnnvar behind host arrays x [nprob][n]
int nlh_nm_solve_batch_device_h(nlh_handle *h, const nlh_options *o, double init_size, int32_t nprob, int32_t n,
                                nlh_device_vecfcn fcn, void *ctx, double *x, double *fout, nlh_iteration_behavior *ib,
                                int32_t *status);
// nlh_1var.hip: brent_solver (newton = 0) / newton_1var_solver (1) on a batch of the user's device fcn1var behind host
// arrays lim [nprob][2], x [nprob]
int nlh_root1v_solve_batch_device_h(nlh_handle *h, const nlh_options *o, int newton, int32_t nprob, nlh_device_vecfcn fcn,
                                    nlh_device_jacfcn diff, void *ctx, const double *lim, double *x, double *fout,
                                    nlh_iteration_behavior *ib, int32_t *status);
void nlh_cls_init_device(int lds_max);
void nlh_poly_init_device(int lds_max);
void nlh_polyroots_init_device(int lds_max);    // nlh_polyroots.hip (polynomial%roots, batched evaluate)
void nlh_covar_init_device(int lds_max);        // nlh_covar.hip (covar, nlh_lm_covariance*)
void nlh_devfcn_init_device(int lds_max);        // nlh_devfcn.hip: the built-in family's launcher kernels keep x in LDS
void nlh_expr_init_device(int lds_max);          // nlh_expr.hip: the formula interpreter keeps its stacks in LDS
void nlh_sep_init_device(int lds_max);           // nlh_sep.hip: the separable fits' kernels keep a point's panel in LDS
void nlh_band_init_device(int lds_max);          // nlh_band.hip: the band kernel keeps a point's packed covariance in LDS
void nlh_guess_init_device(int lds_max);         // nlh_guess.hip: the guess kernels keep a problem's valid rows in LDS
void nlh_boot_init_device(int lds_max);          // nlh_boot.hip: the resampling kernels keep a problem's active residuals in LDS

// A compiled formula (nlh_expr.hip; include/nonlin_hip.h: nlh_expr_*).  ExprProg is what the kernels read, passed by value in
// the kernel arguments: code[i] = op | (arg & 0xff) << 8 | aroot << 16 | broot << 24, aroot the instruction that produced the
// operand a of a binary instruction (b's is i - 1, as is a unary instruction's operand); VOIGT, the one ternary instruction:
// aroot is x's producer, broot sigma's, gamma's is i - 1 (broot is 0 elsewhere); mask[i]: the parameters instruction i's
// subtree names.  LOAD k (a use of definition k, whose value stays in slot k): arg = k, aroot the instruction that produced
// the definition, mask that instruction's.  depth: the frame, the most slots in use, definitions included.  ndef (host side,
// nlh_expr): the definitions, so the slot the model value ends in; the launchers run the kernels' EXPR_DEFS instantiations when it
// is not 0, and ExprProg is what it was for the formulas without definitions.  sf2 (host side): the program holds an
// instruction of NLH_EXPR_J0 .. NLH_EXPR_LOG1P; the launchers then run the EXPR_SF2 instantiations, with definitions or none.
struct ExprProg {
    int32_t ninstr, nvar, nparams, depth;
    uint32_t code[NLH_EXPR_MAX_INSTR];
    uint32_t mask[NLH_EXPR_MAX_INSTR];
    double consts[NLH_EXPR_MAX_CONST];
};
struct nlh_expr {
    ExprProg prog;
    int32_t nconst, ndef, sf2;
};

// The one-call fit + errors of the twenty-eight entry points nlh_{curve,expr}_fit_batch{,_pmap,_loss,_pois,_group,_conv,_sep}{,_h} (nlh_fit.hip).
// FitSource: what a model kind hands the pipeline.  bind points the context's data at problem p0 of dt, dy, dw (the whole
// batch's device arrays) before each run of consecutive problems; whatever else the context holds stays the whole batch's.
struct FitSource {
    int32_t N;                         // parameters of the model; < 0: the model is refused
    size_t tdoubles;                   // doubles of t per abscissa: 1 for a curve, nvar for a formula
    const char *what;                  // the label of error texts: "curve fit"
    nlh_device_vecfcn fcn;
    nlh_device_jacfcn jac;             // NULL: forward differences
    void *ctx;
    void (*bind)(void *ctx, const double *dt, const double *dy, const double *dw, int32_t p0);
};
// FitArgs: the rest of an entry point's arguments, as the header documents them, for the device-pointer form and the
// host-array form alike.  A plain fit is pm = NULL, loss = NLH_LOSS_LINEAR (which reads no scale).  stat: what is minimised
// -- the sum of squares (the twelve least-squares entry points leave it and mu_floor at their defaults), or the Poisson
// deviance of the counts y, w then being the 0 / 1 mask of the rows.
enum { NLH_STAT_LSQ = 0, NLH_STAT_POISSON = 1 };
struct FitArgs {
    int32_t nprob, m;
    const double *t;
    int32_t shared_t;
    const double *y, *w, *xl, *xu;
    const nlh_pmap *pm;
    int32_t loss;
    const double *scale;
    int32_t shared_scale;
    double *x, *fvec, *sigma, *cov, *chi2;
    int32_t *rank;
    nlh_iteration_behavior *ib;
    int32_t *status;
    int32_t stat = NLH_STAT_LSQ;
    double mu_floor = 0.0;
    const nlh_group *grp = nullptr;    // a global fit: nprob data sets in groups; cov, chi2, rank, ib, status per group
    const nlh_conv *cv = nullptr;      // an instrument response: the model is convolved with it (k: as the other arrays, device or host)
    // a separable fit (the _sep entry points set want_sp; sp itself may then not be NULL): the linear parameters are projected
    // out; sp_jac: the model's Jacobian launcher, needed whatever `analytic` says (the source's jac follows analytic)
    bool want_sp = false;
    const nlh_sep *sp = nullptr;
    nlh_device_jacfcn sp_jac = nullptr;
};
// The documented ladder of checks, then: solve (bounded when xl or xu is given), covariance with scaled = 1 when any of sigma,
// cov, chi2 is asked for, the degrees-of-freedom rule of zero weights, NaN and rank -1 for problems that did not solve.  The
// loss wraps the model's launchers; the map, if any, wraps the result.  host: the arrays are host arrays (the scales too).
// NLH_STAT_POISSON: the model is bound without weights, the Poisson wrapper sits where the loss sits, the covariance is
// unscaled, and chi2 = deviance / dof with dof = unmasked rows - n.
int nlh_fit_run(nlh_handle *h, const nlh_options *opts, const FitSource &src, const FitArgs &a, bool host);
// A layer: the context of any of the six pairs of wrapping launchers by its base (nlh_launch.h: WrapCtx, which every nlh_*_ctx
// derives from alone, so the address is the same).  wrap_release is what every nlh_*_unwrap does once it has checked the
// kind: set the device, free the scratch, free the kind's tables, clear the magic, delete; NULL does nothing (nlh_pmap.hip).
struct WrapCtx;
static inline WrapCtx *wrap_layer(void *ctx) { return reinterpret_cast<WrapCtx *>(ctx); }
void wrap_release(WrapCtx *c);
// what the pipeline needs of a wrapping context besides the public nlh_*_wrap / _unwrap: where a run of problems starts in
// the caller's arrays (nlh_loss.hip, nlh_pmap.hip), and the map's three small launches on the context's copy of the tables
struct PmapTables;                     // nlh_kernels_pmap.h
void loss_ctx_rebind(nlh_loss_ctx *c, const double *dscale);
void pois_ctx_rebind(nlh_pois_ctx *c, const double *dy, const double *dw);
void pmap_ctx_rebind(nlh_pmap_ctx *c, const double *dfull);
const PmapTables *pmap_ctx_tables(const nlh_pmap_ctx *c);
void pmap_gather(const PmapTables *T, hipStream_t s, int nprob, const double *full, double *x);
void pmap_expand(const PmapTables *T, hipStream_t s, int nprob, const double *x, const double *full, int shared_full, double *p);
void pmap_cov(const PmapTables *T, hipStream_t s, int nprob, const double *cov, const double *sigma, const int32_t *fail, double *covf,
              double *sigf);
struct GroupTables;                    // nlh_kernels_group.h: the same of a group's context (nlh_group.hip)
const GroupTables *group_ctx_tables(const nlh_group_ctx *c);
void group_gather(const GroupTables *T, hipStream_t s, int ngroup, const double *full, double *x);
void group_expand(const GroupTables *T, hipStream_t s, int ngroup, const double *x, const int32_t *fail, double *p);
// Host arrays, one after the other, into ONE device allocation on the handle's device, the caller's to hipFree; synchronised.
// Errors name `what` in h->err: "hipMalloc (what)", "hipMemcpy (what): ...".  A part of 0 bytes is skipped.  (nlh_model.hip)
struct HostPart { const void *p; size_t bytes; };
int nlh_upload(nlh_handle *h, const char *what, std::initializer_list<HostPart> parts, void **base);
// robust losses (nlh_loss.hip): a kind of the header's table; HOST scales finite and positive, every one of cnt (LINEAR reads
// none); the same check and then a device copy of them, the caller's to hipFree (LINEAR: none, *dscale NULL)
bool nlh_loss_kind_ok(int32_t kind);
bool nlh_loss_scale_ok(int32_t kind, const double *scale, size_t cnt);
int nlh_loss_scale_upload(nlh_handle *h, int32_t kind, const double *scale, size_t cnt, double **dscale);
// Poisson fits (nlh_pois.hip): a floor finite and positive; a HOST mask (NULL: none) of 0.0 / 1.0, every one of cnt, and HOST
// counts finite and not negative on every row the mask keeps
bool nlh_pois_floor_ok(double mu_floor);
bool nlh_pois_data_ok(const double *y, const double *w, size_t cnt);
// instrument-response fits (nlh_conv.hip): a transform the header accepts (k not NULL, L, origin and ext in range); where a
// run of problems starts in the caller's arrays
bool nlh_conv_ok(const nlh_conv *cv);
// ... with HOST taps and HOST data of nprob problems of m rows: every tap and every y finite (every row is convolved)
bool nlh_conv_data_ok(const nlh_conv *cv, const double *y, size_t nprob, size_t m);
void conv_ctx_rebind(nlh_conv_ctx *c, const double *dy, const double *dw, const double *dk);
// columns the built-in dense-quadratic family's kernels accept (x in LDS, lds_max of nlh_create): beyond it NLH_ARRAY_SIZE_ERROR
static const int32_t NLH_DQ_MAX_N = 20000;

static inline int factor_threads(int n) { return n >= 96 ? 1024 : 256; }
void print_status(int iter, int nfeval, int njaceval, double xnorm, double fnorm);


static const int QN_MAX_N = 8192;      // k_qn_retri / k_bf_chol_*: 8 columns per thread at most (4 up to n = 4096)
// eight columns per thread: beyond 4096 columns -- or, NLH_QN_FORCE_NC8 (tests), wherever the four-column instance would run
static inline bool qn_nc8(int n)
{
    static const bool force = [] { const char *e = getenv("NLH_QN_FORCE_NC8"); return e && atoi(e) != 0; }();
    return n > 4096 || force;
}
static const int QN_LDS_ROWS = 18000;  // up to here k_qn_house_dot keeps the reflector (rows doubles) in LDS; beyond: in global memory
// nlh_house_steps / nlh_house_plan: what the grids of the Householder kernels hold (problems on y or z, 16-row groups of
// k_qn_house_apply on y: 65535 each) and a column count whose groups and products with nprob stay far inside int
static const int QN_HOUSE_MAX_NPROB = 65535, QN_HOUSE_MAX_ROWS = 65535 * 16, QN_HOUSE_MAX_NC = 1 << 20;
