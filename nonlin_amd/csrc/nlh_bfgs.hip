// nlh_bfgs.hip -- bfgs (bfgs_solve, src/nonlin_optimize.f90:557-770) with ls_search_miso
// (src/nonlin_linesearch.f90:329-492) and fcnnvar_helper%gradient (src/nonlin_multi_var.f90:182-246): a lock-step device
// state machine, for batches and -- one problem, the callbacks behind the host-callback launchers -- for a single solve; the Cholesky rank-one update / downdate as an entry point.
#include "nlh_internal.h"
#include "nlh_kernels_broyden.h"
#include "nlh_kernels_newton.h"
#include "nlh_kernels_bfgs.h"
#include "nlh_kernels_bfgs_batch.h"

// R = chol(B) (:724): the one place that chooses a form.  The blocked kernel, with as many thread groups per column as
// 1024 threads allow, wherever its LDS fits (lds_fits: n <= 608); beyond, the column form, which has the same bits by
// construction (k_bf_chol_factor<4> with 1024 threads serves any n <= 4096).  G > 0: blocked with G groups; -NC: the
// column form with NC columns per thread.
static int bf_chol_form(int n)
{
    const int CT = ((n + 63) / 64) * 64;
    const int G = CT * 4 <= 1024 ? 4 : CT * 2 <= 1024 ? 2 : 1;
    const void *blocked = G == 4 ? (const void *)k_bf_chol_blocked<4> : G == 2 ? (const void *)k_bf_chol_blocked<2> : (const void *)k_bf_chol_blocked<1>;
    if (n <= 1024 && lds_fits(blocked, bf_chol_lds(n))) return G;
    return qn_nc8(n) ? -8 : -4;
}

static void launch_bf_chol(hipStream_t s, int nprob, int n, const double *dB, double *dR, int *dinfo, const LmState *st, int want)
{
    const int CT = ((n + 63) / 64) * 64;
    switch (bf_chol_form(n)) {
    case 4: hipLaunchKernelGGL(k_bf_chol_blocked<4>, dim3(nprob), dim3(CT * 4), bf_chol_lds(n), s, n, dB, dR, dinfo, st, want); break;
    case 2: hipLaunchKernelGGL(k_bf_chol_blocked<2>, dim3(nprob), dim3(CT * 2), bf_chol_lds(n), s, n, dB, dR, dinfo, st, want); break;
    case 1: hipLaunchKernelGGL(k_bf_chol_blocked<1>, dim3(nprob), dim3(CT), bf_chol_lds(n), s, n, dB, dR, dinfo, st, want); break;
    case -8: hipLaunchKernelGGL(k_bf_chol_factor<8>, dim3(nprob), dim3(1024), sizeof(double) * n, s, n, dB, dR, dinfo, st, want); break;
    default: hipLaunchKernelGGL(k_bf_chol_factor<4>, dim3(nprob), dim3(1024), sizeof(double) * n, s, n, dB, dR, dinfo, st, want); break;
    }
}

void nlh_bfgs_init_device(int lds_max)
{
    hipFuncSetAttribute((const void *)k_bf_solve_upper_t, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_blocked<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_blocked<2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_blocked<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_update<1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_update<4>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_chol_update<8>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    hipFuncSetAttribute((const void *)k_bf_downdate_apply, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    broyden_kernel_attrs(lds_max);
}



// fcnnvar_helper%gradient -- fnh_grad_fcn, src/nonlin_multi_var.f90:182-246: the user's gradient routine when there is
// one, otherwise forward differences with h_j = sqrt(eps) |x_j| (sqrt(eps) at x_j = 0), one evaluation per variable in
// ascending order on the calling thread, true division.  The work is n + 1 calls of a host function: nothing here for
// the device; it lives behind the C ABI for the Fortran shim's fcnnvar_helper%gradient.
int nlh_fd_gradient(int32_t n, nlh_fcnnvar fcn, nlh_gradfcn gradfcn, void *ctx, double *x, const double *fv, double *g)
{
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (n < 1 || !x || !g) return NLH_INVALID_INPUT_ERROR;
    if (gradfcn) { gradfcn(ctx, n, x, g); return 0; }
    const double f0 = fv ? *fv : fcn(ctx, n, x);
    for (int j = 0; j < n; ++j) {
        const double xj = x[j];
        double step = NLH_SQRT_EPS * fabs(xj);
        if (step == 0.0) step = NLH_SQRT_EPS;
        x[j] = xj + step;
        const double fj = fcn(ctx, n, x);
        x[j] = xj;
        g[j] = (fj - f0) / step;
    }
    return 0;
}

// Device model: minimise f(x) = 0.5 * sum_i r_i(x)^2 of the dense-quadratic residual with bfgs; the
// forward-difference gradient (fnh_grad_fcn) is the residual panel kernel + k_bf_fd_gradient.
// bfgs%solve for a batch of device-model problems (objective 0.5 ||F(x)||^2, forward-difference gradient): the lock-step
// state machine of nlh_kernels_bfgs_batch.h.  A round takes every problem that wants a gradient through the residual
// panel and the differences, the tests and the secant pair, the update of the Cholesky factor (rank-one update +
// downdate, or a refactorisation) and the two triangular solves for the direction to the first trial point of its line
// search; every problem with a trial point gets F evaluated there and one turn of the search.  One 8-byte read-back
// per round.
// rs: the dense-quadratic family (objective 0.5 ||F(x)||^2), or -- scalar -- a USER'S fcnnvar handed in as a launcher with
// m = 1 (include/nonlin_hip.h: nlh_bfgs_solve_batch_device): F(x) is the objective itself, the forward-difference gradient
// is the 1 x n Jacobian of residual_jacobian (the same differences, src/nonlin_multi_var.f90:182-246), rs.jac the user's gradient.
static int bfgs_lockstep(nlh_handle *h, const nlh_options *o, int32_t nprob, int32_t m, int32_t n, const ResidualSource &rs, bool scalar,
                         double *dx, double *hfout, nlh_iteration_behavior *ib, int32_t *status)
{
    int rc;
    if (n > QN_MAX_N) return NLH_ARRAY_SIZE_ERROR;
    if (scalar != rs.user() || (scalar && m != 1)) return NLH_INVALID_INPUT_ERROR;
    const size_t mn = (size_t)m * n, nn = (size_t)n * n, np = (size_t)nprob;
    if (!scalar && (rc = ensure(h, h->P, sizeof(double) * mn * np))) return rc;
    if ((rc = ensure(h, h->bfB, sizeof(double) * nn * np))) return rc;
    if ((rc = ensure(h, h->bfR, sizeof(double) * nn * np))) return rc;
    if ((rc = ensure(h, h->bfV, sizeof(double) * ((size_t)m + 10 * (size_t)n + 1) * np + sizeof(int32_t) * np + 64))) return rc;
    if ((rc = ensure(h, h->state, sizeof(LmState) * np))) return rc;
    if ((rc = ensure(h, h->misc, sizeof(BfState) * np + 64))) return rc;
    if ((rc = ensure_pinned(h, sizeof(BfState) * np + 64))) return rc;
    double *dP = (double *)h->P.p, *dB = (double *)h->bfB.p, *dR = (double *)h->bfR.p, *q = (double *)h->bfV.p;
    double *dfv = q; q += (size_t)m * np;                        // F at the point evaluated last
    double *dg = q; q += (size_t)n * np;
    double *dgold = q; q += (size_t)n * np;
    double *ddx = q; q += (size_t)n * np;                        // the direction, then the step taken
    double *dy = q; q += (size_t)n * np;
    double *dbdx = q; q += (size_t)n * np;
    double *du = q; q += (size_t)n * np;
    double *dv = q; q += (size_t)n * np;
    double *dc = q; q += (size_t)n * np;
    double *dw = q; q += (size_t)n * np;
    double *dxnew = q; q += (size_t)n * np;
    double *df0 = q; q += np;                                    // (scalar: the objective at x, contiguous)
    int32_t *dinfo = (int32_t *)q;
    LmState *st = (LmState *)h->state.p;
    int32_t *dcounts = (int32_t *)h->misc.p;
    BfState *bs = (BfState *)((char *)h->misc.p + 64);
    int32_t *hcounts = (int32_t *)h->pinned;
    BfState *hbs = (BfState *)((char *)h->pinned + 64);
    hipStream_t s = h->stream;
    BfOpts bo;
    bo.xtol = o->xtol; bo.gtol = o->gtol; bo.ls_alpha = o->ls_alpha; bo.ls_factor = o->ls_factor;
    bo.max_evals = o->max_evals; bo.ls_max_evals = o->ls_max_evals; bo.use_line_search = o->use_line_search ? 1 : 0;
    bo.rc_divergent = NLH_DIVERGENT_BEHAVIOR_ERROR; bo.rc_convergence = NLH_CONVERGENCE_ERROR; bo.rc_invalid_op = NLH_INVALID_OPERATION_ERROR;
    bo.pad0 = bo.pad1 = 0;
    const int pb = (nprob + 255) / 256;
    const bool echo = o->print_status && nprob == 1;
    const int bs1 = std::min(1024, ((n + 63) / 64) * 64);
    const size_t bstride = sizeof(BfState) / sizeof(double), istride = sizeof(BfState) / sizeof(int32_t);
    static_assert(sizeof(BfState) % sizeof(double) == 0, "BfState is read through strided double / int pointers");
    const double *fp_all = &bs[0].fp, *temp_all = &bs[0].temp;
    const int32_t *iter_all = &bs[0].iter;
    const LmState *cst = st;

    hipLaunchKernelGGL(k_bfl_reset, dim3(pb), dim3(256), 0, s, nprob, st, bs, dinfo);
    if ((rc = residual_eval(h, rs, nprob, m, n, dx, dfv, nullptr, st, BF_START))) return rc;      // :633
    hipLaunchKernelGGL(k_bfl_start, dim3(nprob), dim3(256), 0, s, m, (const double *)dfv, st, bs, scalar ? 1 : 0);
    int need_grad = nprob;                                       // upper bound until the first read-back
    int last_printed_iter = 0;
    // a round costs every live problem an evaluation at least (a trial point, or an iteration's first one)
    const long max_rounds = (long)o->max_evals + (long)o->ls_max_evals + 16;
    for (long round = 0; round < max_rounds; ++round) {
        if (need_grad > 0) {
            // fnh_grad_fcn: n perturbed evaluations, (f_j - f) / h_j (src/nonlin_multi_var.f90:182-246)
            if (scalar) {
                hipLaunchKernelGGL(k_bfl_gather_fp, dim3(pb), dim3(256), 0, s, nprob, (const BfState *)bs, df0);
                // (after the first read-back need_grad is exact: the list is built without waiting for its length)
                if ((rc = residual_jacobian(h, rs, nprob, 1, n, dx, df0, dg, nullptr, st, BF_GRAD, false, false, true, round > 0 ? need_grad : -1))) return rc;
            } else {
                launch_dq_panel(h, nprob, m, n, rs.dA, rs.db, rs.gamma, dx, dP, st, BF_GRAD);
                hipLaunchKernelGGL(k_bf_fd_gradient, dim3(n, nprob), dim3(64), 0, s, m, n, (const double *)dP, (const double *)dx, 0.0, dg,
                                   fp_all, bstride, cst, (int)BF_GRAD);
            }
            hipLaunchKernelGGL(k_bfl_after_grad, dim3(nprob), dim3(256), 0, s, n, bo, (const double *)dx, (const double *)dg, (const double *)dgold,
                               ddx, dy, dxnew, st, bs);
            // :703-712: R = temp I in the first iteration, B = R^T R, B dx
            hipLaunchKernelGGL(k_bf_scaled_identity, dim3((unsigned)((nn + 255) / 256), nprob), dim3(256), 0, s, n, 0.0, dR, temp_all, bstride,
                               iter_all, istride, cst, (int)BF_UPD_A);
            hipLaunchKernelGGL(k_bf_rtr, dim3((n + 255) / 256, n, nprob), dim3(256), 0, s, n, (const double *)dR, dB, cst, (int)BF_UPD_A);
            hipLaunchKernelGGL(k_matvec_cm, dim3((n + 255) / 256, nprob), dim3(256), sizeof(double) * n, s, n, n, (const double *)dB,
                               (const double *)ddx, dbdx, cst, (int)BF_UPD_A);
            hipLaunchKernelGGL(k_bfl_split, dim3(nprob), dim3(256), 0, s, n, (const double *)ddx, (const double *)dbdx, (const double *)dy, du, dv, st, bs);
            // :716-722: R^T R += u u^T, then -= v v^T
            if (n <= 1024) hipLaunchKernelGGL(k_bf_chol_update<1>, dim3(nprob), dim3(bs1), sizeof(double) * 2 * n, s, n, dR, (const double *)du, cst, (int)BF_UPD_RANK);
            else if (qn_nc8(n)) hipLaunchKernelGGL(k_bf_chol_update<8>, dim3(nprob), dim3(1024), sizeof(double) * 2 * n, s, n, dR, (const double *)du, cst, (int)BF_UPD_RANK);
                else hipLaunchKernelGGL(k_bf_chol_update<4>, dim3(nprob), dim3(1024), sizeof(double) * 2 * n, s, n, dR, (const double *)du, cst, (int)BF_UPD_RANK);
            hipLaunchKernelGGL(k_bf_solve_upper_t, dim3(nprob), dim3(bs1), sizeof(double) * n, s, n, (const double *)dR, dv, cst, (int)BF_UPD_RANK);
            hipLaunchKernelGGL(k_bf_downdate_rot, dim3(nprob), dim3(64), 0, s, n, dv, dc, dinfo, cst, (int)BF_UPD_RANK);
            hipLaunchKernelGGL(k_bf_downdate_apply, dim3((n + 255) / 256, nprob), dim3(256), sizeof(double) * 2 * n, s, n, dR, (const double *)dc,
                               (const double *)dv, (const int *)dinfo, cst, (int)BF_UPD_RANK);
            hipLaunchKernelGGL(k_nt_advance, dim3(pb), dim3(256), 0, s, nprob, st, (int)BF_UPD_RANK, (int)BF_DIR);
            // :724: R = chol(B)
            launch_bf_chol(s, nprob, n, (const double *)dB, dR, dinfo, cst, (int)BF_UPD_FACTOR);
            hipLaunchKernelGGL(k_nt_advance, dim3(pb), dim3(256), 0, s, nprob, st, (int)BF_UPD_FACTOR, (int)BF_DIR);
            // :727: dx = -(R^T R)^-1 g
            hipLaunchKernelGGL(k_bfl_neg, dim3((n + 255) / 256, nprob), dim3(256), 0, s, n, (const double *)dg, dw, cst);
            hipLaunchKernelGGL(k_bf_solve_upper_t, dim3(nprob), dim3(bs1), sizeof(double) * n, s, n, (const double *)dR, dw, cst, (int)BF_DIR);
            hipLaunchKernelGGL(k_qn_solve_upper, dim3(nprob), dim3(bs1), sizeof(double) * n, s, n, (const double *)dR, dw, nn, (size_t)n, cst, (int)BF_DIR);
            hipLaunchKernelGGL(k_bfl_dir_done, dim3(nprob), dim3(256), 0, s, n, bo, (const double *)dx, (const double *)dg, ddx, (const double *)dw,
                               dxnew, (const int32_t *)dinfo, st, bs);
        }
        if ((rc = residual_eval(h, rs, nprob, m, n, dxnew, dfv, nullptr, st, BF_TRIAL))) return rc;
        hipLaunchKernelGGL(k_bfl_trial, dim3(nprob), dim3(256), 0, s, m, n, bo, dx, dxnew, ddx, (const double *)dg, dgold, (const double *)dfv, st, bs,
                           scalar ? 1 : 0);
        hipLaunchKernelGGL(k_bfl_count, dim3(1), dim3(256), 0, s, nprob, cst, dcounts);
        HIPCHK(h, hipMemcpyAsync(hcounts, dcounts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (echo) HIPCHK(h, hipMemcpyAsync(hbs, bs, sizeof(BfState), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        // (print_due stays set once an iteration has been printed: the round that ends the solve on a convergence test
        // comes back with the block of the iteration before)
        if (echo && need_grad > 0 && hbs[0].print_due && hbs[0].pr_iter != last_printed_iter) {         // :730-737
            last_printed_iter = hbs[0].pr_iter;
            printf(" \n");
            printf("Iteration: %d\n", hbs[0].pr_iter);
            printf("Function Evaluations: %d\n", hbs[0].pr_neval);
            char e1[16], e2[16], e3[16];
            format_e10_3(hbs[0].pr_fp, e1); format_e10_3(hbs[0].pr_xtest, e2); format_e10_3(hbs[0].pr_gtest, e3);
            printf("Function Value: %s\nChange in Variable: %s\nGradient: %s\n", e1, e2, e3);
        }
        need_grad = hcounts[0];
        if (need_grad == 0 && hcounts[1] == 0) break;
    }
    HIPCHK(h, hipMemcpyAsync(hbs, bs, sizeof(BfState) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (int p = 0; p < nprob; ++p) {
        const BfState &c = hbs[p];
        if (ib) {                                                // :751-759
            ib[p].iter_count = c.iter; ib[p].fcn_count = c.neval; ib[p].jacobian_count = 0; ib[p].gradient_count = c.ngrad;
            ib[p].converge_on_fcn = 0; ib[p].converge_on_chng = c.xcnvrg; ib[p].converge_on_zero_diff = c.gcnvrg;
        }
        const bool finished = c.rc || c.flag || c.xcnvrg || c.gcnvrg;
        if (status) status[p] = c.rc ? c.rc : ((c.flag || !finished) ? NLH_CONVERGENCE_ERROR : 0);   // :765-767
        if (hfout) hfout[p] = c.fp;                              // :762
    }
    return 0;
}

// The lock-step solver over a batch, in the slices its residual source holds (a user's objective is a scalar: m = 1).
static int bfgs_batch_rs(nlh_handle *h, const nlh_options *o, int32_t nprob, int32_t m, int32_t n, const ResidualSource &rs, double *dx,
                         double *hfout, nlh_iteration_behavior *ib, int32_t *status)
{
    return residual_slices(rs, nprob, m, n, {dx, nullptr, hfout, ib, status}, [&](int32_t cnt, const ResidualSource &r, const BatchIO &q) {
        return bfgs_lockstep(h, o, cnt, m, n, r, rs.user(), q.x, q.fout, q.ib, q.status);
    });
}

int nlh_dq_bfgs_solve_batch(nlh_handle *h, const nlh_options *o, int32_t nprob, int32_t m, int32_t n, const double *dA,
                            const double *db, double gamma, double *dx, double *hfout, nlh_iteration_behavior *ib,
                            int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!o || n < 1 || m < 1) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    return bfgs_batch_rs(h, o, nprob, m, n, ResidualSource::dense_quadratic(dA, db, gamma), dx, hfout, ib, status);
}

// bfgs%solve on a batch of problems whose objective is the USER'S device fcnnvar: a launcher of the nlh_device_vecfcn type
// with m = 1 (dF[npoints] = f at each point); gradfcn (optional, nlh_device_jacfcn with m = 1: dJ[npoints][n] = the
// gradients) replaces the forward differences as fcnnvar_helper%gradient does (src/nonlin_multi_var.f90:213-217).
int nlh_bfgs_solve_batch_device(nlh_handle *h, const nlh_options *o, int32_t nprob, int32_t n, nlh_device_vecfcn fcn,
                                nlh_device_jacfcn gradfcn, void *ctx, double *dx, double *hfout, nlh_iteration_behavior *ib,
                                int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;              // src/nonlin_optimize.f90:611-615
    if (!o || n < 1 || (nprob > 0 && !dx)) return NLH_INVALID_INPUT_ERROR;
    if (nprob <= 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    const nlh_options oq = silent_in_batch(*o, nprob);
    return bfgs_batch_rs(h, &oq, nprob, 1, n, ResidualSource::launchers(fcn, gradfcn, ctx), dx, hfout, ib, status);
}

// bfgs%solve -- bfgs_solve, src/nonlin_optimize.f90:557-770 -- with the user's HOST fcnnvar / gradientfcn: the lock-step
// driver on one problem, the callbacks behind the host-callback launchers (the scalar pair: m = 1).
int nlh_bfgs_solve(nlh_handle *h, const nlh_options *o, int32_t n, nlh_fcnnvar fcn, nlh_gradfcn gradfcn, void *ctx,
                   double *x, double *fout, nlh_iteration_behavior *ib)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib) memset(ib, 0, sizeof *ib);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;              // :614
    if (!o || n < 1) return NLH_INVALID_INPUT_ERROR;
    HostCallbacks cb = HostCallbacks::scalar(h, fcn, gradfcn, ctx);
    int32_t status = 0;
    const int rc = staged_call(h, {{x, sizeof(double) * (size_t)n, true, true, &h->xdev}}, [&](void *const *d) {
        return bfgs_lockstep(h, o, 1, 1, n, cb.source(), true, (double *)d[0], fout, ib, &status);
    });
    return rc ? rc : status;
}

// The same behind a host array.
int nlh_bfgs_solve_batch_device_h(nlh_handle *h, const nlh_options *o, int32_t nprob, int32_t n, nlh_device_vecfcn fcn,
                                  nlh_device_jacfcn gradfcn, void *ctx, double *x, double *fout, nlh_iteration_behavior *ib,
                                  int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob <= 0) return 0;
    if (!x || !o || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    return staged_call(h, {{x, sizeof(double) * (size_t)nprob * n, true, true, &h->xdev}}, [&](void *const *d) {
        return nlh_bfgs_solve_batch_device(h, o, nprob, n, fcn, gradfcn, ctx, (double *)d[0], fout, ib, status);
    });
}

// cholesky_rank1_update / cholesky_rank1_downdate stand-ins (call sites src/nonlin_optimize.f90:721-722): in place on the
// row-major upper factor dRt (n x n); du is consumed.  *hinfo = 1 if the downdate would lose positive definiteness.
int nlh_chol_rank1(nlh_handle *h, int32_t n, int32_t downdate, double *dRt, double *du, int32_t *hinfo)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (n < 1) return NLH_INVALID_INPUT_ERROR;
    if (n > QN_MAX_N) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->bfV, sizeof(double) * ((size_t)6 * n + 8)))) return rc;
    double *dc = (double *)h->bfV.p;
    int *dinfo = (int *)(dc + n);
    hipStream_t s = h->stream;
    const int bs1 = std::min(1024, ((n + 63) / 64) * 64);
    int info = 0;
    if (!downdate) {
        if (n <= 1024) hipLaunchKernelGGL(k_bf_chol_update<1>, dim3(1), dim3(bs1), sizeof(double) * 2 * n, s, n, dRt, du, (const LmState *)nullptr, -1);
        else if (qn_nc8(n)) hipLaunchKernelGGL(k_bf_chol_update<8>, dim3(1), dim3(1024), sizeof(double) * 2 * n, s, n, dRt, du, (const LmState *)nullptr, -1);
                else hipLaunchKernelGGL(k_bf_chol_update<4>, dim3(1), dim3(1024), sizeof(double) * 2 * n, s, n, dRt, du, (const LmState *)nullptr, -1);
    } else {
        hipLaunchKernelGGL(k_bf_solve_upper_t, dim3(1), dim3(bs1), sizeof(double) * n, s, n, dRt, du, (const LmState *)nullptr, -1);
        hipLaunchKernelGGL(k_bf_downdate_rot, dim3(1), dim3(64), 0, s, n, du, dc, dinfo, (const LmState *)nullptr, -1);
        hipLaunchKernelGGL(k_bf_downdate_apply, dim3((n + 255) / 256), dim3(256), sizeof(double) * 2 * n, s, n, dRt, dc, du, dinfo, (const LmState *)nullptr, -1);
        HIPCHK(h, hipMemcpyAsync(&info, dinfo, sizeof(int), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (hinfo) *hinfo = info;
    HIPCHK(h, hipGetLastError());
    return 0;
}

// cholesky_factor(b, .true.) stand-in (call site src/nonlin_optimize.f90:724) through launch_bf_chol, the dispatch of the
// solver, every problem taking part: dB [nprob][n][n] symmetric, dRt the row-major upper factors, hinfo [nprob] (host).
int nlh_bf_chol_factor(nlh_handle *h, int32_t nprob, int32_t n, const double *dB, double *dRt, int32_t *hinfo)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 1 || n < 1 || !dB || !dRt || !hinfo) return NLH_INVALID_INPUT_ERROR;
    if (n > QN_MAX_N || nprob > NLH_MAX_LOCKSTEP) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->bfV, sizeof(int32_t) * (size_t)nprob))) return rc;
    int *dinfo = (int *)h->bfV.p;
    hipStream_t s = h->stream;
    launch_bf_chol(s, nprob, n, dB, dRt, dinfo, nullptr, -1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(hinfo, dinfo, sizeof(int32_t) * (size_t)nprob, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The form launch_bf_chol takes for n (0: no form, n out of range).
int32_t nlh_bf_chol_form(int32_t n)
{
    if (n < 1 || n > QN_MAX_N) return 0;
    return bf_chol_form(n);
}

// solve_cholesky(.true., r, x) stand-in (call site :727): x <- R^-T x, then x <- R^-1 x, the solver's two launches.
int nlh_bf_solve_cholesky(nlh_handle *h, int32_t nprob, int32_t n, const double *dRt, double *dx)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 1 || n < 1 || !dRt || !dx) return NLH_INVALID_INPUT_ERROR;
    if (n > QN_MAX_N || nprob > NLH_MAX_LOCKSTEP) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int bs1 = std::min(1024, ((n + 63) / 64) * 64);
    hipLaunchKernelGGL(k_bf_solve_upper_t, dim3(nprob), dim3(bs1), sizeof(double) * n, s, n, dRt, dx, (const LmState *)nullptr, -1);
    hipLaunchKernelGGL(k_qn_solve_upper, dim3(nprob), dim3(bs1), sizeof(double) * n, s, n, dRt, dx, (size_t)n * n, (size_t)n, (const LmState *)nullptr, -1);
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    return 0;
}
