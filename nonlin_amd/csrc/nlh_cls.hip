// nlh_cls.hip -- constrained_least_squares_solver: cls_solve (src/nonlin_least_squares.f90:938-1176: bounded trust
// region, Coleman-Li scaling, dog-leg, projected backtracking) as a lock-step device state machine, for batches and -- one
// problem, the callbacks behind the host-callback launchers -- for a single solve.
#include "nlh_internal.h"
#include "nlh_kernels_broyden.h"
#include "nlh_kernels_cls.h"
#include "nlh_kernels_exact.h"

void nlh_cls_init_device(int lds_max) { broyden_kernel_attrs(lds_max); }


// constrained_least_squares_solver%solve for a batch of device-model problems: the lock-step state machine of
// nlh_kernels_cls.h.  A round takes every problem that wants a Jacobian through J (forward differences, fused into the
// panel kernel), the QR of J with the reflectors applied to f, the Gauss-Newton step, the gradient and the dog-leg (with
// J g and J p where the step needs them) to its trial point, evaluates F there and runs the ratio test; problems inside
// the projected backtracking get one more trial point evaluated.  One 8-byte read-back per round.
static int cls_lockstep(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl_in,
                        const double *xu_in, int32_t nprob, int32_t m, int32_t n, const ResidualSource &rs,
                        double *dx, double *dfvec, nlh_iteration_behavior *ib, int32_t *status)
{   // rs: the built-in dense-quadratic family, or a user's device vecfcn / jacobianfcn launchers (nlh_devfcn.hip)
    int rc;
    const size_t mn = (size_t)m * n, np = (size_t)nprob;
    if ((rc = ensure(h, h->J, sizeof(double) * mn * np))) return rc;
    if ((rc = ensure(h, h->W2, sizeof(double) * mn * np))) return rc;
    const size_t per = 5 * (size_t)m + 7 * (size_t)n + 2 * ((size_t)n + 1) + 8;
    if ((rc = ensure(h, h->qnV, sizeof(double) * (per * np + 2 * (size_t)n)))) return rc;
    if ((rc = ensure(h, h->state, sizeof(LmState) * np))) return rc;
    if ((rc = ensure(h, h->misc, sizeof(ClState) * np + 64))) return rc;
    if ((rc = ensure_pinned(h, sizeof(ClState) * np + 64 + sizeof(double) * 2 * (size_t)n))) return rc;
    double *dJ = (double *)h->J.p, *dW = (double *)h->W2.p, *q = (double *)h->qnV.p;
    double *dE = q; q += (size_t)m * np;                         // the QR's extra column, then u in its head
    double *dJv = q; q += (size_t)m * np;                        // J g, later J p
    double *dfnew = q; q += (size_t)m * np;
    double *vbuf = q; q += 2 * (size_t)m * np;
    double *dg = q; q += (size_t)n * np;
    double *dsc = q; q += (size_t)n * np;
    double *dpgn = q; q += (size_t)n * np;
    double *dpsd = q; q += (size_t)n * np;
    double *du = q; q += (size_t)n * np;
    double *dp = q; q += (size_t)n * np;
    double *dxnew = q; q += (size_t)n * np;
    double *wbuf = q; q += 2 * ((size_t)n + 1) * np;
    double *st2 = q; q += 8 * np;
    double *dxl = q, *dxu = q + n;
    LmState *st = (LmState *)h->state.p;
    int32_t *dcounts = (int32_t *)h->misc.p;
    ClState *cs = (ClState *)((char *)h->misc.p + 64);
    int32_t *hcounts = (int32_t *)h->pinned;
    ClState *hcs = (ClState *)((char *)h->pinned + 64);
    double *hb = (double *)((char *)h->pinned + 64 + sizeof(ClState) * np);
    hipStream_t s = h->stream;
    for (int i = 0; i < n; ++i) {                                // :999-1009
        hb[i] = xl_in ? xl_in[i] : -DBL_MAX;
        hb[n + i] = xu_in ? xu_in[i] : DBL_MAX;
    }
    HIPCHK(h, hipMemcpyAsync(dxl, hb, sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
    ClOpts co;
    co.ftol = o->ftol; co.xtol = o->xtol; co.gtol = o->gtol; co.delta0 = delta0; co.stepscale0 = stepscale0;
    co.max_evals = o->max_evals; co.pad = 0;
    const int pb = (nprob + 255) / 256;
    const bool echo = o->print_status && nprob == 1;
    const int bsn = std::min(1024, ((n + 63) / 64) * 64);

    hipLaunchKernelGGL(k_cls_reset, dim3(pb), dim3(256), 0, s, nprob, delta0, st, cs);
    hipLaunchKernelGGL(k_cls_limits, dim3((n + 255) / 256, nprob), dim3(256), 0, s, n, (const double *)dxl, (const double *)dxu, dx);   // :1023
    if ((rc = residual_eval(h, rs, nprob, m, n, dx, dfvec, nullptr, st, CL_START))) return rc;
    hipLaunchKernelGGL(k_cls_start, dim3(nprob), dim3(256), 0, s, m, n, (const double *)dx, (const double *)dfvec, st, cs);
    int need_jac = nprob;                                        // upper bound until the first read-back
    // a round is an iteration or one backtracking trial: every one of them costs its problem an evaluation
    const long max_rounds = (long)o->max_evals + 16;
    for (long round = 0; round < max_rounds; ++round) {
        if (need_jac > 0) {
            // :1038 fcn%jacobian: forward differences (the built-in family: fused into the panel kernel) or the user's jacobianfcn
            // (after the first read-back need_jac is exact: a user's list is built without waiting for its length)
            if ((rc = residual_jacobian(h, rs, nprob, m, n, dx, dfvec, dJ, nullptr, st, CL_NEED_JAC, false, true, true, round > 0 ? need_jac : -1))) return rc;
            hipLaunchKernelGGL(k_cls_qr_prep, dim3((m + 255) / 256, nprob), dim3(256), 0, s, m, (const double *)dfvec, dE, (const LmState *)st);
            {
                dim3 grid((m + 31) / 32, (n + 31) / 32, nprob);
                hipLaunchKernelGGL(k_transpose, grid, dim3(256), 0, s, m, n, (const double *)dJ, dW, n, (const LmState *)st, (int)CL_NEED_JAC);
            }
            hipLaunchKernelGGL(k_qn_col0, dim3((m + 255) / 256, nprob), dim3(256), 0, s, m, n, (const double *)dW, vbuf);
            launch_house_steps(h, nprob, m, n, 1, dW, dE, vbuf, wbuf, st2, st, CL_NEED_JAC);
            hipLaunchKernelGGL(k_qn_solve_upper, dim3(nprob), dim3(bsn), sizeof(double) * n, s, n, (const double *)dW, dE, mn, (size_t)m,
                               (const LmState *)st, (int)CL_NEED_JAC);
            hipLaunchKernelGGL(k_qn_colsdot, dim3((n + 15) / 16, nprob), dim3(256), 0, s, m, n, (const double *)dJ, (const double *)dfvec, dg, 1.0,
                               (const LmState *)st, (int)CL_NEED_JAC);
            hipLaunchKernelGGL(k_cls_dog1, dim3(nprob), dim3(256), 0, s, m, n, (const double *)dx, (const double *)dxl, (const double *)dxu,
                               (const double *)dE, dsc, dpgn, dp, st, cs);
            hipLaunchKernelGGL(k_matvec_cm, dim3((m + 255) / 256, nprob), dim3(256), sizeof(double) * n, s, m, n, (const double *)dJ,
                               (const double *)dg, dJv, (const LmState *)st, (int)CL_DOG_SD);
            hipLaunchKernelGGL(k_cls_dog2, dim3(nprob), dim3(256), 0, s, m, n, (const double *)dx, (const double *)dxl, (const double *)dxu,
                               (const double *)dg, (const double *)dJv, (const double *)dsc, (const double *)dpgn, dpsd, du, dp, st, cs);
            hipLaunchKernelGGL(k_matvec_cm, dim3((m + 255) / 256, nprob), dim3(256), sizeof(double) * n, s, m, n, (const double *)dJ,
                               (const double *)dp, dJv, (const LmState *)st, (int)CL_PRED);
            hipLaunchKernelGGL(k_cls_pred, dim3(nprob), dim3(256), 0, s, m, n, (const double *)dx, (const double *)dg, (const double *)dp,
                               (const double *)dJv, (const double *)dsc, dxnew, st, cs);
            if ((rc = residual_eval(h, rs, nprob, m, n, dxnew, dfnew, nullptr, st, CL_TRIAL))) return rc;
            hipLaunchKernelGGL(k_cls_judge, dim3(nprob), dim3(256), 0, s, m, n, co, dx, dxnew, dfvec, (const double *)dfnew, (const double *)dg,
                               (const double *)dp, (const double *)dxl, (const double *)dxu, st, cs);
        }
        // (a problem that has just entered the backtracking gets its first point evaluated in the same round)
        if ((rc = residual_eval(h, rs, nprob, m, n, dxnew, dfnew, nullptr, st, CL_BT))) return rc;
        hipLaunchKernelGGL(k_cls_bt, dim3(nprob), dim3(256), 0, s, m, n, co, dx, dxnew, dfvec, (const double *)dfnew, (const double *)dp,
                           (const double *)dxl, (const double *)dxu, st, cs);
        hipLaunchKernelGGL(k_cls_count, dim3(1), dim3(256), 0, s, nprob, (const LmState *)st, dcounts);
        HIPCHK(h, hipMemcpyAsync(hcounts, dcounts, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (echo) HIPCHK(h, hipMemcpyAsync(hcs, cs, sizeof(ClState), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (echo && need_jac > 0 && hcs[0].print_due) print_status(hcs[0].pr_iter, hcs[0].pr_neval, hcs[0].pr_njac, hcs[0].pr_xnorm, hcs[0].pr_fnorm);
        need_jac = hcounts[0];
        if (need_jac == 0 && hcounts[1] == 0) break;
    }
    HIPCHK(h, hipMemcpyAsync(hcs, cs, sizeof(ClState) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (int p = 0; p < nprob; ++p) {
        const ClState &c = hcs[p];
        if (ib) {                                                // :1163-1170 (a non-finite start leaves them zero)
            memset(&ib[p], 0, sizeof ib[p]);
            if (!c.silent) {
                ib[p].iter_count = c.iter; ib[p].fcn_count = c.neval; ib[p].jacobian_count = c.njac;
                ib[p].converge_on_fcn = c.fcnvrg; ib[p].converge_on_chng = c.xcnvrg; ib[p].converge_on_zero_diff = c.gcnvrg;
            }
        }
        if (status) status[p] = (c.silent || c.converged) ? 0 : NLH_CONVERGENCE_ERROR;      // :1173-1175
    }
    return 0;
}

// The lock-step solver over a batch, in the slices its residual source holds.
static int cls_batch_rs(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl, const double *xu,
                        int32_t nprob, int32_t m, int32_t n, const ResidualSource &rs, double *dx, double *dfvec,
                        nlh_iteration_behavior *ib, int32_t *status)
{
    return residual_slices(rs, nprob, m, n, {dx, dfvec, nullptr, ib, status}, [&](int32_t cnt, const ResidualSource &r, const BatchIO &q) {
        return cls_lockstep(h, o, delta0, stepscale0, xl, xu, cnt, m, n, r, q.x, q.fvec, q.ib, q.status);
    });
}

int nlh_dq_cls_solve_batch(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl,
                           const double *xu, int32_t nprob, int32_t m, int32_t n, const double *dA, const double *db,
                           double gamma, double *dx, double *dfvec, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!o || n < 1 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (n > m) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    return cls_batch_rs(h, o, delta0, stepscale0, xl, xu, nprob, m, n, ResidualSource::dense_quadratic(dA, db, gamma), dx, dfvec, ib, status);
}

// constrained_least_squares_solver%solve (cls_solve, src/nonlin_least_squares.f90:938-1176) on a batch of problems whose
// residual is the USER'S device function (launchers, include/nonlin_hip.h): the lock-step state machine above.
int nlh_cls_solve_batch_device(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl, const double *xu,
                               int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *dx,
                               double *dfvec, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;              // :988
    if (nprob <= 0) return 0;
    if (!o || n < 1 || m < 1 || !dx || !dfvec) return NLH_INVALID_INPUT_ERROR;
    if (n > m) return NLH_UNDERDEFINED_PROBLEM_ERROR;           // :989
    HIPCHK(h, hipSetDevice(h->device));
    const nlh_options oq = silent_in_batch(*o, nprob);
    return cls_batch_rs(h, &oq, delta0, stepscale0, xl, xu, nprob, m, n, ResidualSource::launchers(fcn, jacfcn, ctx), dx, dfvec, ib, status);
}

int nlh_cls_solve_batch_device_h(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl, const double *xu,
                                 int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx, double *x,
                                 double *fvec, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob <= 0) return 0;
    if (!o || !x || !fvec || n < 1 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    const size_t xbytes = sizeof(double) * (size_t)nprob * n, fbytes = sizeof(double) * (size_t)nprob * m;
    return staged_call(h, {{x, xbytes, true, true, &h->xdev}, {fvec, fbytes, false, true, &h->fdev}},
                       [&](void *const *d) {
                           return nlh_cls_solve_batch_device(h, o, delta0, stepscale0, xl, xu, nprob, m, n, fcn, jacfcn, ctx, (double *)d[0],
                                                             (double *)d[1], ib, status);
                       });
}

// constrained_least_squares_solver%solve -- cls_solve, src/nonlin_least_squares.f90:938-1176 -- with the user's HOST vecfcn /
// jacobianfcn: the lock-step driver on one problem, the callbacks behind the host-callback launchers.
int nlh_cls_solve(nlh_handle *h, const nlh_options *o, double delta0, double stepscale0, const double *xl,
                  const double *xu, int32_t m, int32_t n, nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx, double *x,
                  double *fvec, nlh_iteration_behavior *ib)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib) memset(ib, 0, sizeof *ib);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;              // :988
    if (!o || n < 1 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (n > m) return NLH_UNDERDEFINED_PROBLEM_ERROR;           // :989
    HostCallbacks cb = HostCallbacks::vector(h, fcn, jacfcn, ctx);
    int32_t status = 0;
    const int rc = staged_call(h, {{x, sizeof(double) * (size_t)n, true, true, &h->xdev}, {fvec, sizeof(double) * (size_t)m, false, true, &h->fdev}},
                               [&](void *const *d) {
                                   return cls_lockstep(h, o, delta0, stepscale0, xl, xu, 1, m, n, cb.source(), (double *)d[0], (double *)d[1], ib, &status);
                               });
    return rc ? rc : status;
}
