// nlh_nm.hip -- nelder_mead (nm_solve, src/nonlin_optimize.f90:104-340, nm_extrapolate :343-399): the lock-step device
// state machine of nlh_kernels_nm.h for a batch of the user's device objectives, and the same machine with nprob = 1
// behind a host callback (the points of a round copied out, evaluated in list order, the values copied back).
#include "nlh_internal.h"
#include "nlh_kernels_nm.h"

// How a round's points are evaluated: npoints points x [npoints][n] of problems dprob, values to f [npoints] (DEVICE).
using NmEval = std::function<int(int32_t npoints, const int32_t *dprob, const double *x, double *f)>;

// nm_solve for nprob problems: dx [nprob][n] device (in: the start, out: vertex 1 on convergence, untouched otherwise),
// dsim [nprob][n+1][n] device (built from dx and init_size unless use_simplex; holds the final simplex).  echo: the status
// block after every iteration (a lone host-callback solve).  One 4-byte read-back per round.
static int nm_lockstep(nlh_handle *h, const nlh_options *o, double init_size, int32_t nprob, int32_t n, int32_t pbase,
                       const NmEval &eval, double *dx, double *dsim, bool use_simplex, bool echo, double *hfout,
                       nlh_iteration_behavior *ib, int32_t *status)
{
    int rc;
    const size_t np = (size_t)nprob, npts = (size_t)n + 1;
    // f [np][npts], pcent, work [np][n]; staging: points [np * npts][n], values [np * npts]
    if ((rc = ensure(h, h->qxV, sizeof(double) * (np * npts + 2 * np * n + np * npts * n + np * npts)))) return rc;
    if ((rc = ensure(h, h->state, sizeof(NmState) * np))) return rc;
    const size_t nb = (np + 1023) / 1024;                           // runs of the scan
    if ((rc = ensure(h, h->misc, sizeof(int32_t) * (np * npts + 2 * np + 2 * nb + 16)))) return rc;
    if ((rc = ensure_pinned(h, sizeof(NmState) * np + 64))) return rc;
    double *q = (double *)h->qxV.p;
    double *df = q; q += np * npts;
    double *dpc = q; q += np * n;
    double *dwork = q; q += np * n;
    double *dxs = q; q += np * npts * n;
    double *dfs = q;
    NmState *st = (NmState *)h->state.p;
    int32_t *dtotal = (int32_t *)h->misc.p;
    int32_t *dcnt = dtotal + 16, *doff = dcnt + np, *dbsum = doff + np, *dbpre = dbsum + nb, *dprob = dbpre + nb;
    int32_t *htotal = (int32_t *)h->pinned;
    NmState *hst = (NmState *)((char *)h->pinned + 64);
    hipStream_t s = h->stream;
    NmOpts no;
    no.ftol = o->gtol; no.init_size = init_size; no.max_evals = o->max_evals; no.build = use_simplex ? 0 : 1;
    const int pb = (nprob + 3) / 4;

    hipLaunchKernelGGL(k_nm_reset, dim3(pb), dim3(256), 0, s, nprob, n, no, (const double *)dx, dsim, st, dcnt);
    // every live problem evaluates at least one point per round and stops once neval >= max_evals: a bound, not a knob
    const long max_rounds = std::max<long>((long)o->max_evals, 0) + 8;
    for (long round = 0;; ++round) {
        if (round > 0)
            hipLaunchKernelGGL(k_nm_advance, dim3(pb), dim3(256), 0, s, nprob, n, no, (const double *)dfs, (const int32_t *)doff, dsim, df,
                               dpc, dwork, dx, st, dcnt);
        hipLaunchKernelGGL(k_nm_scan_blocks, dim3((unsigned)nb), dim3(1024), 0, s, nprob, (const int32_t *)dcnt, doff, dbsum);
        hipLaunchKernelGGL(k_nm_scan_top, dim3(1), dim3(1024), 0, s, (int)nb, (const int32_t *)dbsum, dbpre, dtotal);
        hipLaunchKernelGGL(k_nm_emit, dim3(pb), dim3(256), 0, s, nprob, n, pbase, (const double *)dsim, (const double *)dwork,
                           (const NmState *)st, (const int32_t *)dcnt, doff, (const int32_t *)dbpre, dxs, dprob);
        HIPCHK(h, hipMemcpyAsync(htotal, dtotal, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (echo) HIPCHK(h, hipMemcpyAsync(hst, st, sizeof(NmState), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (echo && round > 0 && hst[0].print_due) {               // :306-313
            char e1[16], e2[16];
            format_e10_3(hst[0].pr_fval, e1); format_e10_3(hst[0].pr_rtol, e2);
            printf(" \nIteration: %d\nFunction Evaluations: %d\nFunction Value: %s\nConvergence Parameter: %s\n",
                   hst[0].pr_iter, hst[0].pr_neval, e1, e2);
            fflush(stdout);
        }
        const int32_t total = *htotal;
        if (total == 0) break;
        if (round > max_rounds) { h->err = "nelder_mead: the round bound was exceeded"; return NLH_ERR_HIP; }
        if ((rc = eval(total, dprob, dxs, dfs))) return rc;
    }
    HIPCHK(h, hipMemcpyAsync(hst, st, sizeof(NmState) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (int32_t p = 0; p < nprob; ++p) {
        const NmState &c = hst[p];
        if (ib) {                                                    // :322-330
            ib[p].iter_count = c.iter; ib[p].fcn_count = c.neval; ib[p].jacobian_count = 0; ib[p].gradient_count = 0;
            ib[p].converge_on_fcn = c.fcnvrg; ib[p].converge_on_chng = 0; ib[p].converge_on_zero_diff = 0;
        }
        if (status) status[p] = c.flag ? NLH_CONVERGENCE_ERROR : 0;  // :335-337
        if (hfout) hfout[p] = c.fval;                                // :333: the stale f(1) after a flag exit
    }
    return 0;
}

int nlh_nelder_mead_solve(nlh_handle *h, const nlh_options *o, double init_size, int32_t n, nlh_fcnnvar fcn, void *ctx,
                          double *x, double *simplex, int32_t use_simplex, double *fout, nlh_iteration_behavior *ib)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib) memset(ib, 0, sizeof *ib);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;                  // :166-174
    if (!o || n < 1 || !x || (use_simplex && !simplex)) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    const size_t npts = (size_t)n + 1;
    if ((rc = ensure(h, h->xdev, sizeof(double) * ((size_t)n + npts * n)))) return rc;
    double *dx = (double *)h->xdev.p, *dsim = dx + n;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(dx, x, sizeof(double) * n, hipMemcpyHostToDevice, s));
    if (use_simplex) HIPCHK(h, hipMemcpyAsync(dsim, simplex, sizeof(double) * npts * n, hipMemcpyHostToDevice, s));
    std::vector<double> hx, hf;
    NmEval ev = [&](int32_t npoints, const int32_t *, const double *dxs, double *dfs) -> int {
        hx.resize((size_t)npoints * n);
        hf.resize((size_t)npoints);
        HIPCHK(h, hipMemcpyAsync(hx.data(), dxs, sizeof(double) * hx.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (int32_t k = 0; k < npoints; ++k) hf[k] = fcn(ctx, n, hx.data() + (size_t)k * n);
        HIPCHK(h, hipMemcpyAsync(dfs, hf.data(), sizeof(double) * hf.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipStreamSynchronize(s));                          // (hf is pageable and reused next round)
        return 0;
    };
    nlh_iteration_behavior lib;
    int32_t st = 0;
    double fo = 0.0;
    if ((rc = nm_lockstep(h, o, init_size, 1, n, 0, ev, dx, dsim, use_simplex != 0, o->print_status != 0, &fo, &lib, &st))) return rc;
    HIPCHK(h, hipMemcpyAsync(x, dx, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (simplex) HIPCHK(h, hipMemcpyAsync(simplex, dsim, sizeof(double) * npts * n, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (ib) *ib = lib;
    if (fout) *fout = fo;
    return st;
}

int nlh_nelder_mead_solve_batch_device(nlh_handle *h, const nlh_options *o, double init_size, int32_t nprob, int32_t n,
                                       nlh_device_vecfcn fcn, void *ctx, double *dx, double *dsimplex, int32_t use_simplex,
                                       double *fout, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;                  // :166-174
    if (!o || n < 1 || nprob < 0 || (nprob > 0 && !dx) || (use_simplex && !dsimplex)) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t slice = slice_simplex(n);
    const size_t npts = (size_t)n + 1;
    int rc;
    double *dsim = dsimplex;
    if (!dsim) {                                                     // a simplex of the library's own, one slice long
        if ((rc = ensure(h, h->bfB, sizeof(double) * (size_t)std::min(slice, nprob) * npts * n))) return rc;
        dsim = (double *)h->bfB.p;
    }
    NmEval ev = [&](int32_t npoints, const int32_t *dprob, const double *dxs, double *dfs) -> int {
        const int urc = fcn(ctx, (void *)h->stream, npoints, dprob, n, dxs, 1, dfs);
        return urc ? launcher_failed(h, urc, "fcnnvar") : 0;
    };
    const BatchIO io = {dx, nullptr, fout, ib, status};
    return lockstep_slices(nprob, slice, [&](int32_t p0, int32_t cnt) {
        const BatchIO q = io.at(p0, 1, n);
        return nm_lockstep(h, o, init_size, cnt, n, p0, ev, q.x, dsimplex ? dsim + (size_t)p0 * npts * n : dsim, use_simplex != 0, false,
                           q.fout, q.ib, q.status);
    });
}

// The same behind host arrays x [nprob][n] (what nlh_dq_model_nelder_mead_solve runs on a user's model).
int nlh_nm_solve_batch_device_h(nlh_handle *h, const nlh_options *o, double init_size, int32_t nprob, int32_t n,
                                nlh_device_vecfcn fcn, void *ctx, double *x, double *fout, nlh_iteration_behavior *ib,
                                int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (!o || n < 1 || nprob < 0 || (nprob > 0 && !x)) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    return staged_call(h, {{x, sizeof(double) * (size_t)nprob * n, true, true, &h->xdev}}, [&](void *const *d) {
        return nlh_nelder_mead_solve_batch_device(h, o, init_size, nprob, n, fcn, ctx, (double *)d[0], nullptr, 0, fout, ib, status);
    });
}
