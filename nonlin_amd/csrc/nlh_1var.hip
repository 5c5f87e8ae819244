// nlh_1var.hip -- brent_solver and newton_1var_solver (brent_solve / newt1var_solve, src/nonlin_solve.f90:643-1032) and
// fcn1var_helper%diff (f1h_diff_fcn, src/nonlin_single_var.f90:154-200): the lock-step device state machine of
// nlh_kernels_1var.h for a batch of the user's device functions, and the same machine with nprob = 1 behind host
// callbacks (the points of a round copied out, evaluated in list order, the values copied back).
#include "nlh_internal.h"
#include "nlh_kernels_1var.h"

// How a round's points are evaluated: npoints points xs [npoints] of problems dprob, values to fs [npoints] and, when
// diff_round, derivatives to ds [npoints] (DEVICE).  dneed [npoints] (DEVICE, host-callback form only): which points want
// the derivative.
using R1Eval = std::function<int(int32_t npoints, const int32_t *dprob, const double *xs, double *fs, double *ds,
                                 const int32_t *dneed, bool diff_round)>;

// brent_solve / newt1var_solve for nprob problems: dlim [nprob][2] device, dx [nprob] device (brent: 0 unless converged;
// newton: the last x, untouched on an invalid bracket).  host: the host-callback form (the derivative is called point by
// point where it is wanted); echo: print_status (only there).  One 4-byte read-back per round.
static int r1_lockstep(nlh_handle *h, const nlh_options *o, int kind, bool user_diff, bool want_f, int32_t nprob,
                       int32_t pbase, const R1Eval &eval, const double *dlim, double *dx, bool host, bool echo, double *hfout,
                       nlh_iteration_behavior *ib, int32_t *status)
{
    int rc;
    const size_t np = (size_t)nprob;
    const size_t nb = (np + 1023) / 1024;                            // runs of the scan
    // slots, pt0, pt1, fo [np]; staging: points, values, derivatives [2 np]
    if ((rc = ensure(h, h->qxV, sizeof(double) * (np * (R1_NSLOT + 3) + 6 * np)))) return rc;
    // phase, iter, neval, ndiff, bits, cnt, off [np]; dprob, dneed [2 np]; bsum, bpre [nb]; total
    if ((rc = ensure(h, h->misc, sizeof(int32_t) * (11 * np + 2 * nb + 16)))) return rc;
    if ((rc = ensure(h, h->state, sizeof(R1Print) * (echo ? np : 1)))) return rc;
    if ((rc = ensure_pinned(h, (sizeof(int32_t) * 4 + sizeof(double)) * np + 64 + sizeof(R1Print)))) return rc;
    double *q = (double *)h->qxV.p;
    R1Soa S;
    for (int k = 0; k < R1_NSLOT; ++k) { S.s[k] = q; q += np; }
    S.pt0 = q; q += np;
    S.pt1 = q; q += np;
    S.fo = q; q += np;
    double *dxs = q; q += 2 * np;
    double *dfs = q; q += 2 * np;
    double *dds = q;
    int32_t *dtotal = (int32_t *)h->misc.p, *ip = dtotal + 16;
    S.phase = ip; ip += np;
    S.iter = ip; ip += np;
    S.neval = ip; ip += np;
    S.ndiff = ip; ip += np;
    S.bits = ip; ip += np;
    int32_t *dcnt = ip; ip += np;
    int32_t *doff = ip; ip += np;
    int32_t *dprob = ip; ip += 2 * np;
    int32_t *dneed = ip; ip += 2 * np;
    int32_t *dbsum = ip; ip += nb;
    int32_t *dbpre = ip;
    R1Print *dpr = echo ? (R1Print *)h->state.p : nullptr;
    int32_t *htotal = (int32_t *)h->pinned;
    R1Print *hpr = (R1Print *)((char *)h->pinned + 16);
    char *hout = (char *)h->pinned + 64 + sizeof(R1Print);
    hipStream_t s = h->stream;
    R1Opts ro;
    ro.ftol = o->ftol; ro.xtol = o->xtol; ro.dtol = o->gtol; ro.max_evals = o->max_evals;
    ro.user_diff = user_diff ? 1 : 0; ro.want_f = want_f ? 1 : 0; ro.pad = 0;
    const bool flags = host && user_diff;                          // the host calls the derivative point by point
    const int eb = (nprob + 255) / 256;

    // every live problem evaluates at least once per round and stops once neval >= max_evals: a bound, not a knob
    const long max_rounds = std::max<long>((long)o->max_evals, 3) + 8;
    for (long round = 0;; ++round) {
        if (kind == R1_BRENT)
            hipLaunchKernelGGL(k_r1_advance<R1_BRENT>, dim3((unsigned)nb), dim3(1024), 0, s, nprob, round == 0 ? 1 : 0, ro, dlim,
                               (const double *)dfs, (const double *)dds, doff, S, dx, dpr, dcnt, dbsum);
        else
            hipLaunchKernelGGL(k_r1_advance<R1_NEWTON>, dim3((unsigned)nb), dim3(1024), 0, s, nprob, round == 0 ? 1 : 0, ro, dlim,
                               (const double *)dfs, (const double *)dds, doff, S, dx, dpr, dcnt, dbsum);
        hipLaunchKernelGGL(k_nm_scan_top, dim3(1), dim3(1024), 0, s, (int)nb, (const int32_t *)dbsum, dbpre, dtotal);
        hipLaunchKernelGGL(k_r1_emit, dim3(eb), dim3(256), 0, s, nprob, pbase, (const double *)S.pt0, (const double *)S.pt1,
                           (const int32_t *)S.phase, (const int32_t *)dcnt, doff, (const int32_t *)dbpre, dxs, dprob,
                           flags ? dneed : nullptr);
        HIPCHK(h, hipMemcpyAsync(htotal, dtotal, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        if (echo) HIPCHK(h, hipMemcpyAsync(hpr, dpr, sizeof(R1Print), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (echo && round > 0 && hpr->due) {                        // brent :808-810, newton :999-1001
            char buf[256];
            nlh_format_status(hpr->iter, hpr->neval, hpr->njac, hpr->xnorm, hpr->fnorm, buf, (int32_t)sizeof buf);
            fputs(buf, stdout);
            fflush(stdout);
        }
        const int32_t total = *htotal;
        if (total == 0) break;
        if (round > max_rounds) { h->err = "brent / newton_1var: the round bound was exceeded"; return NLH_ERR_HIP; }
        if ((rc = eval(total, dprob, dxs, dfs, dds, flags ? dneed : nullptr, round > 0))) return rc;
    }
    int32_t *hit = (int32_t *)hout, *hne = hit + np, *hnd = hne + np, *hbits = hnd + np;
    double *hfo = (double *)(hbits + np);
    HIPCHK(h, hipMemcpyAsync(hit, S.iter, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hne, S.neval, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hnd, S.ndiff, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(hbits, S.bits, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    if (hfout) HIPCHK(h, hipMemcpyAsync(hfo, S.fo, sizeof(double) * np, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    HIPCHK(h, hipGetLastError());
    for (size_t p = 0; p < np; ++p) {
        const int32_t b = hbits[p];
        if (ib) {
            ib[p].iter_count = hit[p]; ib[p].fcn_count = hne[p]; ib[p].jacobian_count = hnd[p]; ib[p].gradient_count = 0;
            ib[p].converge_on_fcn = (b & R1_FCNVRG) != 0; ib[p].converge_on_chng = (b & R1_XCNVRG) != 0;
            ib[p].converge_on_zero_diff = (b & R1_DCNVRG) != 0;
        }
        if (status) status[p] = (b & R1_INVALID) ? NLH_INVALID_INPUT_ERROR : ((b & R1_FLAG) ? NLH_CONVERGENCE_ERROR : 0);
        if (hfout) hfout[p] = hfo[p];
    }
    return 0;
}

// One problem behind host callbacks (fcnnvar flattened to C, called with n = 1).
static int r1_host(nlh_handle *h, const nlh_options *o, int kind, nlh_fcnnvar fcn, nlh_fcnnvar diff, void *ctx, double x1,
                   double x2, double *x, double *f, nlh_iteration_behavior *ib)
{
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->xdev, sizeof(double) * 3))) return rc;
    double *dlim = (double *)h->xdev.p, *dx = dlim + 2;
    const double hl[3] = {x1, x2, *x};
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(dlim, hl, sizeof hl, hipMemcpyHostToDevice, s));
    std::vector<double> hx, hf, hd;
    std::vector<int32_t> hn;
    R1Eval ev = [&](int32_t npoints, const int32_t *, const double *dxs, double *dfs, double *dds, const int32_t *dneed,
                    bool) -> int {
        hx.resize((size_t)npoints); hf.resize((size_t)npoints); hd.assign((size_t)npoints, 0.0); hn.assign((size_t)npoints, 0);
        HIPCHK(h, hipMemcpyAsync(hx.data(), dxs, sizeof(double) * npoints, hipMemcpyDeviceToHost, s));
        if (dneed) HIPCHK(h, hipMemcpyAsync(hn.data(), dneed, sizeof(int32_t) * npoints, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (int32_t k = 0; k < npoints; ++k) {                      // list order: f, then f' where it is wanted
            hf[k] = fcn(ctx, 1, &hx[k]);
            if (hn[k]) hd[k] = diff(ctx, 1, &hx[k]);
        }
        HIPCHK(h, hipMemcpyAsync(dfs, hf.data(), sizeof(double) * npoints, hipMemcpyHostToDevice, s));
        if (dneed) HIPCHK(h, hipMemcpyAsync(dds, hd.data(), sizeof(double) * npoints, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipStreamSynchronize(s));                          // (hf, hd are pageable and reused next round)
        return 0;
    };
    nlh_iteration_behavior lib;
    int32_t st = 0;
    double fo = 0.0;
    if ((rc = r1_lockstep(h, o, kind, diff != nullptr, f != nullptr, 1, 0, ev, dlim, dx, true, o->print_status != 0, &fo, &lib,
                          &st)))
        return rc;
    HIPCHK(h, hipMemcpyAsync(x, dx, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (ib) *ib = lib;
    if (f) *f = fo;
    return st;
}

int nlh_brent_solve(nlh_handle *h, const nlh_options *o, nlh_fcnnvar fcn, void *ctx, double x1, double x2, double *x, double *f,
                    nlh_iteration_behavior *ib)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib) memset(ib, 0, sizeof *ib);                               // :701-709
    if (x) *x = 0.0;                                                 // :691
    if (f) *f = 0.0;                                                 // :700
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;                  // :712
    if (!o || !x) return NLH_INVALID_INPUT_ERROR;
    return r1_host(h, o, R1_BRENT, fcn, nullptr, ctx, x1, x2, x, f, ib);
}

int nlh_newton_1var_solve(nlh_handle *h, const nlh_options *o, nlh_fcnnvar fcn, nlh_fcnnvar diff, void *ctx, double x1,
                          double x2, double *x, double *f, nlh_iteration_behavior *ib)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib) memset(ib, 0, sizeof *ib);                               // :884-892
    if (f) *f = 0.0;                                                 // :883
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;                  // :898
    if (!o || !x) return NLH_INVALID_INPUT_ERROR;
    return r1_host(h, o, R1_NEWTON, fcn, diff, ctx, x1, x2, x, f, ib);
}

static int r1_batch_device(nlh_handle *h, const nlh_options *o, int kind, int32_t nprob, nlh_device_vecfcn fcn,
                           nlh_device_jacfcn diff, void *ctx, const double *dlim, double *dx, double *fout,
                           nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (!o || nprob < 0 || (nprob > 0 && (!dlim || !dx))) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    R1Eval ev = [&](int32_t npoints, const int32_t *dprob, const double *dxs, double *dfs, double *dds, const int32_t *,
                    bool diff_round) -> int {
        int urc = fcn(ctx, (void *)h->stream, npoints, dprob, 1, dxs, 1, dfs);
        if (urc) return launcher_failed(h, urc, "fcn1var");
        if (diff && diff_round && (urc = diff(ctx, (void *)h->stream, npoints, dprob, 1, dxs, 1, dds)))
            return launcher_failed(h, urc, "fcn1var", "derivative launcher");
        return 0;
    };
    const BatchIO io = {dx, nullptr, fout, ib, status};
    return lockstep_slices(nprob, slice_root1v(), [&](int32_t p0, int32_t cnt) {
        const BatchIO q = io.at(p0, 1, 1);
        return r1_lockstep(h, o, kind, diff != nullptr, fout != nullptr, cnt, p0, ev, dlim + 2 * (size_t)p0, q.x, false, false, q.fout, q.ib,
                           q.status);
    });
}

int nlh_brent_solve_batch_device(nlh_handle *h, const nlh_options *o, int32_t nprob, nlh_device_vecfcn fcn, void *ctx,
                                 const double *dlim, double *dx, double *fout, nlh_iteration_behavior *ib, int32_t *status)
{
    return r1_batch_device(h, o, R1_BRENT, nprob, fcn, nullptr, ctx, dlim, dx, fout, ib, status);
}

int nlh_newton_1var_solve_batch_device(nlh_handle *h, const nlh_options *o, int32_t nprob, nlh_device_vecfcn fcn,
                                       nlh_device_jacfcn diff, void *ctx, const double *dlim, double *dx, double *fout,
                                       nlh_iteration_behavior *ib, int32_t *status)
{
    return r1_batch_device(h, o, R1_NEWTON, nprob, fcn, diff, ctx, dlim, dx, fout, ib, status);
}

// The same behind host arrays lim [nprob][2], x [nprob] (what the model entry points run on a user's model).
int nlh_root1v_solve_batch_device_h(nlh_handle *h, const nlh_options *o, int newton, int32_t nprob, nlh_device_vecfcn fcn,
                                    nlh_device_jacfcn diff, void *ctx, const double *lim, double *x, double *fout,
                                    nlh_iteration_behavior *ib, int32_t *status)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (ib && nprob > 0) memset(ib, 0, sizeof(*ib) * (size_t)nprob);
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (!o || nprob < 0 || (nprob > 0 && (!lim || !x))) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    return staged_call(h, {{const_cast<double *>(lim), sizeof(double) * 2 * (size_t)nprob, true, false, &h->fdev},
                           {x, sizeof(double) * (size_t)nprob, true, true, &h->xdev}}, [&](void *const *d) {
        return r1_batch_device(h, o, newton ? R1_NEWTON : R1_BRENT, nprob, fcn, newton ? diff : nullptr, ctx, (const double *)d[0],
                               (double *)d[1], fout, ib, status);
    });
}

// fcn1var_helper%diff on the host: the user's derivative, or the forward difference of :189-198 (f at x + h first, then
// f at x unless fv is given; divided by h, not by (x + h) - x).
int nlh_fd_derivative(nlh_fcnnvar fcn, nlh_fcnnvar diff, void *ctx, double x, const double *fv, double *df)
{
    if (!df) return NLH_INVALID_INPUT_ERROR;
    if (diff) { *df = diff(ctx, 1, &x); return 0; }                  // :184-186
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    double hstep = NLH_SQRT_EPS * fabs(x);                           // :189
    if (hstep < NLH_EPS) hstep = NLH_SQRT_EPS;                       // :190
    double temp = x + hstep;                                         // :191
    const double f1 = fcn(ctx, 1, &temp);                            // :192
    double xx = x;
    const double f0 = fv ? *fv : fcn(ctx, 1, &xx);                   // :193-197
    *df = (f1 - f0) / hstep;                                         // :198
    return 0;
}
