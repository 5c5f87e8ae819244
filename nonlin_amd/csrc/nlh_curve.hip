// nlh_curve.hip -- the built-in curve models: Gaussian / Lorentzian peaks and exponential decays on a polynomial baseline
// (kernels and arithmetic: nlh_kernels_curve.h) as library-owned launchers of the open device-residual path, so that the
// lock-step machines of least_squares_solver, constrained_least_squares_solver and the covariance chain fit them without
// knowing them.  Here: the launchers and which workgroup form a call runs, model values at arbitrary abscissae
// (nlh_curve_eval_batch), and the one-call fit + errors (nlh_curve_fit_batch: solve, covariance at the solution, the
// degrees of freedom of zero-weight padding).  The model object that owns its data is nlh_curve_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_kernels_curve.h"

int32_t nlh_curve_nparams(int32_t kind, int32_t ncomp, int32_t nbase)
{
    if (kind != NLH_CURVE_GAUSS && kind != NLH_CURVE_LORENTZ && kind != NLH_CURVE_EXPDECAY) return -1;
    if (ncomp < 1 || nbase < -1 || nbase > NLH_CURVE_MAX_BASE) return -1;
    const int64_t n = (int64_t)(kind == NLH_CURVE_EXPDECAY ? 2 : 3) * ncomp + nbase + 1;
    return n > NLH_CURVE_MAX_N ? -1 : (int32_t)n;
}

// The form a launch runs: flat (several points per workgroup) while two points or more fit a workgroup's 256 threads.
// NLH_CURVE_FORM = row | flat (environment, read at every call; tests) forces a form for the sizes it can hold: flat holds
// m <= 256 with the workgroup's x vectors inside CURVE_FLAT_LDS.
static const size_t CURVE_FLAT_LDS = 32 * 1024;
static bool curve_flat(int m, int n)
{
    if (m > 256) return false;
    const int ppw = 256 / m;
    if (sizeof(double) * (size_t)ppw * n > CURVE_FLAT_LDS) return false;
    if (const char *e = getenv("NLH_CURVE_FORM")) {
        if (!strcmp(e, "row")) return false;
        if (!strcmp(e, "flat")) return true;
    }
    return ppw >= 2;
}

template <int KIND>
static void curve_launch_kind(bool jac, const CurveData &cd, int n, int npoints, const int32_t *dprob, const double *dX, double *out,
                              hipStream_t s)
{
    const int m = cd.m;
    if (curve_flat(m, n)) {
        const int ppw = 256 / m;
        const dim3 grid((unsigned)((npoints + ppw - 1) / ppw));
        const size_t lds = sizeof(double) * (size_t)ppw * n;
        if (jac) hipLaunchKernelGGL((k_curve_jac<KIND, true>), grid, dim3(256), lds, s, cd, n, 1, ppw, npoints, dprob, dX, out);
        else hipLaunchKernelGGL((k_curve_fcn<KIND, true>), grid, dim3(256), lds, s, cd, n, 1, ppw, npoints, dprob, dX, out);
        return;
    }
    const int nblk = (m + 255) / 256;
    const dim3 grid((unsigned)((size_t)npoints * nblk));
    const size_t lds = sizeof(double) * (size_t)n;
    if (jac) hipLaunchKernelGGL((k_curve_jac<KIND, false>), grid, dim3(256), lds, s, cd, n, nblk, 1, npoints, dprob, dX, out);
    else hipLaunchKernelGGL((k_curve_fcn<KIND, false>), grid, dim3(256), lds, s, cd, n, nblk, 1, npoints, dprob, dX, out);
}

// Checks everything, launches nothing when anything is wrong.  y == nullptr: model values (no data term, no weights).
static int curve_launch(bool jac, int kind, int K, int B, int shared_t, int m, const double *t, const double *y, const double *w,
                        int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, double *out, hipStream_t s)
{
    const int32_t np = nlh_curve_nparams(kind, K, B);
    if (np < 0 || np != n || m < 1 || !t || !dX || !out) return NLH_INVALID_INPUT_ERROR;
    if (npoints <= 0) return 0;
    if ((size_t)npoints * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    CurveData cd;
    cd.K = K; cd.B = B; cd.shared_t = shared_t != 0; cd.m = m; cd.t = t; cd.y = y; cd.w = w;
    if (kind == NLH_CURVE_GAUSS) curve_launch_kind<NLH_CURVE_GAUSS>(jac, cd, n, npoints, dprob, dX, out, s);
    else if (kind == NLH_CURVE_LORENTZ) curve_launch_kind<NLH_CURVE_LORENTZ>(jac, cd, n, npoints, dprob, dX, out, s);
    else curve_launch_kind<NLH_CURVE_EXPDECAY>(jac, cd, n, npoints, dprob, dX, out, s);
    return 0;
}

int nlh_curve_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                         double *dF)
{
    const nlh_curve_ctx *c = (const nlh_curve_ctx *)ctx;
    if (!c || m != c->m || !c->dy || !dprob) return NLH_INVALID_INPUT_ERROR;
    return curve_launch(false, c->kind, c->ncomp, c->nbase, c->shared_t, c->m, c->dt, c->dy, c->dw, npoints, dprob, n, dX, dF,
                        (hipStream_t)hip_stream);
}

int nlh_curve_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                         double *dJ)
{
    const nlh_curve_ctx *c = (const nlh_curve_ctx *)ctx;
    if (!c || m != c->m || !c->dy || !dprob) return NLH_INVALID_INPUT_ERROR;
    return curve_launch(true, c->kind, c->ncomp, c->nbase, c->shared_t, c->m, c->dt, c->dy, c->dw, npoints, dprob, n, dX, dJ,
                        (hipStream_t)hip_stream);
}

// the checks every entry point with (kind, ncomp, nbase, nprob, m) makes, in the documented order
static int curve_shape_check(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, bool data, int32_t *n)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    *n = nlh_curve_nparams(kind, ncomp, nbase);
    if (*n < 0 || nprob < 0 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (data && m < *n) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    return 0;
}

int nlh_curve_eval_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t npts, const double *dt,
                         int32_t shared_t, const double *dx, double *dy)
{
    int32_t n;
    int rc = curve_shape_check(h, kind, ncomp, nbase, nprob, npts, false, &n);
    if (rc) return rc;
    if (nprob == 0) return 0;
    if (!dt || !dx || !dy) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = curve_launch(false, kind, ncomp, nbase, shared_t, npts, dt, nullptr, nullptr, nprob, nullptr, n, dx, dy, h->stream))) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fit + errors
// ---------------------------------------------------------------------------------------------------------------------
// The composition for any launcher pair (nlh_internal.h: nlh_fit_compose); nlh_curve_fit_batch and nlh_expr_fit_batch are it.
int nlh_fit_compose(nlh_handle *h, const nlh_options *opts, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                    nlh_device_jacfcn jac, void *ctx, const std::function<void(int32_t)> &at, const double *dw, const double *xl,
                    const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                    nlh_iteration_behavior *ib, int32_t *status)
{
    int rc;
    const bool errors = dsigma || dcov || dchi2;
    if (errors && m <= n) return NLH_INVALID_INPUT_ERROR;        // no degree of freedom (nlh_lm_covariance_batch_device, scaled)
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t np = (size_t)nprob, nn = (size_t)n * n;
    // the handle's own buffer for this entry point: status and non-zero-weight counts, a cov when the caller wants none
    const size_t ints = 2 * np + 2;
    if ((rc = ensure(h, h->crv, sizeof(int32_t) * ints + sizeof(double) * (errors && !dcov ? np * nn : 0) + 64))) return rc;
    int32_t *dstat = (int32_t *)h->crv.p, *dnz = dstat + np;
    double *cov = dcov ? dcov : (double *)(dstat + (ints & ~(size_t)1));
    std::vector<int32_t> st(np, 0), nz;
    if (dw) {                                                    // degrees of freedom, before anything is evaluated
        nz.resize(np);
        hipLaunchKernelGGL(k_curve_count, dim3((nprob + 63) / 64), dim3(64), 0, s, nprob, m, dw, dnz);
        HIPCHK(h, hipMemcpyAsync(nz.data(), dnz, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (size_t p = 0; p < np; ++p)
            if (nz[p] - n <= 0) st[p] = NLH_INVALID_INPUT_ERROR;
    }
    // runs of consecutive problems that have degrees of freedom (all of them, as a rule): exactly the calls a user makes
    for (int32_t p0 = 0; p0 < nprob;) {
        if (st[p0]) { ++p0; continue; }
        int32_t p1 = p0;
        while (p1 < nprob && !st[p1]) ++p1;
        const int32_t cnt = p1 - p0;
        at(p0);
        double *xs = dx + (size_t)p0 * n, *fs = dfvec + (size_t)p0 * m;
        nlh_iteration_behavior *ibs = ib ? ib + p0 : nullptr;
        if (xl || xu) rc = nlh_cls_solve_batch_device(h, opts, 1.0, 1.0, xl, xu, cnt, m, n, fcn, jac, ctx, xs, fs, ibs, &st[p0]);
        else rc = nlh_lm_solve_batch_device(h, opts, cnt, m, n, fcn, jac, ctx, xs, fs, ibs, &st[p0]);
        if (rc) return rc;
        if (errors &&
            (rc = nlh_lm_covariance_batch_device(h, cnt, m, n, fcn, jac, ctx, xs, 1, 0.0, cov + (size_t)p0 * nn,
                                                 dsigma ? dsigma + (size_t)p0 * n : nullptr, drank ? drank + p0 : nullptr,
                                                 dchi2 ? dchi2 + p0 : nullptr))) return rc;
        p0 = p1;
    }
    if (errors) {
        HIPCHK(h, hipMemcpyAsync(dstat, st.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_curve_post, dim3((nprob + 63) / 64), dim3(64), 0, s, nprob, m, n, (const int32_t *)dstat,
                           dw ? (const int32_t *)dnz : (const int32_t *)nullptr, (const double *)dfvec, cov, dsigma, dchi2, drank);
        HIPCHK(h, hipStreamSynchronize(s));                      // (st is a host vector)
    }
    if (status) memcpy(status, st.data(), sizeof(int32_t) * np);
    if (ib)
        for (size_t p = 0; p < np; ++p)
            if (st[p] == NLH_INVALID_INPUT_ERROR && nz.size() && nz[p] - n <= 0) ib[p] = nlh_iteration_behavior{};
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_curve_fit_batch(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                        const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                        const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                        nlh_iteration_behavior *ib, int32_t *status)
{
    int32_t n;
    int rc = curve_shape_check(h, kind, ncomp, nbase, nprob, m, true, &n);
    if (rc) return rc;
    if (nprob == 0) return 0;
    if (!opts || !dt || !dy || !dx || !dfvec) return NLH_INVALID_INPUT_ERROR;
    nlh_curve_ctx c;
    c.kind = kind; c.ncomp = ncomp; c.nbase = nbase; c.shared_t = shared_t != 0; c.m = m;
    auto at = [&](int32_t p0) {
        c.dt = shared_t ? dt : dt + (size_t)p0 * m;
        c.dy = dy + (size_t)p0 * m;
        c.dw = dw ? dw + (size_t)p0 * m : nullptr;
    };
    return nlh_fit_compose(h, opts, nprob, m, n, nlh_curve_device_fcn, analytic ? nlh_curve_device_jac : nullptr, &c, at, dw, xl, xu, dx,
                           dfvec, dsigma, dcov, dchi2, drank, ib, status);
}

// ... behind HOST arrays (nlh_internal.h: nlh_fit_compose_h): t (tm doubles), y, w, x, fvec, sigma, cov, chi2, rank
int nlh_fit_compose_h(nlh_handle *h, const char *what, size_t tm, int32_t nprob, int32_t m, int32_t n, const double *t, const double *y,
                      const double *w, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                      const std::function<int(const double *, const double *, const double *, double *, double *, double *, double *,
                                              double *, int32_t *)> &fit, int32_t nfree)
{
    int rc;
    if ((sigma || cov || chi2) && m <= (nfree >= 0 ? nfree : n)) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t np = (size_t)nprob, pm = np * m, nn = (size_t)n * n;
    const size_t doubles = tm + pm * (w ? 3 : 2) + np * n + (sigma ? np * n : 0) + (cov ? np * nn : 0) + (chi2 ? np : 0);
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * doubles + sizeof(int32_t) * np) != hipSuccess) {
        h->err = std::string("hipMalloc (") + what + ")";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    double *q = base;
    double *dt = q; q += tm;
    double *dy = q; q += pm;
    double *dw = w ? q : nullptr; q += w ? pm : 0;
    double *df = q; q += pm;
    double *dx = q; q += np * n;
    double *ds = sigma ? q : nullptr; q += sigma ? np * n : 0;
    double *dc = cov ? q : nullptr; q += cov ? np * nn : 0;
    double *dq = chi2 ? q : nullptr; q += chi2 ? np : 0;
    int32_t *dr = rank ? (int32_t *)q : nullptr;
    hipError_t e = hipMemcpyAsync(dt, t, sizeof(double) * tm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dy, y, sizeof(double) * pm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && w) e = hipMemcpyAsync(dw, w, sizeof(double) * pm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dx, x, sizeof(double) * np * n, hipMemcpyHostToDevice, s);
    rc = 0;
    if (e == hipSuccess) rc = fit(dt, dy, dw, dx, df, ds, dc, dq, dr);
    if (e == hipSuccess && !rc) {
        e = hipMemcpyAsync(x, dx, sizeof(double) * np * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(fvec, df, sizeof(double) * pm, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && sigma) e = hipMemcpyAsync(sigma, ds, sizeof(double) * np * n, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && cov) e = hipMemcpyAsync(cov, dc, sizeof(double) * np * nn, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && chi2) e = hipMemcpyAsync(chi2, dq, sizeof(double) * np, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && rank) e = hipMemcpyAsync(rank, dr, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(base);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        h->err = std::string(what) + " (host arrays): " + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return rc;
}

int nlh_curve_fit_batch_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                          const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                          const double *xu, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                          nlh_iteration_behavior *ib, int32_t *status)
{
    int32_t n;
    int rc = curve_shape_check(h, kind, ncomp, nbase, nprob, m, true, &n);
    if (rc) return rc;
    if (nprob == 0) return 0;
    if (!opts || !t || !y || !x || !fvec) return NLH_INVALID_INPUT_ERROR;
    return nlh_fit_compose_h(h, "curve fit", shared_t ? (size_t)m : (size_t)nprob * m, nprob, m, n, t, y, w, x, fvec, sigma, cov, chi2, rank,
                             [&](const double *dt, const double *dy, const double *dw, double *dx, double *df, double *ds, double *dc,
                                 double *dq, int32_t *dr) {
                                 return nlh_curve_fit_batch(h, opts, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, dx,
                                                            df, ds, dc, dq, dr, ib, status);
                             });
}
