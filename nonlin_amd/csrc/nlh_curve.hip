// nlh_curve.hip -- the built-in curve models: Gaussian / Lorentzian peaks and exponential decays on a polynomial baseline
// (kernels and arithmetic: nlh_kernels_curve.h) as library-owned launchers of the open device-residual path, so that the
// lock-step machines of least_squares_solver, constrained_least_squares_solver and the covariance chain fit them without
// knowing them.  Here: the launchers and which workgroup form a call runs, model values at arbitrary abscissae
// (nlh_curve_eval_batch), and the eight one-call fits nlh_curve_fit_batch*: a curve model as the FitSource of the pipeline
// (nlh_fit.hip).  The model object that owns its data is nlh_curve_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
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
    return m <= 256 && sizeof(double) * (size_t)(256 / m) * n <= CURVE_FLAT_LDS && launch_flat("NLH_CURVE_FORM", m);
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

int nlh_curve_eval_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t npts, const double *dt,
                         int32_t shared_t, const double *dx, double *dy)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t n = nlh_curve_nparams(kind, ncomp, nbase);
    if (n < 0 || nprob < 0 || npts < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    int rc;
    if (!dt || !dx || !dy) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = curve_launch(false, kind, ncomp, nbase, shared_t, npts, dt, nullptr, nullptr, nprob, nullptr, n, dx, dy, h->stream))) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}

// The model itself as a launcher pair -- no data term, no weights: what nlh_curve_eval_batch launches, with a problem list --
// for the band (nlh_band.hip), on a context of the call's own.
static int curve_value_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                           double *dF)
{
    const nlh_curve_ctx *c = (const nlh_curve_ctx *)ctx;
    if (!c || m != c->m || !dprob) return NLH_INVALID_INPUT_ERROR;
    return curve_launch(false, c->kind, c->ncomp, c->nbase, c->shared_t, c->m, c->dt, nullptr, nullptr, npoints, dprob, n, dX, dF,
                        (hipStream_t)hip_stream);
}

static int curve_value_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                           double *dJ)
{
    const nlh_curve_ctx *c = (const nlh_curve_ctx *)ctx;
    if (!c || m != c->m || !dprob) return NLH_INVALID_INPUT_ERROR;
    return curve_launch(true, c->kind, c->ncomp, c->nbase, c->shared_t, c->m, c->dt, nullptr, nullptr, npoints, dprob, n, dX, dJ,
                        (hipStream_t)hip_stream);
}

int nlh_curve_band_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t npts, const double *dt,
                         int32_t shared_t, const double *dx, const double *dcov, const double *dnoise, double *dy, double *dsd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t n = nlh_curve_nparams(kind, ncomp, nbase);
    if (n < 0 || nprob < 0 || npts < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!dt || !dx || !dcov || !dsd) return NLH_INVALID_INPUT_ERROR;
    nlh_curve_ctx c;
    c.kind = kind; c.ncomp = ncomp; c.nbase = nbase; c.shared_t = shared_t != 0; c.m = npts; c.dt = dt; c.dy = nullptr; c.dw = nullptr;
    return nlh_propagate_batch_device(h, nprob, npts, n, curve_value_fcn, curve_value_jac, &c, dx, dcov, dnoise, dy, dsd);
}

// ---------------------------------------------------------------------------------------------------------------------
// fit + errors: the pipeline of nlh_fit.hip on a curve model
// ---------------------------------------------------------------------------------------------------------------------
static void curve_bind(void *ctx, const double *dt, const double *dy, const double *dw, int32_t p0)
{
    nlh_curve_ctx *c = (nlh_curve_ctx *)ctx;
    const size_t at = (size_t)p0 * c->m;
    c->dt = c->shared_t ? dt : dt + at;
    c->dy = dy + at;
    c->dw = dw ? dw + at : nullptr;
}

static int curve_fit(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t analytic, const FitArgs &a,
                     bool host)
{
    nlh_curve_ctx c;                                              // (its data pointers: curve_bind, before every run of problems)
    c.kind = kind; c.ncomp = ncomp; c.nbase = nbase; c.shared_t = a.shared_t != 0; c.m = a.m;
    const FitSource src = {nlh_curve_nparams(kind, ncomp, nbase), 1, "curve fit", nlh_curve_device_fcn,
                           analytic ? nlh_curve_device_jac : nullptr, &c, curve_bind};
    return nlh_fit_run(h, opts, src, a, host);
}

int nlh_curve_fit_batch(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                        const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                        const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                        nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, dx,
                                                             dfvec, dsigma, dcov, dchi2, drank, ib, status}, false);
}

int nlh_curve_fit_batch_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                          const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                          const double *xu, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                          nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, x, fvec,
                                                             sigma, cov, chi2, rank, ib, status}, true);
}

int nlh_curve_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                             const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                             const double *xu, const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                             int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec,
                                                             dsigma, dcov, dchi2, drank, ib, status}, false);
}

int nlh_curve_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                               const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                               const double *xu, const nlh_pmap *pm, double *x, double *fvec, double *sigma, double *cov, double *chi2,
                               int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, x, fvec,
                                                             sigma, cov, chi2, rank, ib, status}, true);
}

int nlh_curve_fit_batch_loss(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                             const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                             const double *xu, const nlh_pmap *pm, int32_t loss, const double *dscale, int32_t shared_scale, double *dx,
                             double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                             int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, loss, dscale, shared_scale, dx, dfvec,
                                                             dsigma, dcov, dchi2, drank, ib, status}, false);
}

int nlh_curve_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                               const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                               const double *xu, const nlh_pmap *pm, int32_t loss, const double *scale, int32_t shared_scale, double *x,
                               double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib,
                               int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, loss, scale, shared_scale, x, fvec, sigma,
                                                             cov, chi2, rank, ib, status}, true);
}

int nlh_curve_fit_batch_pois(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *dt,
    int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu, const nlh_pmap *pm,
    double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
    nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, dx, dfvec, dsigma,
                                             dcov, dchi2, drank, ib, status, NLH_STAT_POISSON, mu_floor}, false);
}

int nlh_curve_fit_batch_pois_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *t,
    int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu, const nlh_pmap *pm,
    double mu_floor, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
    nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, NLH_LOSS_LINEAR, nullptr, 0, x, fvec, sigma,
                                             cov, chi2, rank, ib, status, NLH_STAT_POISSON, mu_floor}, true);
}

// The global fits: the loss (or the Poisson pair) wraps the curve per data set, the group wraps the result (nlh_fit.hip).
int nlh_curve_fit_batch_group(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                              const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                              const double *xu, const nlh_group *g, int32_t loss, const double *dscale, int32_t shared_scale, int32_t stat,
                              double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                              nlh_iteration_behavior *ib, int32_t *status)
{
    if (h && !g) return NLH_INVALID_INPUT_ERROR;
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, loss, dscale, shared_scale, dx,
                                                             dfvec, dsigma, dcov, dchi2, drank, ib, status, stat, mu_floor, g}, false);
}

int nlh_curve_fit_batch_group_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                                const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                                const double *xu, const nlh_group *g, int32_t loss, const double *scale, int32_t shared_scale, int32_t stat,
                                double mu_floor, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                                nlh_iteration_behavior *ib, int32_t *status)
{
    if (h && !g) return NLH_INVALID_INPUT_ERROR;
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, loss, scale, shared_scale, x, fvec,
                                                             sigma, cov, chi2, rank, ib, status, stat, mu_floor, g}, true);
}

// The fits with an instrument response: the convolving pair wraps the model's launchers, then the loss or the Poisson pair, then
// the map or the group (nlh_fit.hip).
int nlh_curve_fit_batch_conv(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *dt,
                              int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                              const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss, const double *dscale, int32_t shared_scale,
                              int32_t stat, double mu_floor, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                              int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    static const nlh_conv none{};                                 // (a NULL cv: refused where the ladder checks the transform)
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, pm, loss, dscale, shared_scale, dx, dfvec, dsigma, dcov, dchi2, drank,
            ib, status, stat, mu_floor, g, cv ? cv : &none}, false);
}

int nlh_curve_fit_batch_conv_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                              const nlh_group *g, const nlh_pmap *pm, const nlh_conv *cv, int32_t loss, const double *scale, int32_t shared_scale,
                              int32_t stat, double mu_floor, double *x, double *fvec, double *sigma, double *cov, double *chi2,
                              int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    static const nlh_conv none{};                                 // (a NULL cv: refused where the ladder checks the transform)
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, pm, loss, scale, shared_scale, x, fvec, sigma, cov, chi2, rank,
            ib, status, stat, mu_floor, g, cv ? cv : &none}, true);
}

// The separable fits: the convolving pair, if any, wraps the model's launchers, the projecting pair wraps that (nlh_fit.hip).
int nlh_curve_fit_batch_sep(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                            const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                            const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *dx, double *dfvec,
                            double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, dt, shared_t, dy, dw, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, dx,
                                                             dfvec, dsigma, dcov, dchi2, drank, ib, status, NLH_STAT_LSQ, 0.0, g, cv, true, sp,
                                                             nlh_curve_device_jac}, false);
}

int nlh_curve_fit_batch_sep_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                              const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                              const double *xu, const nlh_group *g, const nlh_conv *cv, const nlh_sep *sp, double *x, double *fvec,
                              double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    return curve_fit(h, opts, kind, ncomp, nbase, analytic, {nprob, m, t, shared_t, y, w, xl, xu, nullptr, NLH_LOSS_LINEAR, nullptr, 0, x, fvec,
                                                             sigma, cov, chi2, rank, ib, status, NLH_STAT_LSQ, 0.0, g, cv, true, sp,
                                                             nlh_curve_device_jac}, true);
}
