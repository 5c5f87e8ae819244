// nlh_loss.hip -- robust losses (include/nonlin_hip.h: nlh_loss_*): Huber, soft-L1 and Cauchy fits for any device model, as a
// pair of wrapping launchers around any inner launcher pair (kernels and arithmetic: nlh_kernels_loss.h).  Here: the wrapping
// context and its per-stream scratch, the launchers and the form a row scaling runs, nlh_loss_apply_batch, and the one-call
// fits with a loss (nlh_curve_fit_batch_loss, nlh_expr_fit_batch_loss: the loss wraps the model's launchers, the parameter
// map, if any, wraps the result).  The model object is nlh_loss_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_kernels_loss.h"

static const uint32_t LOSS_MAGIC = 0x73736f6cu;
static const size_t LOSS_SCRATCH_CAP = (size_t)1 << 30;          // per call, so per stream; beyond it the points go in slices

struct LossScratch { hipStream_t s; void *p; size_t bytes; };

struct nlh_loss_ctx {
    uint32_t magic = LOSS_MAGIC;
    int device = 0, cus = 1;
    int kind = NLH_LOSS_LINEAR;
    nlh_device_vecfcn fcn = nullptr;
    nlh_device_jacfcn jac = nullptr;
    void *inner = nullptr;
    const double *dscale = nullptr;
    int shared_scale = 0;
    // One buffer per stream, as a parameter map's context keeps them (nlh_pmap.hip): calls on one stream are ordered, calls
    // from several host threads come on different streams.  A buffer is at most the cap, is kept until nlh_loss_unwrap and
    // never shrinks.
    std::mutex mu;
    std::vector<LossScratch> scratch;
};

bool nlh_loss_kind_ok(int32_t kind) { return kind >= NLH_LOSS_LINEAR && kind <= NLH_LOSS_CAUCHY; }

// host scales: finite and positive, every one (LINEAR reads none)
bool nlh_loss_scale_ok(int32_t kind, const double *scale, size_t cnt)
{
    if (kind == NLH_LOSS_LINEAR) return true;
    if (!scale) return false;
    for (size_t p = 0; p < cnt; ++p)
        if (!(scale[p] > 0.0) || !std::isfinite(scale[p])) return false;
    return true;
}

int nlh_loss_wrap(nlh_handle *h, int32_t kind, const double *dscale, int32_t shared_scale, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                  void *inner_ctx, nlh_loss_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !nlh_loss_kind_ok(kind)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (kind != NLH_LOSS_LINEAR && !dscale) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    nlh_loss_ctx *c = new nlh_loss_ctx();
    c->device = h->device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) c->cus = cus;
    c->kind = kind; c->fcn = fcn; c->jac = jac; c->inner = inner_ctx; c->dscale = dscale; c->shared_scale = shared_scale != 0;
    *out = c;
    return 0;
}

void nlh_loss_unwrap(nlh_loss_ctx *c)
{
    if (!c || c->magic != LOSS_MAGIC) return;
    hipSetDevice(c->device);
    for (LossScratch &s : c->scratch) hipFree(s.p);               // (hipFree waits for the work that still uses it)
    c->magic = 0;
    delete c;
}

// Growing a buffer is hipFree + hipMalloc under the context's mutex, in the first calls of a solve, not per round.
static void *loss_scratch(nlh_loss_ctx *c, hipStream_t s, size_t bytes)
{
    std::lock_guard<std::mutex> lock(c->mu);
    LossScratch *b = nullptr;
    for (LossScratch &e : c->scratch) if (e.s == s) b = &e;
    if (!b) { c->scratch.push_back({s, nullptr, 0}); b = &c->scratch.back(); }
    if (b->bytes < bytes) {
        if (b->p) hipFree(b->p);
        b->p = nullptr; b->bytes = 0;
        if (hipMalloc(&b->p, bytes) != hipSuccess) { b->p = nullptr; return nullptr; }
        b->bytes = bytes;
    }
    return b->p;
}

// The form a row scaling runs, as the parameter maps choose it: flat while two or more points fit 256 threads (m <= 128).
// NLH_LOSS_FORM = row | flat (environment, read at every call; tests) forces a form for the sizes it can hold (flat: m <= 256).
static bool loss_flat(int m)
{
    if (m > 256) return false;
    if (const char *e = getenv("NLH_LOSS_FORM")) {
        if (!strcmp(e, "row")) return false;
        if (!strcmp(e, "flat")) return true;
    }
    return 256 / m >= 2;
}

// Groups the columns are split into: pmap_groups' occupancy argument (nlh_pmap.hip) -- below four workgroups of 256 threads per
// compute unit a streaming kernel does not keep enough loads in flight, so the columns are dealt over gridDim.y until the
// launch has that many (or a column per group).  NLH_LOSS_SPLIT (environment; tests) overrides.
static int loss_groups(int cus, size_t wgs, int n)
{
    size_t g = 1;
    const size_t want = (size_t)4 * cus;
    if (wgs < want) g = (want + wgs - 1) / wgs;
    if (const char *e = getenv("NLH_LOSS_SPLIT")) {
        const int v = atoi(e);
        if (v >= 1) g = (size_t)v;
    }
    return (int)std::min<size_t>(g, (size_t)n);
}

static void loss_launch_jac(const nlh_loss_ctx *c, const LossArgs &A, int m, int n, int npoints, const double *R, double *J, hipStream_t s)
{
    const bool flat = loss_flat(m);
    const int ppw = flat ? 256 / m : 1, nblk = flat ? 1 : (m + 255) / 256;
    const size_t wgs = flat ? (size_t)(npoints + ppw - 1) / ppw : (size_t)npoints * nblk;
    const int groups = loss_groups(c->cus, wgs, n);
    const int cpg = (n + groups - 1) / groups;
    const dim3 grid((unsigned)wgs, (unsigned)((n + cpg - 1) / cpg));
    if (flat) hipLaunchKernelGGL(k_loss_jac<true>, grid, dim3(256), 0, s, A, m, n, nblk, ppw, cpg, npoints, R, J);
    else hipLaunchKernelGGL(k_loss_jac<false>, grid, dim3(256), 0, s, A, m, n, nblk, ppw, cpg, npoints, R, J);
}

// Both launchers.  What they check themselves is refused before any launch; an inner error comes back as it is, with no
// further launch.  Scratch: the inner residual R of a Jacobian call, and a problem list for the inner launcher when the caller
// passed none.
static int loss_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_loss_ctx *c = (nlh_loss_ctx *)ctx;
    if (!c || c->magic != LOSS_MAGIC || !c->fcn) return NLH_INVALID_INPUT_ERROR;
    if (n < 1 || m < 1 || !dX || !out) return NLH_INVALID_INPUT_ERROR;
    if (jac && !c->jac) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (npoints <= 0) return 0;
    const bool lin = c->kind == NLH_LOSS_LINEAR;                  // no kernel of the table, no R: the inner pair's output as it is
    hipStream_t s = (hipStream_t)hip_stream;
    const bool needR = jac && !lin;
    const size_t per = (needR ? sizeof(double) * (size_t)m : 0) + (dprob ? 0 : sizeof(int32_t));
    size_t cap = LOSS_SCRATCH_CAP;
    if (const char *e = getenv("NLH_LOSS_SCRATCH")) {
        const long long v = atoll(e);
        if (v > 0 && (size_t)v < cap) cap = (size_t)v;
    }
    const int slice = per ? (int)std::max<size_t>(1, std::min<size_t>((size_t)npoints, cap / per)) : npoints;
    if ((size_t)slice * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return NLH_ERR_HIP;
    char *base = nullptr;
    if (per) {
        base = (char *)loss_scratch(c, s, (size_t)slice * per + 64);
        if (!base) return NLH_OUT_OF_MEMORY_ERROR;
    }
    double *R = (double *)base;
    int32_t *list = (int32_t *)(base + (needR ? sizeof(double) * (size_t)slice * m : 0));
    LossArgs A;
    A.kind = c->kind; A.shared_scale = c->shared_scale; A.scale = c->dscale;
    for (int q0 = 0; q0 < npoints; q0 += slice) {
        const int cnt = std::min(slice, npoints - q0);
        const int32_t *lp = dprob ? dprob + q0 : list;
        if (!dprob) hipLaunchKernelGGL(k_loss_iota, dim3((cnt + 255) / 256), dim3(256), 0, s, cnt, q0, list);
        A.dprob = lp;
        const double *Xs = dX + (size_t)q0 * n;
        int rc;
        if (!jac) {
            double *F = out + (size_t)q0 * m;
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, F))) return rc;
            if (!lin) hipLaunchKernelGGL(k_loss_fcn, dim3((unsigned)(((size_t)cnt * m + 255) / 256)), dim3(256), 0, s, A, m, cnt, F);
        } else {
            double *J = out + (size_t)q0 * m * n;
            if (!lin && (rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, R))) return rc;
            if ((rc = c->jac(c->inner, hip_stream, cnt, lp, n, Xs, m, J))) return rc;
            if (!lin) loss_launch_jac(c, A, m, n, cnt, R, J, s);
        }
    }
    return 0;
}

int nlh_loss_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return loss_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_loss_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return loss_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

int nlh_loss_apply_batch(nlh_handle *h, int32_t kind, int32_t nprob, int32_t m, const double *dscale, int32_t shared_scale, const double *dr,
                         double *dout, double *dg, double *dwgt)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!nlh_loss_kind_ok(kind) || nprob < 0 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)nprob * m + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0 || (!dout && !dg && !dwgt)) return 0;
    if (!dr || (kind != NLH_LOSS_LINEAR && !dscale)) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    LossArgs A;
    A.kind = kind; A.shared_scale = shared_scale != 0; A.scale = dscale; A.dprob = nullptr;
    hipLaunchKernelGGL(k_loss_apply, dim3((unsigned)(((size_t)nprob * m + 255) / 256)), dim3(256), 0, h->stream, A, m, nprob, dr, dout, dg, dwgt);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fit + errors with a loss: the loss wraps the model's launchers, the map, if any, wraps the result
// ---------------------------------------------------------------------------------------------------------------------
static int fit_compose_loss(nlh_handle *h, const nlh_options *opts, const nlh_pmap *pm, int32_t kind, const double *dscale,
                            int32_t shared_scale, int32_t nprob, int32_t m, int32_t N, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *ctx,
                            const std::function<void(int32_t)> &at, const double *dw, const double *xl, const double *xu, double *dx,
                            double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                            int32_t *status)
{
    nlh_loss_ctx *lc = nullptr;
    int rc = nlh_loss_wrap(h, kind, dscale, shared_scale, fcn, jac, ctx, &lc);
    if (rc) return rc;
    auto at_run = [&](int32_t p0) {                               // a run of problems counts its dprob from its first one
        at(p0);
        lc->dscale = shared_scale ? dscale : dscale + p0;
    };
    nlh_device_jacfcn lj = jac ? nlh_loss_device_jac : nullptr;
    if (pm)
        rc = nlh_fit_compose_pmap(h, opts, pm, nprob, m, nlh_loss_device_fcn, lj, lc, at_run, dw, xl, xu, dx, dfvec, dsigma, dcov, dchi2, drank,
                                  ib, status);
    else
        rc = nlh_fit_compose(h, opts, nprob, m, N, nlh_loss_device_fcn, lj, lc, at_run, dw, xl, xu, dx, dfvec, dsigma, dcov, dchi2, drank, ib,
                             status);
    const hipError_t e = hipStreamSynchronize(h->stream);         // (the context's scratch goes)
    nlh_loss_unwrap(lc);
    if (!rc && e != hipSuccess) {
        h->err = std::string("fit with a loss: ") + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return rc;
}

// the checks the four entry points make after the handle's, in the documented order: the model (N < 0: none), the map, the
// degrees of freedom over the free unknowns, the kind of loss
static int loss_fit_check(int32_t N, int32_t nprob, int32_t m, const nlh_pmap *pm, int32_t loss, int32_t *nfree)
{
    if (N < 0 || nprob < 0 || m < 1) return NLH_INVALID_INPUT_ERROR;
    *nfree = N;
    if (pm) {
        int32_t nf;
        nlh_pmap_shape(pm, &nf, nfree, nullptr);
        if (nf != N) return NLH_INVALID_INPUT_ERROR;
    }
    if (m < *nfree) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    return nlh_loss_kind_ok(loss) ? 0 : NLH_INVALID_INPUT_ERROR;
}

int nlh_curve_fit_batch_loss(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                             const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                             const double *xu, const nlh_pmap *pm, int32_t loss, const double *dscale, int32_t shared_scale, double *dx,
                             double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib,
                             int32_t *status)
{
    if (loss == NLH_LOSS_LINEAR)
        return nlh_curve_fit_batch_pmap(h, opts, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, pm, dx, dfvec, dsigma,
                                        dcov, dchi2, drank, ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    int32_t nfree;
    const int32_t N = nlh_curve_nparams(kind, ncomp, nbase);
    if (const int rc = loss_fit_check(N, nprob, m, pm, loss, &nfree)) return rc;
    if (nprob == 0) return 0;
    if (!opts || !dt || !dy || !dx || !dfvec || !dscale) return NLH_INVALID_INPUT_ERROR;
    nlh_curve_ctx c;
    c.kind = kind; c.ncomp = ncomp; c.nbase = nbase; c.shared_t = shared_t != 0; c.m = m;
    auto at = [&](int32_t p0) {
        c.dt = shared_t ? dt : dt + (size_t)p0 * m;
        c.dy = dy + (size_t)p0 * m;
        c.dw = dw ? dw + (size_t)p0 * m : nullptr;
    };
    return fit_compose_loss(h, opts, pm, loss, dscale, shared_scale, nprob, m, N, nlh_curve_device_fcn, analytic ? nlh_curve_device_jac : nullptr,
                            &c, at, dw, xl, xu, dx, dfvec, dsigma, dcov, dchi2, drank, ib, status);
}

int nlh_expr_fit_batch_loss(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                            const nlh_pmap *pm, int32_t loss, const double *dscale, int32_t shared_scale, double *dx, double *dfvec,
                            double *dsigma, double *dcov, double *dchi2, int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    if (loss == NLH_LOSS_LINEAR)
        return nlh_expr_fit_batch_pmap(h, opts, e, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, pm, dx, dfvec, dsigma, dcov, dchi2, drank,
                                       ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    int32_t nfree;
    const int32_t N = e ? e->prog.nparams : -1;
    if (const int rc = loss_fit_check(N, nprob, m, pm, loss, &nfree)) return rc;
    if (nprob == 0) return 0;
    if (!opts || !dt || !dy || !dx || !dfvec || !dscale) return NLH_INVALID_INPUT_ERROR;
    nlh_expr_ctx c;
    c.e = e; c.shared_t = shared_t != 0; c.m = m;
    c.dt_stride = shared_t ? (int64_t)m : (int64_t)nprob * m;      // (a run of problems keeps the whole batch's stride)
    auto at = [&](int32_t p0) {
        c.dt = shared_t ? dt : dt + (size_t)p0 * m;
        c.dy = dy + (size_t)p0 * m;
        c.dw = dw ? dw + (size_t)p0 * m : nullptr;
    };
    return fit_compose_loss(h, opts, pm, loss, dscale, shared_scale, nprob, m, N, nlh_expr_device_fcn, analytic ? nlh_expr_device_jac : nullptr,
                            &c, at, dw, xl, xu, dx, dfvec, dsigma, dcov, dchi2, drank, ib, status);
}

// ... behind host arrays: the scales are checked here (finite, positive) and get a device copy, the caller's to hipFree
// (nlh_internal.h: the model object uses it too)
int nlh_loss_scale_upload(nlh_handle *h, int32_t loss, const double *scale, size_t cnt, double **dscale)
{
    *dscale = nullptr;
    if (!nlh_loss_scale_ok(loss, scale, cnt)) return NLH_INVALID_INPUT_ERROR;
    if (loss == NLH_LOSS_LINEAR) return 0;                        // reads no scale
    if (hipSetDevice(h->device) != hipSuccess) return NLH_ERR_HIP;
    if (hipMalloc(dscale, sizeof(double) * cnt) != hipSuccess) {
        h->err = "hipMalloc (the scales of a loss)";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    hipError_t e = hipMemcpyAsync(*dscale, scale, sizeof(double) * cnt, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        hipFree(*dscale);
        *dscale = nullptr;
        h->err = std::string("hipMemcpy (the scales of a loss): ") + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return 0;
}

int nlh_curve_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                               const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                               const double *xu, const nlh_pmap *pm, int32_t loss, const double *scale, int32_t shared_scale, double *x,
                               double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib,
                               int32_t *status)
{
    if (loss == NLH_LOSS_LINEAR)
        return nlh_curve_fit_batch_pmap_h(h, opts, kind, ncomp, nbase, nprob, m, t, shared_t, y, w, analytic, xl, xu, pm, x, fvec, sigma, cov,
                                          chi2, rank, ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    int32_t nfree;
    const int32_t N = nlh_curve_nparams(kind, ncomp, nbase);
    if (const int rc = loss_fit_check(N, nprob, m, pm, loss, &nfree)) return rc;
    if (nprob == 0) return 0;
    if (!opts || !t || !y || !x || !fvec) return NLH_INVALID_INPUT_ERROR;
    double *dscale = nullptr;
    int rc = nlh_loss_scale_upload(h, loss, scale, shared_scale ? 1 : (size_t)nprob, &dscale);
    if (rc) return rc;
    rc = nlh_fit_compose_h(h, "curve fit", shared_t ? (size_t)m : (size_t)nprob * m, nprob, m, N, t, y, w, x, fvec, sigma, cov, chi2, rank,
                           [&](const double *dt, const double *dy, const double *dw, double *dx, double *df, double *ds, double *dc, double *dq,
                               int32_t *dr) {
                               return nlh_curve_fit_batch_loss(h, opts, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, pm,
                                                               loss, dscale, shared_scale, dx, df, ds, dc, dq, dr, ib, status);
                           }, nfree);
    (void)hipFree(dscale);
    return rc;
}

int nlh_expr_fit_batch_loss_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                              const nlh_pmap *pm, int32_t loss, const double *scale, int32_t shared_scale, double *x, double *fvec,
                              double *sigma, double *cov, double *chi2, int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    if (loss == NLH_LOSS_LINEAR)
        return nlh_expr_fit_batch_pmap_h(h, opts, e, nprob, m, t, shared_t, y, w, analytic, xl, xu, pm, x, fvec, sigma, cov, chi2, rank, ib,
                                         status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    int32_t nfree;
    const int32_t N = e ? e->prog.nparams : -1;
    if (const int rc = loss_fit_check(N, nprob, m, pm, loss, &nfree)) return rc;
    if (nprob == 0) return 0;
    if (!opts || !t || !y || !x || !fvec) return NLH_INVALID_INPUT_ERROR;
    double *dscale = nullptr;
    int rc = nlh_loss_scale_upload(h, loss, scale, shared_scale ? 1 : (size_t)nprob, &dscale);
    if (rc) return rc;
    const size_t tm = (size_t)e->prog.nvar * (shared_t ? (size_t)m : (size_t)nprob * m);
    rc = nlh_fit_compose_h(h, "formula fit", tm, nprob, m, N, t, y, w, x, fvec, sigma, cov, chi2, rank,
                           [&](const double *dt, const double *dy, const double *dw, double *dx, double *df, double *ds, double *dc, double *dq,
                               int32_t *dr) {
                               return nlh_expr_fit_batch_loss(h, opts, e, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, pm, loss, dscale,
                                                              shared_scale, dx, df, ds, dc, dq, dr, ib, status);
                           }, nfree);
    (void)hipFree(dscale);
    return rc;
}
