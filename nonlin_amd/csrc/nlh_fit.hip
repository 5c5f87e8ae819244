// nlh_fit.hip -- the one-call fit + errors pipeline behind the entry points
// nlh_{curve,expr}_fit_batch{,_pmap,_loss,_pois,_group,_conv,_sep}{,_h} (nlh_internal.h: nlh_fit_run).  A model kind hands it a
// FitSource -- its launchers, a context and how to point that context at a run of problems -- and the rest of the entry point's arguments as a FitArgs; here are the documented ladder of checks,
// the staging of host arrays, the composition (the loss wraps the model's launchers, the parameter map, if any, wraps the
// result), the solve and covariance of every run of consecutive problems that have degrees of freedom, and the rule of
// zero-weight padding.  A Poisson fit (FitArgs::stat) puts the Poisson wrapper where the loss sits, around a model bound
// without weights: w is then the wrapper's 0 / 1 mask, the covariance is unscaled and chi2 is the deviance over the degrees
// of freedom.  An instrument response (FitArgs::cv) puts the convolving pair innermost, around a model bound without weights.
// Nothing here knows what a curve or a formula is.  Kernels: nlh_kernels_fit.h.
#include "nlh_internal.h"
#include "nlh_kernels_fit.h"

namespace {
// The launchers a solve sees -- the model's, inside the loss's, inside the map's -- and what each run of consecutive
// problems re-points: a run counts its dprob from its first problem.
struct FitRun {
    nlh_handle *h;
    const nlh_options *opts;
    const FitSource *src;
    const FitArgs *a;                  // device pointers
    int32_t N;                         // the model's parameters
    nlh_device_vecfcn fcn;
    nlh_device_jacfcn jac;
    void *ctx;
    nlh_loss_ctx *lc = nullptr;
    nlh_pois_ctx *qc = nullptr;
    nlh_pmap_ctx *pc = nullptr;
    nlh_conv_ctx *cc = nullptr;        // an instrument response: innermost, around the model's launchers
    const double *fullc = nullptr;     // the map's private copy of the full parameters
    // a separable fit: the solve runs over the nonlinear unknowns (of a group: the outer ones of the reduced group) through the
    // projecting pair; after each run `full` turns the solved unknowns into the caller's full parameters and hands back where
    // the unknowns of the errors lie; the errors and the degrees of freedom are those of the unprojected pair (ifcn, ijac, ictx)
    // over its ne unknowns
    std::function<int(int32_t p0, int32_t cnt, const double *solved, double **xerr)> full;
    nlh_device_vecfcn ifcn = nullptr;
    nlh_device_jacfcn ijac = nullptr;
    void *ictx = nullptr;
    int32_t ne = 0;
    int32_t G = 1;                     // a global fit: a problem of the solve is G of the model's, a->m its G m rows
    void bind(int32_t p0) const
    {
        src->bind(src->ctx, a->t, a->y, qc || cc ? nullptr : a->w, p0 * G);
        if (cc) {                                                 // (its weights: none under the Poisson pair, which keeps the mask)
            const size_t at = (size_t)p0 * a->m;
            conv_ctx_rebind(cc, a->y + at, a->w && !qc ? a->w + at : nullptr,
                            a->cv->shared_k ? a->cv->k : a->cv->k + (size_t)p0 * G * a->cv->L);
        }
        if (qc) pois_ctx_rebind(qc, a->y + (size_t)p0 * a->m, a->w ? a->w + (size_t)p0 * a->m : nullptr);
        if (lc) loss_ctx_rebind(lc, a->shared_scale ? a->scale : a->scale + (size_t)p0 * G);
        if (pc) pmap_ctx_rebind(pc, fullc + (size_t)p0 * N);
    }
};

// run() inside a layer -- the context an nlh_*_wrap just made around r's launchers --: the stream is synchronised (the
// context's scratch goes), the layer released, and a HIP error becomes NLH_ERR_HIP with `label` in h->err unless run's own
// return code is not 0, which wins.
template <class Run> int in_layer(nlh_handle *h, void *layer, const char *label, Run &&run)
{
    const int rc = run();
    const hipError_t e = hipStreamSynchronize(h->stream);
    wrap_release(wrap_layer(layer));
    if (!rc && e != hipSuccess) {
        h->err = std::string(label) + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return rc;
}

// The end of a fit through a map or a group: the stream is synchronised (st is a host vector; the buffers go), the layer
// (NULL: none was made) and base released, and a HIP error -- e, then the synchronisation's -- wins over rc; the status comes
// back when rc is 0.
int mapped_end(nlh_handle *h, void *layer, void *base, const char *label, int rc, hipError_t e, const std::vector<int32_t> &st,
               int32_t *status)
{
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    wrap_release(wrap_layer(layer));
    (void)hipFree(base);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        h->err = std::string(label) + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    if (!rc && status) memcpy(status, st.data(), sizeof(int32_t) * st.size());
    return rc;
}

// The box of a solve over nu unknowns: the caller's xl / xu, which are per parameter of the model, carried to the unknowns.
// at(g, k) for k < K of each of G sets: {u, p}, unknown u is parameter p.  A bound the caller did not give stays NULL.
struct FitBox {
    std::vector<double> lo, hi;
    const double *xl() const { return lo.empty() ? nullptr : lo.data(); }
    const double *xu() const { return hi.empty() ? nullptr : hi.data(); }
};
template <class At> FitBox fit_box(const FitArgs &a, int32_t nu, int32_t G, int32_t K, At &&at)
{
    FitBox b;
    if (a.xl) b.lo.resize(nu);
    if (a.xu) b.hi.resize(nu);
    for (int32_t g = 0; g < G; ++g)
        for (int32_t k = 0; k < K; ++k) {
            const std::pair<int32_t, int32_t> up = at(g, k);
            if (a.xl) b.lo[up.first] = a.xl[up.second];
            if (a.xu) b.hi[up.first] = a.xu[up.second];
        }
    return b;
}
}   // namespace

// Solve (bounded when xl or xu is given), covariance with scaled = 1 (a Poisson fit: 0) when any of dsigma, dcov, the caller's chi2 is asked for,
// the degrees-of-freedom rule of zero weights, NaN and rank -1 for problems that did not solve: over n unknowns -- the
// model's parameters, or the free ones of a map, whose arrays xl .. status these then are.
static int fit_solve(const FitRun &r, int32_t n, const double *xl, const double *xu, double *dx, double *dsigma, double *dcov, int32_t *status)
{
    nlh_handle *h = r.h;
    const FitArgs &a = *r.a;
    const int32_t nprob = a.nprob, m = a.m;
    const double *dw = a.w;
    double *dfvec = a.fvec, *dchi2 = a.chi2;
    int32_t *drank = a.rank;
    nlh_iteration_behavior *ib = a.ib;
    int rc;
    const bool errors = dsigma || dcov || dchi2;
    const bool pois = a.stat == NLH_STAT_POISSON;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int32_t ne = r.full ? r.ne : n;                        // the unknowns of the errors and of the degrees of freedom
    const size_t np = (size_t)nprob, nn = (size_t)ne * ne;
    // the handle's own buffer for this entry point: status and non-zero-weight counts, a cov when the caller wants none
    const size_t ints = 2 * np + 2;
    if ((rc = ensure(h, h->crv, sizeof(int32_t) * ints + sizeof(double) * (errors && !dcov ? np * nn : 0) + 64))) return rc;
    int32_t *dstat = (int32_t *)h->crv.p, *dnz = dstat + np;
    double *cov = dcov ? dcov : (double *)(dstat + (ints & ~(size_t)1));
    std::vector<int32_t> st(np, 0), nz;
    if (dw) {                                                    // degrees of freedom, before anything is evaluated
        nz.resize(np);
        hipLaunchKernelGGL(k_fit_count, dim3((nprob + 63) / 64), dim3(64), 0, s, nprob, m, dw, dnz);
        HIPCHK(h, hipMemcpyAsync(nz.data(), dnz, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (size_t p = 0; p < np; ++p)
            if (nz[p] - ne <= 0) st[p] = NLH_INVALID_INPUT_ERROR;
    }
    // runs of consecutive problems that have degrees of freedom (all of them, as a rule): exactly the calls a user makes
    for (int32_t p0 = 0; p0 < nprob;) {
        if (st[p0]) { ++p0; continue; }
        int32_t p1 = p0;
        while (p1 < nprob && !st[p1]) ++p1;
        const int32_t cnt = p1 - p0;
        r.bind(p0);
        double *xs = dx + (size_t)p0 * n, *fs = dfvec + (size_t)p0 * m;
        nlh_iteration_behavior *ibs = ib ? ib + p0 : nullptr;
        if (xl || xu) rc = nlh_cls_solve_batch_device(h, r.opts, 1.0, 1.0, xl, xu, cnt, m, n, r.fcn, r.jac, r.ctx, xs, fs, ibs, &st[p0]);
        else rc = nlh_lm_solve_batch_device(h, r.opts, cnt, m, n, r.fcn, r.jac, r.ctx, xs, fs, ibs, &st[p0]);
        if (rc) return rc;
        if (r.full && (rc = r.full(p0, cnt, xs, &xs))) return rc;  // the full parameters of the solution, for the caller and the errors
        if (errors &&
            (rc = nlh_lm_covariance_batch_device(h, cnt, m, ne, r.full ? r.ifcn : r.fcn, r.full ? r.ijac : r.jac, r.full ? r.ictx : r.ctx, xs,
                                                 pois ? 0 : 1, 0.0, cov + (size_t)p0 * nn, dsigma ? dsigma + (size_t)p0 * ne : nullptr,
                                                 drank ? drank + p0 : nullptr, dchi2 ? dchi2 + p0 : nullptr))) return rc;
        p0 = p1;
    }
    if (errors) {
        HIPCHK(h, hipMemcpyAsync(dstat, st.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fit_post, dim3((nprob + 63) / 64), dim3(64), 0, s, nprob, m, ne, (const int32_t *)dstat,
                           dw ? (const int32_t *)dnz : (const int32_t *)nullptr, (const double *)dfvec, cov, dsigma, dchi2, drank, pois ? 1 : 0);
        HIPCHK(h, hipStreamSynchronize(s));                      // (st is a host vector)
    }
    if (status) memcpy(status, st.data(), sizeof(int32_t) * np);
    if (ib)
        for (size_t p = 0; p < np; ++p)
            if (st[p] == NLH_INVALID_INPUT_ERROR && nz.size() && nz[p] - ne <= 0) ib[p] = nlh_iteration_behavior{};
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ... through a parameter map: fit_solve over the n free unknowns with the map's launchers around r's, between a gather and
// an expansion; every array of the caller's has the map's full size.
static int fit_mapped(FitRun r, int32_t n)
{
    nlh_handle *h = r.h;
    const FitArgs &a = *r.a;
    const size_t N = (size_t)r.N, nf = (size_t)n, np = (size_t)a.nprob;
    if ((np * (a.cov ? N * N : N) + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc = 0;
    // a private copy of the full parameters (the fixed values), the free unknowns, the free sigma and cov, the failure flags
    const size_t doubles = np * N + np * nf + (a.sigma ? np * nf : 0) + (a.cov ? np * nf * nf : 0);
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * doubles + sizeof(int32_t) * np) != hipSuccess) {
        h->err = "hipMalloc (fit through a parameter map)";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    double *q = base;
    double *fullc = q; q += np * N;
    double *xf = q; q += np * nf;
    double *sf = a.sigma ? q : nullptr; q += a.sigma ? np * nf : 0;
    double *cf = a.cov ? q : nullptr; q += a.cov ? np * nf * nf : 0;
    int32_t *dfail = (int32_t *)q;
    std::vector<int32_t> f2f(nf);
    nlh_pmap_tables(a.pm, nullptr, nullptr, nullptr, nullptr, f2f.data());
    const FitBox box = fit_box(a, n, 1, n, [&](int32_t, int32_t j) { return std::make_pair(j, f2f[j]); });
    std::vector<int32_t> st(np, 0);
    nlh_pmap_ctx *pc = nullptr;                                   // its copy of the tables serves the steps here too
    hipError_t e = hipSuccess;
    rc = nlh_pmap_wrap(h, a.pm, r.fcn, r.jac, r.ctx, fullc, 0, &pc);
    if (!rc) e = hipMemcpyAsync(fullc, a.x, sizeof(double) * np * N, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && !rc) {
        pmap_gather(pmap_ctx_tables(pc), s, a.nprob, fullc, xf);
        r.fcn = nlh_pmap_device_fcn; r.jac = r.jac ? nlh_pmap_device_jac : nullptr; r.ctx = pc;
        r.pc = pc; r.fullc = fullc;
        rc = fit_solve(r, n, box.xl(), box.xu(), xf, sf, cf, st.data());
    }
    if (e == hipSuccess && !rc) {
        // every problem, also one that was refused on its degrees of freedom and kept its x: on exit x obeys the map
        pmap_expand(pmap_ctx_tables(pc), s, a.nprob, xf, fullc, 0, a.x);
        if (a.sigma || a.cov) {
            e = hipMemcpyAsync(dfail, st.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) pmap_cov(pmap_ctx_tables(pc), s, a.nprob, cf, sf, dfail, a.cov, a.sigma);
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    return mapped_end(h, pc, base, "fit through a parameter map: ", rc, e, st, a.status);
}

// ... of groups: fit_solve over the n outer unknowns of ngroup problems of M = G m rows with the group's launchers around r's,
// between a gather and an expansion.  y, w and fvec are the caller's as they stand; x and sigma are per data set on the
// caller's side and per group in between; cov, chi2, rank, ib and status are per group on both.
static int fit_grouped(FitRun r, int32_t n)
{
    nlh_handle *h = r.h;
    const FitArgs &a = *r.a;
    int32_t G;
    nlh_group_shape(a.grp, nullptr, nullptr, &G, nullptr);
    const int32_t ngroup = a.nprob / G;
    const size_t N = (size_t)r.N, nf = (size_t)n, ng = (size_t)ngroup;
    if ((ng * std::max(nf, (size_t)G * N) + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc = 0;
    const size_t doubles = ng * nf + (a.sigma ? ng * nf : 0);    // the outer unknowns, their sigma; the failure flags
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * doubles + sizeof(int32_t) * ng) != hipSuccess) {
        h->err = "hipMalloc (global fit)";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    double *xo = base, *so = a.sigma ? base + ng * nf : nullptr;
    int32_t *dfail = (int32_t *)(base + doubles);
    // the bounds of parameter k at every outer unknown of k
    const FitBox box = fit_box(a, n, G, r.N, [&](int32_t g, int32_t k) { return std::make_pair(nlh_group_index(a.grp, g, k), k); });
    FitArgs ga = a;                                               // what the solve sees: ngroup problems of G m rows
    ga.nprob = ngroup; ga.m = G * a.m;
    std::vector<int32_t> st(ng, 0);
    nlh_group_ctx *gc = nullptr;                                  // its copy of the tables serves the steps here too
    hipError_t e = hipSuccess;
    rc = nlh_group_wrap(h, a.grp, r.fcn, r.jac, r.ctx, &gc);
    if (!rc) {
        group_gather(group_ctx_tables(gc), s, ngroup, a.x, xo);
        r.fcn = nlh_group_device_fcn; r.jac = r.jac ? nlh_group_device_jac : nullptr; r.ctx = gc;
        r.a = &ga; r.G = G;
        rc = fit_solve(r, n, box.xl(), box.xu(), xo, so, a.cov, st.data());
    }
    if (!rc) {
        // every group, also one that was refused on its degrees of freedom: on exit a shared parameter is equal across it
        group_expand(group_ctx_tables(gc), s, ngroup, xo, nullptr, a.x);
        if (a.sigma) {
            e = hipMemcpyAsync(dfail, st.data(), sizeof(int32_t) * ng, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) group_expand(group_ctx_tables(gc), s, ngroup, so, dfail, a.sigma);
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    return mapped_end(h, gc, base, "global fit: ", rc, e, st, a.status);
}

// ... of a separable model: fit_solve over the n = N - L nonlinear unknowns with the projecting launchers around r's pair,
// whose Jacobian launcher is given whatever `analytic` says -- its linear columns are the basis --; analytic chooses the outer
// Jacobian (the projected one, or forward differences over the nonlinear unknowns) and the Jacobian of the errors.  The
// caller's arrays are the model's: x is gathered on entry and solved for on exit, problem by problem as they are solved (one
// that is refused on its degrees of freedom keeps its x); sigma, cov, chi2 and rank are the inner pair's at the full solution.
// With a group -- declared over the model's N parameters, its shared ones all nonlinear -- the group of the same shared
// parameters over the n nonlinear ones wraps the projecting pair, and the errors are those of the caller's group around the
// unprojected pair at the full solution: what the _group entry point reports there.
static int fit_separated(FitRun r, bool analytic)
{
    nlh_handle *h = r.h;
    const FitArgs &a = *r.a;
    int32_t n;
    nlh_sep_shape(a.sp, nullptr, nullptr, &n);
    const int32_t N = r.N, m = a.m;
    const size_t np = (size_t)a.nprob;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    std::vector<int32_t> nl(n);
    nlh_sep_tables(a.sp, nullptr, nl.data());
    int32_t G = 1, S = 0, no = n, nof = N;                        // a group: its sets, shared parameters, outer unknowns reduced and full
    nlh_group *gred = nullptr;
    if (a.grp) {
        nlh_group_shape(a.grp, nullptr, &S, &G, &nof);
        std::vector<int32_t> sh;
        for (int32_t j = 0; j < n; ++j)
            if (nlh_group_index(a.grp, 0, nl[j]) < S) sh.push_back(j);
        if (const int rc = nlh_group_create(n, (int32_t)sh.size(), sh.data(), G, &gred)) return rc;
        nlh_group_shape(gred, nullptr, nullptr, nullptr, &no);
    }
    const int32_t nsolve = a.nprob / G;
    const size_t ns = (size_t)nsolve;
    // the bounds of the nonlinear parameters at the unknowns of the solve
    const FitBox box = fit_box(a, no, G, n, [&](int32_t g, int32_t j) { return std::make_pair(gred ? nlh_group_index(gred, g, j) : j, nl[j]); });
    // the handle's buffer: alpha [nprob][n], and of a group the unknowns of the solve, those of the errors, their sigma, the flags
    const size_t doubles = np * n + (gred ? ns * no + ns * nof + (a.sigma ? ns * nof : 0) : 0);
    int rc = ensure(h, h->sepx, sizeof(double) * doubles + sizeof(int32_t) * ns + 64);
    if (rc) { nlh_group_destroy(gred); return rc; }
    double *alpha = (double *)h->sepx.p, *xo = alpha + np * n, *xof = xo + (gred ? ns * no : 0), *so = xof + (gred ? ns * nof : 0);
    int32_t *dfail = (int32_t *)(alpha + doubles);
    nlh_sep_ctx *sc = nullptr;
    nlh_group_ctx *gc = nullptr, *gcf = nullptr;                  // the reduced group around the projecting pair; the caller's around r's
    FitArgs ga = a;                                               // what the solve sees: nsolve problems of G m rows
    ga.nprob = nsolve; ga.m = G * m;
    std::vector<int32_t> st(ns, 0);
    const nlh_device_vecfcn fcn = r.fcn;
    const nlh_device_jacfcn jac = r.jac;
    void *const ctx = r.ctx;
    rc = nlh_sep_wrap(h, a.sp, fcn, jac, ctx, &sc);
    if (!rc) rc = nlh_sep_gather_batch(h, a.sp, a.nprob, a.x, alpha);
    if (!rc && gred) rc = nlh_group_wrap(h, gred, nlh_sep_device_fcn, analytic ? nlh_sep_device_jac : nullptr, sc, &gc);
    if (!rc && gred) rc = nlh_group_wrap(h, a.grp, fcn, analytic ? jac : nullptr, ctx, &gcf);
    if (!rc && gred) rc = nlh_group_gather_batch(h, gred, nsolve, alpha, xo);
    if (!rc) {
        r.ifcn = gred ? nlh_group_device_fcn : fcn;
        r.ijac = !analytic ? nullptr : gred ? nlh_group_device_jac : jac;
        r.ictx = gred ? (void *)gcf : ctx;
        r.ne = nof;
        r.fcn = gred ? nlh_group_device_fcn : nlh_sep_device_fcn;
        r.jac = !analytic ? nullptr : gred ? nlh_group_device_jac : nlh_sep_device_jac;
        r.ctx = gred ? (void *)gc : (void *)sc;
        r.a = &ga; r.G = G;
        r.full = [&](int32_t p0, int32_t cnt, const double *solved, double **xerr) -> int {
            double *al = alpha + (size_t)p0 * G * n, *xf = a.x + (size_t)p0 * G * N;
            int e = 0;
            if (gred && (e = nlh_group_expand_batch(h, gred, cnt, solved, al))) return e;
            if ((e = nlh_sep_solve_batch(h, sc, cnt * G, m, gred ? al : solved, xf, nullptr))) return e;
            *xerr = xf;
            if (!gred) return 0;
            *xerr = xof + (size_t)p0 * nof;
            return nlh_group_gather_batch(h, a.grp, cnt, xf, *xerr);
        };
        rc = fit_solve(r, no, box.xl(), box.xu(), gred ? xo : alpha, gred ? (a.sigma ? so : nullptr) : a.sigma, a.cov, st.data());
    }
    hipError_t e = hipSuccess;
    if (!rc && gred && a.sigma) {                                 // sigma per data set, NaN for a group that did not solve
        e = hipMemcpyAsync(dfail, st.data(), sizeof(int32_t) * ns, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) rc = nlh_group_sigma_batch(h, a.grp, nsolve, so, dfail, a.sigma);
    }
    const hipError_t e2 = hipStreamSynchronize(s);                // (st is a host vector; the contexts' scratch goes)
    nlh_group_unwrap(gc);
    nlh_group_unwrap(gcf);
    nlh_sep_unwrap(sc);
    nlh_group_destroy(gred);
    if (e == hipSuccess) e = e2;
    if (!rc && e != hipSuccess) {
        h->err = std::string("separable fit: ") + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    if (!rc && a.status) memcpy(a.status, st.data(), sizeof(int32_t) * ns);
    return rc;
}

// The composition on device pointers: the loss wraps r's launchers -- the model's, or the convolved model's -- (NLH_LOSS_LINEAR:
// no context, no kernel of the loss) -- in a Poisson fit the Poisson wrapper does, in the same place --, the map or the group,
// if any, wraps the result.  n: the unknowns of the solve.
static int fit_composed(nlh_handle *h, FitRun &r, const FitArgs &a, int32_t n)
{
    const nlh_device_vecfcn fcn = r.fcn;
    const nlh_device_jacfcn jac = r.jac;
    void *const ctx = r.ctx;
    auto run = [&]() {
        return a.sp ? fit_separated(r, r.src->jac != nullptr) : a.grp ? fit_grouped(r, n) : a.pm ? fit_mapped(r, n)
                                                                          : fit_solve(r, n, a.xl, a.xu, a.x, a.sigma, a.cov, a.status);
    };
    if (a.stat == NLH_STAT_POISSON) {
        if (const int rc = nlh_pois_wrap(h, a.y, a.w, a.mu_floor, fcn, jac, ctx, &r.qc)) return rc;
        r.fcn = nlh_pois_device_fcn; r.jac = jac ? nlh_pois_device_jac : nullptr; r.ctx = r.qc;
        return in_layer(h, r.qc, "Poisson fit: ", run);
    }
    if (a.loss == NLH_LOSS_LINEAR) return run();
    if (const int rc = nlh_loss_wrap(h, a.loss, a.scale, a.shared_scale, fcn, jac, ctx, &r.lc)) return rc;
    r.fcn = nlh_loss_device_fcn; r.jac = jac ? nlh_loss_device_jac : nullptr; r.ctx = r.lc;
    return in_layer(h, r.lc, "fit with a loss: ", run);
}

// ... with an instrument response (FitArgs::cv) first: the convolving pair wraps the model's launchers, the model bound
// without weights; w is the convolving pair's, unless a Poisson pair follows, which keeps it as its mask.
static int fit_device(nlh_handle *h, const nlh_options *opts, const FitSource &src, const FitArgs &a, int32_t n)
{
    // (a separable fit needs the model's Jacobian launcher whatever `analytic` says: a.sp_jac; src.jac keeps saying which)
    const nlh_device_jacfcn mjac = a.sp ? a.sp_jac : src.jac;
    FitRun r{h, opts, &src, &a, src.N, src.fcn, mjac, src.ctx};
    if (!a.cv) return fit_composed(h, r, a, n);
    if (const int rc = nlh_conv_wrap(h, a.cv, a.y, a.stat == NLH_STAT_POISSON ? nullptr : a.w, src.fcn, mjac, src.ctx, &r.cc)) return rc;
    r.fcn = nlh_conv_device_fcn; r.jac = mjac ? nlh_conv_device_jac : nullptr; r.ctx = r.cc;
    return in_layer(h, r.cc, "fit with an instrument response: ", [&]() { return fit_composed(h, r, a, n); });
}

// ... behind HOST arrays t, y, w, x, fvec, sigma, cov, chi2, rank (and the scales, which dscale is the device copy of): one
// allocation, the copies in, fit_device, the copies out.
static int fit_staged(nlh_handle *h, const nlh_options *opts, const FitSource &src, const FitArgs &a, int32_t n, const double *dscale)
{
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t N = (size_t)src.N, np = (size_t)a.nprob, pm = np * a.m;
    size_t nq = np, nn = N * N;                                   // problems of the solve and the doubles of one's cov: a global fit's
    if (a.grp) {                                                  // are per group and over the outer unknowns
        int32_t G;
        nlh_group_shape(a.grp, nullptr, nullptr, &G, nullptr);
        nq = np / G; nn = (size_t)n * n;
    }
    const size_t tm = src.tdoubles * (a.shared_t ? (size_t)a.m : pm);
    const size_t kd = a.cv ? (size_t)a.cv->L * (a.cv->shared_k ? 1 : np) : 0;      // the taps of an instrument response
    const size_t doubles = tm + pm * (a.w ? 3 : 2) + np * N + (a.sigma ? np * N : 0) + (a.cov ? nq * nn : 0) + (a.chi2 ? nq : 0) + kd;
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * doubles + sizeof(int32_t) * nq) != hipSuccess) {
        h->err = std::string("hipMalloc (") + src.what + ")";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    FitArgs d = a;
    double *q = base;
    double *dt = q; q += tm;
    double *dy = q; q += pm;
    double *dw = a.w ? q : nullptr; q += a.w ? pm : 0;
    d.fvec = q; q += pm;
    d.x = q; q += np * N;
    d.sigma = a.sigma ? q : nullptr; q += a.sigma ? np * N : 0;
    d.cov = a.cov ? q : nullptr; q += a.cov ? nq * nn : 0;
    d.chi2 = a.chi2 ? q : nullptr; q += a.chi2 ? nq : 0;
    double *dk = q; q += kd;
    d.rank = a.rank ? (int32_t *)q : nullptr;
    d.t = dt; d.y = dy; d.w = dw; d.scale = dscale;
    nlh_conv dcv{};
    if (a.cv) { dcv = *a.cv; dcv.k = dk; d.cv = &dcv; }
    hipError_t e = hipMemcpyAsync(dt, a.t, sizeof(double) * tm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(dy, a.y, sizeof(double) * pm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && a.w) e = hipMemcpyAsync(dw, a.w, sizeof(double) * pm, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d.x, a.x, sizeof(double) * np * N, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && a.cv) e = hipMemcpyAsync(dk, a.cv->k, sizeof(double) * kd, hipMemcpyHostToDevice, s);
    int rc = 0;
    if (e == hipSuccess) rc = fit_device(h, opts, src, d, n);
    if (e == hipSuccess && !rc) {
        e = hipMemcpyAsync(a.x, d.x, sizeof(double) * np * N, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(a.fvec, d.fvec, sizeof(double) * pm, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && a.sigma) e = hipMemcpyAsync(a.sigma, d.sigma, sizeof(double) * np * N, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && a.cov) e = hipMemcpyAsync(a.cov, d.cov, sizeof(double) * nq * nn, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && a.chi2) e = hipMemcpyAsync(a.chi2, d.chi2, sizeof(double) * nq, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && a.rank) e = hipMemcpyAsync(a.rank, d.rank, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, s);
    }
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(base);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        h->err = std::string(src.what) + " (host arrays): " + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return rc;
}

// The checks of every one of the entry points, in the documented order, and then the fit.
int nlh_fit_run(nlh_handle *h, const nlh_options *opts, const FitSource &src, const FitArgs &a, bool host)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (src.N < 0 || a.nprob < 0 || a.m < 1) return NLH_INVALID_INPUT_ERROR;
    int32_t n = src.N;                                            // the unknowns: the free parameters of a map
    if (a.pm) {
        int32_t nfull;
        nlh_pmap_shape(a.pm, &nfull, &n, nullptr);
        if (nfull != src.N) return NLH_INVALID_INPUT_ERROR;
    }
    int64_t M = a.m;                                              // the rows of a problem of the solve: a group's G m
    if (a.grp) {
        int32_t nfull, G;
        if (a.pm) return NLH_INVALID_INPUT_ERROR;
        nlh_group_shape(a.grp, &nfull, nullptr, &G, &n);
        if (nfull != src.N || a.nprob % G != 0) return NLH_INVALID_INPUT_ERROR;
        M = (int64_t)G * a.m;
        if (M > 0x7fffffff) return NLH_ARRAY_SIZE_ERROR;
    }
    if (M < n) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    if (!nlh_loss_kind_ok(a.loss)) return NLH_INVALID_INPUT_ERROR;
    if (a.stat != NLH_STAT_LSQ && a.stat != NLH_STAT_POISSON) return NLH_INVALID_INPUT_ERROR;
    if (a.stat == NLH_STAT_POISSON && a.loss != NLH_LOSS_LINEAR) return NLH_INVALID_INPUT_ERROR;
    if (a.nprob == 0) return 0;
    if (!opts || !a.t || !a.y || !a.x || !a.fvec || (a.loss != NLH_LOSS_LINEAR && !a.scale)) return NLH_INVALID_INPUT_ERROR;
    if ((a.sigma || a.cov || a.chi2) && M <= n) return NLH_INVALID_INPUT_ERROR;     // no degree of freedom for errors
    if (a.stat == NLH_STAT_POISSON && !nlh_pois_floor_ok(a.mu_floor)) return NLH_INVALID_INPUT_ERROR;
    if (a.cv && !nlh_conv_ok(a.cv)) return NLH_INVALID_INPUT_ERROR;
    if (host && a.cv && !nlh_conv_data_ok(a.cv, a.y, (size_t)a.nprob, (size_t)a.m)) return NLH_INVALID_INPUT_ERROR;
    if (host && a.stat == NLH_STAT_POISSON && !nlh_pois_data_ok(a.y, a.w, (size_t)a.nprob * a.m)) return NLH_INVALID_INPUT_ERROR;
    if (a.want_sp) {            // a separable fit, after every check of the _conv entry point: the object, its N, no shared or bounded projected parameter
        int32_t nfull, L, S = 0;
        if (!a.sp || !a.sp_jac) return NLH_INVALID_INPUT_ERROR;
        nlh_sep_shape(a.sp, &nfull, &L, nullptr);
        if (nfull != src.N) return NLH_INVALID_INPUT_ERROR;
        if (a.pm || a.loss != NLH_LOSS_LINEAR || a.stat != NLH_STAT_LSQ) return NLH_INVALID_INPUT_ERROR;
        std::vector<int32_t> lin(L);
        nlh_sep_tables(a.sp, lin.data(), nullptr);
        if (a.grp) nlh_group_shape(a.grp, nullptr, &S, nullptr, nullptr);
        for (int32_t k : lin)
            if (a.grp && nlh_group_index(a.grp, 0, k) < S) return NLH_INVALID_INPUT_ERROR;     // a shared linear parameter
        for (int32_t k : lin)
            if ((a.xl && std::isfinite(a.xl[k])) || (a.xu && std::isfinite(a.xu[k]))) return NLH_INVALID_INPUT_ERROR;
    }
    if (!host) return fit_device(h, opts, src, a, n);
    double *dscale = nullptr;                                     // checks the host scales: finite, positive (LINEAR: none, NULL)
    int rc = nlh_loss_scale_upload(h, a.loss, a.scale, a.shared_scale ? 1 : (size_t)a.nprob, &dscale);
    if (rc) return rc;
    rc = fit_staged(h, opts, src, a, n, dscale);
    if (dscale) (void)hipFree(dscale);
    return rc;
}
