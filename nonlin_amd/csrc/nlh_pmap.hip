// nlh_pmap.hip -- parameter maps (include/nonlin_hip.h: nlh_pmap_*): fixed and tied parameters for any device model, as a
// pair of wrapping launchers around any inner launcher pair (kernels and arithmetic: nlh_kernels_pmap.h).  Here: the map
// object (host code; needs no GPU), the wrapping context and its per-stream scratch, the launchers and the form a contraction runs,
// the small gather / expand / covariance steps, and the one-call fits through a map (nlh_curve_fit_batch_pmap,
// nlh_expr_fit_batch_pmap: nlh_fit_compose over the free unknowns, between a gather and an expansion).  The model object is
// nlh_pmap_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_kernels_pmap.h"

// ---------------------------------------------------------------------------------------------------------------------
// the map object
// ---------------------------------------------------------------------------------------------------------------------
struct PmapDev {                       // device copies of a map's tables: one allocation
    PmapTables T;
    void *base = nullptr;
    int device = 0;
};

struct nlh_pmap {
    int32_t nfull = 0, nfree = 0, ntied = 0;
    bool any_fixed = false;            // then full is read, and may not be NULL (nlh_pmap_wrap, nlh_pmap_expand_batch)
    std::vector<int32_t> kind, index, f2f;
    std::vector<double> scale, offset;
    // per free column, its ties in ascending k (CSR); the covariance's free number and factor per full parameter
    std::vector<int32_t> tptr, tk, cj;
    std::vector<double> ts, cg;
    // Device copies for the three entry points that take a map and no context (nlh_pmap_gather_batch, _expand_batch,
    // _cov_batch), made on their first use on a device and freed by nlh_pmap_destroy: the one thing of a map that is not
    // host memory.  A context (nlh_pmap_wrap) uploads its own copy and does not depend on the map afterwards.
    mutable std::mutex mu;
    mutable std::vector<PmapDev> dev;
};

int nlh_pmap_create(int32_t nfull, const int32_t *kind, const int32_t *src, const double *scale, const double *offset, nlh_pmap **pm)
{
    if (!pm) return NLH_INVALID_INPUT_ERROR;
    *pm = nullptr;
    if (nfull < 1 || nfull > NLH_PMAP_MAX_N || !kind) return NLH_INVALID_INPUT_ERROR;
    const int N = nfull;
    for (int k = 0; k < N; ++k) {
        if (kind[k] < NLH_PMAP_FREE || kind[k] > NLH_PMAP_TIED) return NLH_INVALID_INPUT_ERROR;
        if (kind[k] != NLH_PMAP_TIED) continue;
        if (!src || !scale || !offset) return NLH_INVALID_INPUT_ERROR;
        const int s = src[k];
        if (s < 0 || s >= N || s == k || kind[s] == NLH_PMAP_TIED) return NLH_INVALID_INPUT_ERROR;
        if (!std::isfinite(scale[k]) || !std::isfinite(offset[k]) || scale[k] == 0.0) return NLH_INVALID_INPUT_ERROR;
    }
    nlh_pmap *p = new nlh_pmap();
    p->nfull = N;
    p->kind.assign(kind, kind + N);
    p->index.assign(N, -1); p->scale.assign(N, 1.0); p->offset.assign(N, 0.0);
    p->cj.assign(N, -1); p->cg.assign(N, 1.0);
    for (int k = 0; k < N; ++k)
        if (kind[k] == NLH_PMAP_FREE) { p->index[k] = p->nfree++; p->f2f.push_back(k); p->cj[k] = p->index[k]; }
        else if (kind[k] == NLH_PMAP_FIXED) p->any_fixed = true;
    if (p->nfree == 0) { delete p; return NLH_INVALID_INPUT_ERROR; }
    std::vector<std::vector<int32_t>> ties(p->nfree);
    for (int k = 0; k < N; ++k)
        if (kind[k] == NLH_PMAP_TIED) {
            ++p->ntied;
            p->index[k] = src[k]; p->scale[k] = scale[k]; p->offset[k] = offset[k];
            if (kind[src[k]] == NLH_PMAP_FREE) {
                ties[p->index[src[k]]].push_back(k);
                p->cj[k] = p->index[src[k]]; p->cg[k] = scale[k];
            }
        }
    p->tptr.push_back(0);
    for (int j = 0; j < p->nfree; ++j) {
        for (int32_t k : ties[j]) { p->tk.push_back(k); p->ts.push_back(scale[k]); }
        p->tptr.push_back((int32_t)p->tk.size());
    }
    *pm = p;
    return 0;
}

void nlh_pmap_destroy(nlh_pmap *pm)
{
    if (!pm) return;
    for (PmapDev &d : pm->dev) { hipSetDevice(d.device); hipFree(d.base); }
    delete pm;
}

void nlh_pmap_shape(const nlh_pmap *pm, int32_t *nfull, int32_t *nfree, int32_t *ntied)
{
    if (nfull) *nfull = pm ? pm->nfull : 0;
    if (nfree) *nfree = pm ? pm->nfree : 0;
    if (ntied) *ntied = pm ? pm->ntied : 0;
}

int nlh_pmap_tables(const nlh_pmap *pm, int32_t *kind, int32_t *index, double *scale, double *offset, int32_t *free_to_full)
{
    if (!pm) return NLH_INVALID_INPUT_ERROR;
    const size_t N = pm->nfull;
    if (kind) memcpy(kind, pm->kind.data(), sizeof(int32_t) * N);
    if (index) memcpy(index, pm->index.data(), sizeof(int32_t) * N);
    if (scale) memcpy(scale, pm->scale.data(), sizeof(double) * N);
    if (offset) memcpy(offset, pm->offset.data(), sizeof(double) * N);
    if (free_to_full) memcpy(free_to_full, pm->f2f.data(), sizeof(int32_t) * pm->nfree);
    return 0;
}

// The tables on the current device: doubles first (scale, offset, cg [N], ts), then the int32 ones.
static int pmap_upload(const nlh_pmap *pm, PmapDev *d)
{
    const size_t N = pm->nfull, n = pm->nfree, nt = pm->tk.size();
    std::vector<double> hd;
    hd.insert(hd.end(), pm->scale.begin(), pm->scale.end());
    hd.insert(hd.end(), pm->offset.begin(), pm->offset.end());
    hd.insert(hd.end(), pm->cg.begin(), pm->cg.end());
    hd.insert(hd.end(), pm->ts.begin(), pm->ts.end());
    std::vector<int32_t> hi;
    hi.insert(hi.end(), pm->kind.begin(), pm->kind.end());
    hi.insert(hi.end(), pm->index.begin(), pm->index.end());
    hi.insert(hi.end(), pm->cj.begin(), pm->cj.end());
    hi.insert(hi.end(), pm->f2f.begin(), pm->f2f.end());
    hi.insert(hi.end(), pm->tptr.begin(), pm->tptr.end());
    hi.insert(hi.end(), pm->tk.begin(), pm->tk.end());
    const size_t db = sizeof(double) * hd.size(), ib = sizeof(int32_t) * hi.size();
    char *base = nullptr;
    if (hipMalloc(&base, db + ib) != hipSuccess) return NLH_OUT_OF_MEMORY_ERROR;
    if (hipMemcpy(base, hd.data(), db, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + db, hi.data(), ib, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(base);
        return NLH_ERR_HIP;
    }
    const double *dd = (const double *)base;
    const int32_t *di = (const int32_t *)(base + db);
    PmapTables &T = d->T;
    T.N = (int)N; T.n = (int)n;
    T.scale = dd; T.offset = dd + N; T.cg = dd + 2 * N; T.ts = dd + 3 * N;
    T.kind = di; T.index = di + N; T.cj = di + 2 * N; T.f2f = di + 3 * N; T.tptr = T.f2f + n; T.tk = T.tptr + n + 1;
    (void)nt;
    d->base = base;
    return 0;
}

// the map's own copy on the handle's device (made on first use, freed by nlh_pmap_destroy)
static int pmap_device_tables(nlh_handle *h, const nlh_pmap *pm, PmapTables *T)
{
    std::lock_guard<std::mutex> lock(pm->mu);
    for (const PmapDev &d : pm->dev)
        if (d.device == h->device) { *T = d.T; return 0; }
    PmapDev d;
    d.device = h->device;
    const int rc = pmap_upload(pm, &d);
    if (rc) { h->err = "parameter map: tables to the device"; return rc; }
    pm->dev.push_back(d);
    *T = d.T;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the wrapping context
// ---------------------------------------------------------------------------------------------------------------------
static const uint32_t PMAP_MAGIC = 0x70614d70u;
static const size_t PMAP_SCRATCH_CAP = (size_t)1 << 30;         // per call, so per stream; beyond it the points go in slices

struct PmapScratch { hipStream_t s; void *p; size_t bytes; };

struct nlh_pmap_ctx {
    uint32_t magic = PMAP_MAGIC;
    int device = 0, cus = 1;
    PmapDev tab;
    nlh_device_vecfcn fcn = nullptr;
    nlh_device_jacfcn jac = nullptr;
    void *inner = nullptr;
    const double *dfull = nullptr;
    int shared_full = 0;
    // One buffer per stream: calls on one stream are ordered, so the next call's kernels find the last call's done with it;
    // calls from several host threads come on different streams and never share one.  A buffer is at most the cap, is kept
    // until nlh_pmap_unwrap and never shrinks: a context holds up to the cap times the streams it was called on.
    std::mutex mu;
    std::vector<PmapScratch> scratch;
};

int nlh_pmap_wrap(nlh_handle *h, const nlh_pmap *pm, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, const double *dfull,
                  int32_t shared_full, nlh_pmap_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !pm) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (pm->any_fixed && !dfull) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    nlh_pmap_ctx *c = new nlh_pmap_ctx();
    c->device = h->device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) c->cus = cus;
    c->tab.device = h->device;
    const int rc = pmap_upload(pm, &c->tab);
    if (rc) { h->err = "parameter map: tables to the device"; delete c; return rc; }
    c->fcn = fcn; c->jac = jac; c->inner = inner_ctx; c->dfull = dfull; c->shared_full = shared_full != 0;
    *out = c;
    return 0;
}

void nlh_pmap_unwrap(nlh_pmap_ctx *c)
{
    if (!c || c->magic != PMAP_MAGIC) return;
    hipSetDevice(c->device);
    for (PmapScratch &s : c->scratch) hipFree(s.p);               // (hipFree waits for the work that still uses it)
    hipFree(c->tab.base);
    c->magic = 0;
    delete c;
}

// Growing a buffer is hipFree + hipMalloc under the context's mutex: the free waits for the device, and other threads' calls
// wait for the mutex meanwhile.  That happens on the first calls of a solve (its largest launch comes early), not per round.
static void *pmap_scratch(nlh_pmap_ctx *c, hipStream_t s, size_t bytes)
{
    std::lock_guard<std::mutex> lock(c->mu);
    PmapScratch *b = nullptr;
    for (PmapScratch &e : c->scratch) if (e.s == s) b = &e;
    if (!b) { c->scratch.push_back({s, nullptr, 0}); b = &c->scratch.back(); }
    if (b->bytes < bytes) {
        if (b->p) hipFree(b->p);
        b->p = nullptr; b->bytes = 0;
        if (hipMalloc(&b->p, bytes) != hipSuccess) { b->p = nullptr; return nullptr; }
        b->bytes = bytes;
    }
    return b->p;
}

// The form a contraction runs, as the curve models choose it.  NLH_PMAP_FORM = row | flat (environment, read at every call;
// tests) forces a form for the sizes it can hold (flat: m <= 256).
static bool pmap_flat(int m)
{
    if (m > 256) return false;
    if (const char *e = getenv("NLH_PMAP_FORM")) {
        if (!strcmp(e, "row")) return false;
        if (!strcmp(e, "flat")) return true;
    }
    return 256 / m >= 2;
}

// Groups the free columns are split into.  A compute unit holds eight workgroups of 256 threads; below four per unit -- four
// waves per SIMD, half of what it can hold -- a streaming kernel does not keep enough loads in flight, so the columns are
// dealt over gridDim.y until the launch has that many (or a column per group).  NLH_PMAP_SPLIT (environment; tests) overrides.
static int pmap_groups(int cus, size_t wgs, int n)
{
    size_t g = 1;
    const size_t want = (size_t)4 * cus;
    if (wgs < want) g = (want + wgs - 1) / wgs;
    if (const char *e = getenv("NLH_PMAP_SPLIT")) {
        const int v = atoi(e);
        if (v >= 1) g = (size_t)v;
    }
    return (int)std::min<size_t>(g, (size_t)n);
}

static void pmap_launch_jac(const nlh_pmap_ctx *c, int m, int npoints, const double *Jf, double *J, hipStream_t s)
{
    const PmapTables &T = c->tab.T;
    const bool flat = pmap_flat(m);
    const int ppw = flat ? 256 / m : 1, nblk = flat ? 1 : (m + 255) / 256;
    const size_t wgs = flat ? (size_t)(npoints + ppw - 1) / ppw : (size_t)npoints * nblk;
    const int groups = pmap_groups(c->cus, wgs, T.n);
    const int cpg = (T.n + groups - 1) / groups;
    const dim3 grid((unsigned)wgs, (unsigned)((T.n + cpg - 1) / cpg));
    if (flat) hipLaunchKernelGGL(k_pmap_jac<true>, grid, dim3(256), 0, s, T, m, nblk, ppw, cpg, npoints, Jf, J);
    else hipLaunchKernelGGL(k_pmap_jac<false>, grid, dim3(256), 0, s, T, m, nblk, ppw, cpg, npoints, Jf, J);
}

// Both launchers.  What they check themselves is refused before any launch.  The inner launcher can refuse only once it is
// called, which is after the expansion of its slice has been enqueued: then only the context's scratch has been written,
// nothing of the caller's, and the call returns the inner error without a further launch.
static int pmap_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_pmap_ctx *c = (nlh_pmap_ctx *)ctx;
    if (!c || c->magic != PMAP_MAGIC || !c->fcn) return NLH_INVALID_INPUT_ERROR;
    const PmapTables &T = c->tab.T;
    if (n != T.n || m < 1 || !dX || !out) return NLH_INVALID_INPUT_ERROR;
    if (jac && !c->jac) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (npoints <= 0) return 0;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t N = (size_t)T.N;
    const size_t per = sizeof(double) * N * (jac ? (size_t)m + 1 : 1) + (dprob ? 0 : sizeof(int32_t));
    size_t cap = PMAP_SCRATCH_CAP;
    if (const char *e = getenv("NLH_PMAP_SCRATCH")) {
        const long long v = atoll(e);
        if (v > 0 && (size_t)v < cap) cap = (size_t)v;
    }
    const int slice = (int)std::max<size_t>(1, std::min<size_t>((size_t)npoints, cap / per));
    if ((size_t)slice * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (hipSetDevice(c->device) != hipSuccess) return NLH_ERR_HIP;
    char *base = (char *)pmap_scratch(c, s, (size_t)slice * per + 64);
    if (!base) return NLH_OUT_OF_MEMORY_ERROR;
    double *P = (double *)base, *Jf = P + (size_t)slice * N;
    int32_t *list = (int32_t *)(base + sizeof(double) * (size_t)slice * N * (jac ? (size_t)m + 1 : 1));
    for (int q0 = 0; q0 < npoints; q0 += slice) {
        const int cnt = std::min(slice, npoints - q0);
        const int32_t *lp = dprob ? dprob + q0 : list;
        if (!dprob) hipLaunchKernelGGL(k_pmap_iota, dim3((cnt + 255) / 256), dim3(256), 0, s, cnt, q0, list);
        hipLaunchKernelGGL(k_pmap_expand, dim3((unsigned)(((size_t)cnt * N + 255) / 256)), dim3(256), 0, s, T, cnt, lp, dX + (size_t)q0 * n,
                           c->dfull, c->shared_full, P);
        int rc;
        if (!jac) rc = c->fcn(c->inner, hip_stream, cnt, lp, T.N, P, m, out + (size_t)q0 * m);
        else rc = c->jac(c->inner, hip_stream, cnt, lp, T.N, P, m, Jf);
        if (rc) return rc;
        if (jac) pmap_launch_jac(c, m, cnt, Jf, out + (size_t)q0 * m * n, s);
    }
    return 0;
}

int nlh_pmap_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return pmap_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_pmap_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return pmap_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

// ---------------------------------------------------------------------------------------------------------------------
// gather, expand, covariance of the full parameters
// ---------------------------------------------------------------------------------------------------------------------
static unsigned pmap_blocks(size_t threads) { return (unsigned)((threads + 255) / 256); }

static int pmap_batch_check(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, size_t per, PmapTables *T)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!pm || nprob < 0) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)nprob * per + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    return pmap_device_tables(h, pm, T);
}

int nlh_pmap_gather_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dfull, double *dx)
{
    PmapTables T;
    const int rc = pmap_batch_check(h, pm, nprob, pm ? pm->nfull : 0, &T);
    if (rc) return rc;
    if (nprob == 0) return 0;
    if (!dfull || !dx) return NLH_INVALID_INPUT_ERROR;
    hipLaunchKernelGGL(k_pmap_gather, dim3(pmap_blocks((size_t)nprob * T.N)), dim3(256), 0, h->stream, T, nprob, dfull, dx);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_pmap_expand_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dx, const double *dfull, int32_t shared_full,
                          double *dp)
{
    PmapTables T;
    const int rc = pmap_batch_check(h, pm, nprob, pm ? pm->nfull : 0, &T);
    if (rc) return rc;
    if (nprob == 0) return 0;
    if (!dx || !dp || dp == dfull || (pm->any_fixed && !dfull)) return NLH_INVALID_INPUT_ERROR;    // (dfull: nlh_pmap_wrap's rule)
    hipLaunchKernelGGL(k_pmap_expand, dim3(pmap_blocks((size_t)nprob * T.N)), dim3(256), 0, h->stream, T, nprob, (const int32_t *)nullptr, dx,
                       dfull, shared_full != 0, dp);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_pmap_cov_batch(nlh_handle *h, const nlh_pmap *pm, int32_t nprob, const double *dcov, const double *dsigma, const int32_t *dfail,
                       double *dcov_full, double *dsigma_full)
{
    PmapTables T;
    const size_t N = pm ? pm->nfull : 0;
    const int rc = pmap_batch_check(h, pm, nprob, dcov_full ? N * N : N, &T);
    if (rc) return rc;
    if (nprob == 0 || (!dcov_full && !dsigma_full)) return 0;
    if ((dcov_full && !dcov) || (dsigma_full && !dsigma)) return NLH_INVALID_INPUT_ERROR;
    hipLaunchKernelGGL(k_pmap_cov, dim3(pmap_blocks((size_t)nprob * (dcov_full ? N * N : N))), dim3(256), 0, h->stream, T, nprob, dcov, dsigma,
                       dfail, dcov_full, dsigma_full);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fit + errors through a map: nlh_fit_compose over the free unknowns, between a gather and an expansion
// ---------------------------------------------------------------------------------------------------------------------
int nlh_fit_compose_pmap(nlh_handle *h, const nlh_options *opts, const nlh_pmap *pm, int32_t nprob, int32_t m, nlh_device_vecfcn fcn,
                            nlh_device_jacfcn jac, void *ctx, const std::function<void(int32_t)> &at, const double *dw, const double *xl,
                            const double *xu, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                            nlh_iteration_behavior *ib, int32_t *status)
{
    const size_t N = pm->nfull, n = pm->nfree, np = (size_t)nprob;
    if ((dsigma || dcov || dchi2) && m <= (int32_t)n) return NLH_INVALID_INPUT_ERROR;
    if ((np * (dcov ? N * N : N) + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc = 0;
    // a private copy of the full parameters (the fixed values), the free unknowns, the free sigma and cov, the failure flags
    const size_t doubles = np * N + np * n + (dsigma ? np * n : 0) + (dcov ? np * n * n : 0);
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * doubles + sizeof(int32_t) * np) != hipSuccess) {
        h->err = "hipMalloc (fit through a parameter map)";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    double *q = base;
    double *fullc = q; q += np * N;
    double *xf = q; q += np * n;
    double *sf = dsigma ? q : nullptr; q += dsigma ? np * n : 0;
    double *cf = dcov ? q : nullptr; q += dcov ? np * n * n : 0;
    int32_t *dfail = (int32_t *)q;
    std::vector<double> lo, hi;
    if (xl) { lo.resize(n); for (size_t j = 0; j < n; ++j) lo[j] = xl[pm->f2f[j]]; }
    if (xu) { hi.resize(n); for (size_t j = 0; j < n; ++j) hi[j] = xu[pm->f2f[j]]; }
    std::vector<int32_t> st(np, 0);
    nlh_pmap_ctx *pc = nullptr;                                   // its copy of the tables serves the steps here too
    hipError_t e = hipSuccess;
    rc = nlh_pmap_wrap(h, pm, fcn, jac, ctx, fullc, 0, &pc);
    if (!rc) e = hipMemcpyAsync(fullc, dx, sizeof(double) * np * N, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && !rc) {
        const PmapTables &T = pc->tab.T;
        hipLaunchKernelGGL(k_pmap_gather, dim3(pmap_blocks(np * N)), dim3(256), 0, s, T, nprob, (const double *)fullc, xf);
        auto at_run = [&](int32_t p0) {                           // a run of problems counts its dprob from its first one
            at(p0);
            pc->dfull = fullc + (size_t)p0 * N;
        };
        rc = nlh_fit_compose(h, opts, nprob, m, (int32_t)n, nlh_pmap_device_fcn, jac ? nlh_pmap_device_jac : nullptr, pc, at_run, dw,
                             xl ? lo.data() : nullptr, xu ? hi.data() : nullptr, xf, dfvec, sf, cf, dchi2, drank, ib, st.data());
    }
    if (e == hipSuccess && !rc) {
        // every problem, also one that was refused on its degrees of freedom and kept its x: on exit dx obeys the map
        const PmapTables &T = pc->tab.T;
        hipLaunchKernelGGL(k_pmap_expand, dim3(pmap_blocks(np * N)), dim3(256), 0, s, T, nprob, (const int32_t *)nullptr, (const double *)xf,
                           (const double *)fullc, 0, dx);
        if (dsigma || dcov) {
            e = hipMemcpyAsync(dfail, st.data(), sizeof(int32_t) * np, hipMemcpyHostToDevice, s);
            if (e == hipSuccess)
                hipLaunchKernelGGL(k_pmap_cov, dim3(pmap_blocks(np * (dcov ? N * N : N))), dim3(256), 0, s, T, nprob, (const double *)cf,
                                   (const double *)sf, (const int32_t *)dfail, dcov, dsigma);
        }
        if (e == hipSuccess) e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(s);                // (st is a host vector; the buffers go)
    nlh_pmap_unwrap(pc);
    (void)hipFree(base);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        h->err = std::string("fit through a parameter map: ") + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    if (!rc && status) memcpy(status, st.data(), sizeof(int32_t) * np);
    return rc;
}

int nlh_curve_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                             const double *dt, int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl,
                             const double *xu, const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2,
                             int32_t *drank, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!pm)
        return nlh_curve_fit_batch(h, opts, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, dx, dfvec, dsigma, dcov, dchi2,
                                   drank, ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t N = nlh_curve_nparams(kind, ncomp, nbase);
    if (N < 0 || nprob < 0 || m < 1 || pm->nfull != N) return NLH_INVALID_INPUT_ERROR;
    if (m < pm->nfree) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    if (nprob == 0) return 0;
    if (!opts || !dt || !dy || !dx || !dfvec) return NLH_INVALID_INPUT_ERROR;
    nlh_curve_ctx c;
    c.kind = kind; c.ncomp = ncomp; c.nbase = nbase; c.shared_t = shared_t != 0; c.m = m;
    auto at = [&](int32_t p0) {
        c.dt = shared_t ? dt : dt + (size_t)p0 * m;
        c.dy = dy + (size_t)p0 * m;
        c.dw = dw ? dw + (size_t)p0 * m : nullptr;
    };
    return nlh_fit_compose_pmap(h, opts, pm, nprob, m, nlh_curve_device_fcn, analytic ? nlh_curve_device_jac : nullptr, &c, at, dw, xl, xu, dx, dfvec,
                            dsigma, dcov, dchi2, drank, ib, status);
}

int nlh_curve_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m,
                               const double *t, int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl,
                               const double *xu, const nlh_pmap *pm, double *x, double *fvec, double *sigma, double *cov, double *chi2,
                               int32_t *rank, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!pm)
        return nlh_curve_fit_batch_h(h, opts, kind, ncomp, nbase, nprob, m, t, shared_t, y, w, analytic, xl, xu, x, fvec, sigma, cov, chi2, rank,
                                     ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t N = nlh_curve_nparams(kind, ncomp, nbase);
    if (N < 0 || nprob < 0 || m < 1 || pm->nfull != N) return NLH_INVALID_INPUT_ERROR;
    if (m < pm->nfree) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    if (nprob == 0) return 0;
    if (!opts || !t || !y || !x || !fvec) return NLH_INVALID_INPUT_ERROR;
    return nlh_fit_compose_h(h, "curve fit", shared_t ? (size_t)m : (size_t)nprob * m, nprob, m, N, t, y, w, x, fvec, sigma, cov, chi2, rank,
                             [&](const double *dt, const double *dy, const double *dw, double *dx, double *df, double *ds, double *dc,
                                 double *dq, int32_t *dr) {
                                 return nlh_curve_fit_batch_pmap(h, opts, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu,
                                                                 pm, dx, df, ds, dc, dq, dr, ib, status);
                             }, pm->nfree);
}

int nlh_expr_fit_batch_pmap(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *dt,
                            int32_t shared_t, const double *dy, const double *dw, int32_t analytic, const double *xl, const double *xu,
                            const nlh_pmap *pm, double *dx, double *dfvec, double *dsigma, double *dcov, double *dchi2, int32_t *drank,
                            nlh_iteration_behavior *ib, int32_t *status)
{
    if (!pm)
        return nlh_expr_fit_batch(h, opts, e, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, dx, dfvec, dsigma, dcov, dchi2, drank, ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!e || nprob < 0 || m < 1 || pm->nfull != e->prog.nparams) return NLH_INVALID_INPUT_ERROR;
    if (m < pm->nfree) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    if (nprob == 0) return 0;
    if (!opts || !dt || !dy || !dx || !dfvec) return NLH_INVALID_INPUT_ERROR;
    nlh_expr_ctx c;
    c.e = e; c.shared_t = shared_t != 0; c.m = m;
    c.dt_stride = shared_t ? (int64_t)m : (int64_t)nprob * m;      // (a run of problems keeps the whole batch's stride)
    auto at = [&](int32_t p0) {
        c.dt = shared_t ? dt : dt + (size_t)p0 * m;
        c.dy = dy + (size_t)p0 * m;
        c.dw = dw ? dw + (size_t)p0 * m : nullptr;
    };
    return nlh_fit_compose_pmap(h, opts, pm, nprob, m, nlh_expr_device_fcn, analytic ? nlh_expr_device_jac : nullptr, &c, at, dw, xl, xu, dx, dfvec,
                            dsigma, dcov, dchi2, drank, ib, status);
}

int nlh_expr_fit_batch_pmap_h(nlh_handle *h, const nlh_options *opts, const nlh_expr *e, int32_t nprob, int32_t m, const double *t,
                              int32_t shared_t, const double *y, const double *w, int32_t analytic, const double *xl, const double *xu,
                              const nlh_pmap *pm, double *x, double *fvec, double *sigma, double *cov, double *chi2, int32_t *rank,
                              nlh_iteration_behavior *ib, int32_t *status)
{
    if (!pm)
        return nlh_expr_fit_batch_h(h, opts, e, nprob, m, t, shared_t, y, w, analytic, xl, xu, x, fvec, sigma, cov, chi2, rank, ib, status);
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!e || nprob < 0 || m < 1 || pm->nfull != e->prog.nparams) return NLH_INVALID_INPUT_ERROR;
    if (m < pm->nfree) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    if (nprob == 0) return 0;
    if (!opts || !t || !y || !x || !fvec) return NLH_INVALID_INPUT_ERROR;
    const size_t tm = (size_t)e->prog.nvar * (shared_t ? (size_t)m : (size_t)nprob * m);
    return nlh_fit_compose_h(h, "formula fit", tm, nprob, m, e->prog.nparams, t, y, w, x, fvec, sigma, cov, chi2, rank,
                             [&](const double *dt, const double *dy, const double *dw, double *dx, double *df, double *ds, double *dc,
                                 double *dq, int32_t *dr) {
                                 return nlh_expr_fit_batch_pmap(h, opts, e, nprob, m, dt, shared_t, dy, dw, analytic, xl, xu, pm, dx, df, ds,
                                                                dc, dq, dr, ib, status);
                             }, pm->nfree);
}
