// nlh_pmap.hip -- parameter maps (include/nonlin_hip.h: nlh_pmap_*): fixed and tied parameters for any device model, as a
// pair of wrapping launchers around any inner launcher pair (kernels and arithmetic: nlh_kernels_pmap.h; scratch, grid and
// slice loop: nlh_launch.h).  Here: the map object (host code; needs no GPU), the wrapping context, the launchers, and the
// small gather / expand / covariance steps, which the one-call fits through a map use too (nlh_fit.hip).  The model object is
// nlh_pmap_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
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

struct nlh_pmap_ctx : WrapCtx {
    PmapTables T;                      // the context's own copy of the tables (WrapCtx::tables: their allocation)
    const double *dfull = nullptr;
    int shared_full = 0;
};

const PmapTables *pmap_ctx_tables(const nlh_pmap_ctx *c) { return &c->T; }
void pmap_ctx_rebind(nlh_pmap_ctx *c, const double *dfull) { c->dfull = dfull; }

int nlh_pmap_wrap(nlh_handle *h, const nlh_pmap *pm, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, const double *dfull,
                  int32_t shared_full, nlh_pmap_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !pm) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (pm->any_fixed && !dfull) return NLH_INVALID_INPUT_ERROR;
    nlh_pmap_ctx *c = nullptr;
    int rc = wrap_new(h, PMAP_MAGIC, fcn, jac, inner_ctx, &c);
    if (rc) return rc;
    PmapDev tab;
    if ((rc = pmap_upload(pm, &tab))) { h->err = "parameter map: tables to the device"; delete c; return rc; }
    c->T = tab.T; c->tables = tab.base; c->dfull = dfull; c->shared_full = shared_full != 0;
    *out = c;
    return 0;
}

// The one release of a wrapping context of any kind (nlh_internal.h).
void wrap_release(WrapCtx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    c->scratch.free_all();
    if (c->tables) hipFree(c->tables);
    c->magic = 0;
    delete c;
}

void nlh_pmap_unwrap(nlh_pmap_ctx *c)
{
    if (c && c->magic == PMAP_MAGIC) wrap_release(c);
}

static void pmap_launch_jac(const nlh_pmap_ctx *c, int m, int npoints, const double *Jf, double *J, hipStream_t s)
{
    const PmapTables &T = c->T;
    const JacGrid g = jac_grid("NLH_PMAP_FORM", "NLH_PMAP_SPLIT", c->cus, m, T.n, npoints);
    if (g.flat) hipLaunchKernelGGL(k_pmap_jac<true>, g.grid, dim3(256), 0, s, T, m, g.nblk, g.ppw, g.cpg, npoints, Jf, J);
    else hipLaunchKernelGGL(k_pmap_jac<false>, g.grid, dim3(256), 0, s, T, m, g.nblk, g.ppw, g.cpg, npoints, Jf, J);
}

// Both launchers.  What they check themselves is refused before any launch.  The inner launcher can refuse only once it is
// called, which is after the expansion of its slice has been enqueued: then only the context's scratch has been written,
// nothing of the caller's, and the call returns the inner error without a further launch.
static int pmap_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_pmap_ctx *c = wrap_ctx<nlh_pmap_ctx>(ctx, PMAP_MAGIC);
    int end;
    if (wrap_refused(c, c && n == c->T.n && m >= 1 && dX && out, jac, npoints, &end)) return end;
    const PmapTables &T = c->T;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t N = (size_t)T.N;
    // scratch per point: the full parameters P and, for a Jacobian call, the inner Jacobian Jf over them
    return wrap_slices(c->scratch, "NLH_PMAP_SCRATCH", c->device, s, N * (jac ? (size_t)m + 1 : 1), npoints, m, dprob,
                       [&](double *P, int slice, int q0, int cnt, const int32_t *lp) {
        double *Jf = P + (size_t)slice * N;
        hipLaunchKernelGGL(k_pmap_expand, dim3((unsigned)(((size_t)cnt * N + 255) / 256)), dim3(256), 0, s, T, cnt, lp, dX + (size_t)q0 * n,
                           c->dfull, c->shared_full, P);
        if (!jac) return c->fcn(c->inner, hip_stream, cnt, lp, T.N, P, m, out + (size_t)q0 * m);
        if (const int rc = c->jac(c->inner, hip_stream, cnt, lp, T.N, P, m, Jf)) return rc;
        pmap_launch_jac(c, m, cnt, Jf, out + (size_t)q0 * m * n, s);
        return 0;
    });
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

// the three launches, on any copy of the tables (nlh_internal.h: the one-call fits use a context's)
void pmap_gather(const PmapTables *T, hipStream_t s, int nprob, const double *full, double *x)
{
    hipLaunchKernelGGL(k_pmap_gather, dim3(pmap_blocks((size_t)nprob * T->N)), dim3(256), 0, s, *T, nprob, full, x);
}

void pmap_expand(const PmapTables *T, hipStream_t s, int nprob, const double *x, const double *full, int shared_full, double *p)
{
    hipLaunchKernelGGL(k_pmap_expand, dim3(pmap_blocks((size_t)nprob * T->N)), dim3(256), 0, s, *T, nprob, (const int32_t *)nullptr, x, full,
                       shared_full, p);
}

void pmap_cov(const PmapTables *T, hipStream_t s, int nprob, const double *cov, const double *sigma, const int32_t *fail, double *covf,
              double *sigf)
{
    const size_t N = (size_t)T->N;
    hipLaunchKernelGGL(k_pmap_cov, dim3(pmap_blocks((size_t)nprob * (covf ? N * N : N))), dim3(256), 0, s, *T, nprob, cov, sigma, fail, covf,
                       sigf);
}

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
    pmap_gather(&T, h->stream, nprob, dfull, dx);
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
    pmap_expand(&T, h->stream, nprob, dx, dfull, shared_full != 0, dp);
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
    pmap_cov(&T, h->stream, nprob, dcov, dsigma, dfail, dcov_full, dsigma_full);
    HIPCHK(h, hipGetLastError());
    return 0;
}
