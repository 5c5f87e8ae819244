// nlh_group.hip -- global fits (include/nonlin_hip.h: nlh_group_*): parameters shared across the data sets of a group, for any
// device model, as a pair of wrapping launchers around any inner launcher pair (kernels: nlh_kernels_group.h; scratch, grid
// and slice loop: nlh_launch.h).  Here: the group object (host code; needs no GPU), the wrapping context, the launchers, and
// the small gather / expand / sigma steps, which the one-call global fits use too (nlh_fit.hip).  The model object is
// nlh_group_model_create (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_group.h"

// ---------------------------------------------------------------------------------------------------------------------
// the group object
// ---------------------------------------------------------------------------------------------------------------------
struct GroupDev {                      // device copies of a group's tables: one allocation
    GroupTables T;
    void *base = nullptr;
    int device = 0;
};

struct nlh_group {
    int32_t N = 0, S = 0, L = 0, G = 0, n = 0;
    std::vector<int32_t> shared, slot, sidx, lidx;
    // Device copies for the three entry points that take a group and no context (nlh_group_gather_batch, _expand_batch,
    // _sigma_batch), made on their first use on a device and freed by nlh_group_destroy.  A context (nlh_group_wrap) uploads
    // its own copy and does not depend on the group afterwards.
    mutable std::mutex mu;
    mutable std::vector<GroupDev> dev;
};

int nlh_group_create(int32_t nfull, int32_t nshared, const int32_t *shared, int32_t nsets, nlh_group **g)
{
    if (!g) return NLH_INVALID_INPUT_ERROR;
    *g = nullptr;
    if (nfull < 1 || nfull > NLH_PMAP_MAX_N || nshared < 0 || nshared > nfull || nsets < 1 || (nshared > 0 && !shared))
        return NLH_INVALID_INPUT_ERROR;
    const int64_t nouter = (int64_t)nshared + (int64_t)nsets * (nfull - nshared);
    if (nouter > 0x7fffffff) return NLH_INVALID_INPUT_ERROR;
    std::vector<int32_t> is(nfull, 0);
    for (int s = 0; s < nshared; ++s) {
        const int k = shared[s];
        if (k < 0 || k >= nfull || is[k]) return NLH_INVALID_INPUT_ERROR;
        is[k] = 1;
    }
    nlh_group *p = new nlh_group();
    p->N = nfull; p->S = nshared; p->L = nfull - nshared; p->G = nsets; p->n = (int32_t)nouter;
    p->shared = is;
    p->slot.assign(nfull, 0);
    for (int k = 0; k < nfull; ++k) {
        std::vector<int32_t> &idx = is[k] ? p->sidx : p->lidx;
        p->slot[k] = (int32_t)idx.size();
        idx.push_back(k);
    }
    *g = p;
    return 0;
}

void nlh_group_destroy(nlh_group *g)
{
    if (!g) return;
    for (GroupDev &d : g->dev) { hipSetDevice(d.device); hipFree(d.base); }
    delete g;
}

void nlh_group_shape(const nlh_group *g, int32_t *nfull, int32_t *nshared, int32_t *nsets, int32_t *nouter)
{
    if (nfull) *nfull = g ? g->N : 0;
    if (nshared) *nshared = g ? g->S : 0;
    if (nsets) *nsets = g ? g->G : 0;
    if (nouter) *nouter = g ? g->n : 0;
}

int32_t nlh_group_index(const nlh_group *g, int32_t set, int32_t k)
{
    if (!g || set < 0 || set >= g->G || k < 0 || k >= g->N) return -1;
    return g->shared[k] ? g->slot[k] : g->S + set * g->L + g->slot[k];
}

// The tables on the current device: shared [N], slot [N], sidx [S], lidx [L].
static int group_upload(const nlh_group *g, GroupDev *d)
{
    std::vector<int32_t> hi;
    hi.insert(hi.end(), g->shared.begin(), g->shared.end());
    hi.insert(hi.end(), g->slot.begin(), g->slot.end());
    hi.insert(hi.end(), g->sidx.begin(), g->sidx.end());
    hi.insert(hi.end(), g->lidx.begin(), g->lidx.end());
    const size_t ib = sizeof(int32_t) * hi.size();
    int32_t *base = nullptr;
    if (hipMalloc(&base, ib) != hipSuccess) return NLH_OUT_OF_MEMORY_ERROR;
    if (hipMemcpy(base, hi.data(), ib, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(base);
        return NLH_ERR_HIP;
    }
    GroupTables &T = d->T;
    T.N = g->N; T.S = g->S; T.L = g->L; T.G = g->G; T.n = g->n;
    T.shared = base; T.slot = base + g->N; T.sidx = base + 2 * (size_t)g->N; T.lidx = T.sidx + g->S;
    d->base = base;
    return 0;
}

// the group's own copy on the handle's device (made on first use, freed by nlh_group_destroy)
static int group_device_tables(nlh_handle *h, const nlh_group *g, GroupTables *T)
{
    std::lock_guard<std::mutex> lock(g->mu);
    for (const GroupDev &d : g->dev)
        if (d.device == h->device) { *T = d.T; return 0; }
    GroupDev d;
    d.device = h->device;
    const int rc = group_upload(g, &d);
    if (rc) { h->err = "group: tables to the device"; return rc; }
    g->dev.push_back(d);
    *T = d.T;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the wrapping context
// ---------------------------------------------------------------------------------------------------------------------
static const uint32_t GROUP_MAGIC = 0x70755267u;

struct nlh_group_ctx : WrapCtx {
    GroupTables T;                     // the context's own copy of the tables (WrapCtx::tables: their allocation)
};

const GroupTables *group_ctx_tables(const nlh_group_ctx *c) { return &c->T; }

int nlh_group_wrap(nlh_handle *h, const nlh_group *g, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, nlh_group_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !g) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_group_ctx *c = nullptr;
    int rc = wrap_new(h, GROUP_MAGIC, fcn, jac, inner_ctx, &c);
    if (rc) return rc;
    GroupDev tab;
    if ((rc = group_upload(g, &tab))) { h->err = "group: tables to the device"; delete c; return rc; }
    c->T = tab.T; c->tables = tab.base;
    *out = c;
    return 0;
}

void nlh_group_unwrap(nlh_group_ctx *c)
{
    if (c && c->magic == GROUP_MAGIC) wrap_release(c);
}

static unsigned group_blocks(size_t threads) { return (unsigned)((threads + 255) / 256); }

// the scatter of npoints outer points: the grid is jac_grid's over the npoints G inner points and the n outer columns
static void group_launch_jac(const nlh_group_ctx *c, int m, int npoints, const double *Jf, double *J, hipStream_t s)
{
    const GroupTables &T = c->T;
    const int npin = npoints * T.G;
    const JacGrid g = jac_grid("NLH_GROUP_FORM", "NLH_GROUP_SPLIT", c->cus, m, T.n, npin);
    if (g.flat) hipLaunchKernelGGL(k_group_jac<true>, g.grid, dim3(256), 0, s, T, m, g.nblk, g.ppw, g.cpg, npin, Jf, J);
    else hipLaunchKernelGGL(k_group_jac<false>, g.grid, dim3(256), 0, s, T, m, g.nblk, g.ppw, g.cpg, npin, Jf, J);
}

// Both launchers.  What they check themselves is refused before any launch.  The inner launcher can refuse only once it is
// called, which is after the expansion of its slice has been enqueued: then only the context's scratch has been written,
// nothing of the caller's, and the call returns the inner error without a further launch.
static int group_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t M,
                      double *out)
{
    nlh_group_ctx *c = wrap_ctx<nlh_group_ctx>(ctx, GROUP_MAGIC);
    int end;
    if (wrap_refused(c, c && n == c->T.n && M >= 1 && M % c->T.G == 0 && dX && out, jac, npoints, &end)) return end;
    const GroupTables &T = c->T;
    if ((int64_t)npoints * T.G > 0x7fffffff) return NLH_ARRAY_SIZE_ERROR;
    hipStream_t s = (hipStream_t)hip_stream;
    const int m = M / T.G;
    const size_t N = (size_t)T.N, G = (size_t)T.G;
    // scratch per outer point: the inner parameters P of its G inner points, for a Jacobian call the inner Jacobian Jf over
    // them, and the G entries of the inner problem list (in whole doubles, behind the doubles)
    const size_t pd = G * N, jd = jac ? G * N * (size_t)m : 0, ld = (G + 1) / 2;
    return wrap_slices(c->scratch, "NLH_GROUP_SCRATCH", c->device, s, pd + jd + ld, npoints, M, dprob,
                       [&](double *P, int slice, int q0, int cnt, const int32_t *lp) {
        double *Jf = P + (size_t)slice * pd;
        int32_t *list = (int32_t *)(Jf + (size_t)slice * jd);
        const int cin = cnt * T.G;
        hipLaunchKernelGGL(k_group_expand, dim3(group_blocks((size_t)cin * N)), dim3(256), 0, s, T, cnt, lp, dX + (size_t)q0 * n,
                           (const int32_t *)nullptr, P, list);
        if (!jac) return c->fcn(c->inner, hip_stream, cin, list, T.N, P, m, out + (size_t)q0 * M);
        if (const int rc = c->jac(c->inner, hip_stream, cin, list, T.N, P, m, Jf)) return rc;
        group_launch_jac(c, m, cnt, Jf, out + (size_t)q0 * M * n, s);
        return 0;
    });
}

int nlh_group_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t M, double *dF)
{
    return group_call(false, ctx, hip_stream, npoints, dprob, n, dX, M, dF);
}

int nlh_group_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t M, double *dJ)
{
    return group_call(true, ctx, hip_stream, npoints, dprob, n, dX, M, dJ);
}

// ---------------------------------------------------------------------------------------------------------------------
// gather, expand, sigma per data set
// ---------------------------------------------------------------------------------------------------------------------
// the launches, on any copy of the tables (nlh_internal.h: the one-call fits use a context's)
void group_gather(const GroupTables *T, hipStream_t s, int ngroup, const double *full, double *x)
{
    hipLaunchKernelGGL(k_group_gather, dim3(group_blocks((size_t)ngroup * T->n)), dim3(256), 0, s, *T, ngroup, full, x);
}

void group_expand(const GroupTables *T, hipStream_t s, int ngroup, const double *x, const int32_t *fail, double *p)
{
    hipLaunchKernelGGL(k_group_expand, dim3(group_blocks((size_t)ngroup * T->G * T->N)), dim3(256), 0, s, *T, ngroup, (const int32_t *)nullptr, x,
                       fail, p, (int32_t *)nullptr);
}

static int group_batch_check(nlh_handle *h, const nlh_group *g, int32_t ngroup, GroupTables *T)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!g || ngroup < 0) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)ngroup * std::max((size_t)g->n, (size_t)g->G * g->N) + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    return group_device_tables(h, g, T);
}

int nlh_group_gather_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dfull, double *dx)
{
    GroupTables T;
    const int rc = group_batch_check(h, g, ngroup, &T);
    if (rc) return rc;
    if (ngroup == 0) return 0;
    if (!dfull || !dx) return NLH_INVALID_INPUT_ERROR;
    group_gather(&T, h->stream, ngroup, dfull, dx);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_group_expand_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dx, double *dfull)
{
    GroupTables T;
    const int rc = group_batch_check(h, g, ngroup, &T);
    if (rc) return rc;
    if (ngroup == 0) return 0;
    if (!dx || !dfull) return NLH_INVALID_INPUT_ERROR;
    group_expand(&T, h->stream, ngroup, dx, nullptr, dfull);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_group_sigma_batch(nlh_handle *h, const nlh_group *g, int32_t ngroup, const double *dsigma, const int32_t *dfail, double *dsigma_full)
{
    GroupTables T;
    const int rc = group_batch_check(h, g, ngroup, &T);
    if (rc) return rc;
    if (ngroup == 0) return 0;
    if (!dsigma || !dsigma_full) return NLH_INVALID_INPUT_ERROR;
    group_expand(&T, h->stream, ngroup, dsigma, dfail, dsigma_full);
    HIPCHK(h, hipGetLastError());
    return 0;
}
