// nlh_launch.h -- the host side of the (point, row) kernels' two workgroup forms (nlh_kernels_place.h), and what the eight
// pairs of wrapping launchers -- parameter maps (nlh_pmap.hip), robust losses (nlh_loss.hip), Poisson fits (nlh_pois.hip),
// global fits (nlh_group.hip), instrument responses (nlh_conv.hip), separable fits (nlh_sep.hip), bins (nlh_bin.hip), pins
// (nlh_pin.hip) -- share: WrapCtx, the base
// of their contexts, with how one is made and what its launchers refuse; the per-stream scratch of a context, its cap, the
// column groups and grid of a column-split Jacobian kernel, and the slice loop of a call.
// Every environment variable is read at every call (tests set them between calls).
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

// The form a launch runs: flat (several points per workgroup) while two points or more fit a workgroup's 256 threads.
// `env` = row | flat forces a form for the sizes it can hold (flat: m <= 256).
static inline bool launch_flat(const char *env, int m)
{
    if (m > 256) return false;
    if (const char *e = getenv(env)) {
        if (!strcmp(e, "row")) return false;
        if (!strcmp(e, "flat")) return true;
    }
    return 256 / m >= 2;
}

// One buffer per stream: calls on one stream are ordered, so the next call's kernels find the last call's done with it;
// calls from several host threads come on different streams and never share one.  A buffer is at most the cap, is kept
// until the context goes and never shrinks: a context holds up to the cap times the streams it was called on.
struct StreamScratch {
    struct Buf { hipStream_t s; void *p; size_t bytes; };
    std::mutex mu;
    std::vector<Buf> bufs;
    // Growing a buffer is hipFree + hipMalloc under the mutex: the free waits for the device, and other threads' calls wait
    // for the mutex meanwhile.  That happens on the first calls of a solve (its largest launch comes early), not per round.
    void *get(hipStream_t s, size_t bytes)
    {
        std::lock_guard<std::mutex> lock(mu);
        Buf *b = nullptr;
        for (Buf &e : bufs) if (e.s == s) b = &e;
        if (!b) { bufs.push_back({s, nullptr, 0}); b = &bufs.back(); }
        if (b->bytes < bytes) {
            if (b->p) hipFree(b->p);
            b->p = nullptr; b->bytes = 0;
            if (hipMalloc(&b->p, bytes) != hipSuccess) { b->p = nullptr; return nullptr; }
            b->bytes = bytes;
        }
        return b->p;
    }
    void free_all()                                              // (hipFree waits for the work that still uses it)
    {
        for (Buf &b : bufs) hipFree(b.p);
        bufs.clear();
    }
};

// The compute units of a device (1 when the runtime does not say): what jac_grid and the convolution deal columns over.
static inline int device_cus(int device)
{
    int cus = 0;
    return hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0 ? cus : 1;
}

// The base of the eight wrapping contexts: what a layer around an inner launcher pair (fcn, jac -- NULL: none --, inner) holds
// whatever it computes.  Each nlh_*_ctx derives from it alone and adds its own fields, so a context's address is its base's:
// the launchers read magic -- one value per kind -- through the void * they are handed, and nlh_model.hip and nlh_fit.hip
// hold a layer of any kind as a WrapCtx * (nlh_internal.h: wrap_layer, wrap_release).  tables: the kind's own device
// allocation, if it has one.
struct WrapCtx {
    uint32_t magic = 0;
    int device = 0, cus = 1;
    nlh_device_vecfcn fcn = nullptr;
    nlh_device_jacfcn jac = nullptr;
    void *inner = nullptr;
    void *tables = nullptr;
    StreamScratch scratch;             // kept until wrap_release
    virtual ~WrapCtx() = default;      // (wrap_release deletes a context of any kind through this base)
};

// The common part of every nlh_*_wrap, after the kind's own refusals: a context of the kind on the handle's device.
template <class Ctx>
static int wrap_new(nlh_handle *h, uint32_t magic, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner, Ctx **out)
{
    static_assert(std::is_base_of<WrapCtx, Ctx>::value, "a wrapping context derives from WrapCtx");
    HIPCHK(h, hipSetDevice(h->device));
    Ctx *c = new Ctx();
    c->magic = magic; c->device = h->device; c->cus = device_cus(h->device);
    c->fcn = fcn; c->jac = jac; c->inner = inner;
    *out = c;
    return 0;
}

// What the launchers of every kind refuse before any launch, in this order.  wrap_ctx: the live context of the kind with an
// inner fcn behind ctx, or NULL.  wrap_refused: no such context, or `ok` -- what else the kind asks of its context, its shape
// check, the caller's pointers; the caller's expression, which reads c only where there is one -- fails:
// NLH_INVALID_INPUT_ERROR; a Jacobian asked for without an inner one: NLH_UNDEFINED_FUNCTION_ERROR; no points: 0.  true: the
// call ends with *rc.
template <class Ctx> static inline Ctx *wrap_ctx(void *ctx, uint32_t magic)
{
    Ctx *c = (Ctx *)ctx;
    return c && c->magic == magic && c->fcn ? c : nullptr;
}
static inline bool wrap_refused(const WrapCtx *c, bool ok, bool jac, int npoints, int *rc)
{
    if (!c || !ok) *rc = NLH_INVALID_INPUT_ERROR;
    else if (jac && !c->jac) *rc = NLH_UNDEFINED_FUNCTION_ERROR;
    else if (npoints <= 0) *rc = 0;
    else return false;
    return true;
}

// Scratch bytes per call, so per stream; beyond it the points go in slices.  `env` asks for less.
static inline size_t scratch_cap(const char *env)
{
    size_t cap = (size_t)1 << 30;
    if (const char *e = getenv(env)) {
        const long long v = atoll(e);
        if (v > 0 && (size_t)v < cap) cap = (size_t)v;
    }
    return cap;
}

// The grid of a column-split Jacobian kernel: grid.x workgroups over (point, row block) -- flat: ppw points each --, grid.y
// groups of cpg of the n columns.  A compute unit holds eight workgroups of 256 threads; below four per unit -- four waves per
// SIMD, half of what it can hold -- a streaming kernel does not keep enough loads in flight, so the columns are dealt over
// gridDim.y until the launch has that many (or a column per group).  `split_env` overrides the number of groups.
struct JacGrid {
    bool flat;
    int ppw, nblk, cpg;
    dim3 grid;
};
static inline JacGrid jac_grid(const char *form_env, const char *split_env, int cus, int m, int n, int npoints)
{
    JacGrid g;
    g.flat = launch_flat(form_env, m);
    g.ppw = g.flat ? 256 / m : 1; g.nblk = g.flat ? 1 : (m + 255) / 256;
    const size_t wgs = g.flat ? (size_t)(npoints + g.ppw - 1) / g.ppw : (size_t)npoints * g.nblk;
    size_t groups = 1;
    const size_t want = (size_t)4 * cus;
    if (wgs < want) groups = (want + wgs - 1) / wgs;
    if (const char *e = getenv(split_env)) {
        const int v = atoi(e);
        if (v >= 1) groups = (size_t)v;
    }
    groups = std::min<size_t>(groups, (size_t)n);
    g.cpg = (n + (int)groups - 1) / (int)groups;
    g.grid = dim3((unsigned)wgs, (unsigned)((n + g.cpg - 1) / g.cpg));
    return g;
}

// The slice loop of a wrapping launcher's call on npoints points of m rows.  A point needs `doubles` doubles of the
// context's scratch, and a list entry when the caller passed no dprob; a call takes as many points at a time as the cap
// holds.  body(base, slice, q0, cnt, lp) works on points q0 .. q0 + cnt: base the scratch (doubles first, slice points of
// them; null when nothing is needed), lp their problem list.  A non-zero return ends the call with it.
template <class Body>
static int wrap_slices(StreamScratch &scratch, const char *cap_env, int device, hipStream_t s, size_t doubles, int npoints, int m,
                       const int32_t *dprob, const Body &body)
{
    const size_t per = sizeof(double) * doubles + (dprob ? 0 : sizeof(int32_t));
    const size_t cap = scratch_cap(cap_env);
    const int slice = per ? (int)std::max<size_t>(1, std::min<size_t>((size_t)npoints, cap / per)) : npoints;
    if ((size_t)slice * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (hipSetDevice(device) != hipSuccess) return NLH_ERR_HIP;
    char *base = nullptr;
    if (per) {
        base = (char *)scratch.get(s, (size_t)slice * per + 64);
        if (!base) return NLH_OUT_OF_MEMORY_ERROR;
    }
    int32_t *list = (int32_t *)(base + sizeof(double) * (size_t)slice * doubles);
    for (int q0 = 0; q0 < npoints; q0 += slice) {
        const int cnt = std::min(slice, npoints - q0);
        const int32_t *lp = dprob ? dprob + q0 : list;
        if (!dprob) hipLaunchKernelGGL(k_wrap_iota, dim3((cnt + 255) / 256), dim3(256), 0, s, cnt, q0, list);
        if (const int rc = body((double *)base, slice, q0, cnt, lp)) return rc;
    }
    return 0;
}
