// nlh_model.hip -- several GPUs behind the boundary (device sets) and device residual models behind host arrays: what
// a Fortran / C caller without device pointers uses to reach the batched device path (the extension of vecfcn_helper
// SURVEY.md section 7 asks for: set_device_model).
#include "nlh_internal.h"


// ===========================================================================
// Device residual models behind host arrays: what a Fortran / C caller without device pointers uses to reach the
// batched device path (the extension of vecfcn_helper SURVEY.md section 7 asks for: set_device_model).
// A model owns device copies of the data of nprob dense-quadratic problems (SURVEY 8(d) family:
// r = (u + gamma u u) - b, u = A x); the solves stage x / fvec through the handle's buffers.
// ===========================================================================
// ---- several GPUs behind the boundary (SURVEY 8(b) `nlx_init(device, comm)`, 8(e)) ---------------------------------
// A device set owns one handle -- own non-blocking stream, own workspaces -- per entry of its device list.  A model
// created on a set is DEALT over the entries block-cyclically (problem k -> entry k mod ndev: iteration counts differ
// per problem) and a solve on it runs one host thread per entry: independent problems, no collective, the same bits as
// on one device (a problem's arithmetic never depends on its batch).
struct nlh_device_set {
    std::vector<nlh_handle *> handles;
    std::string err;
    std::atomic<int> refs{1};          // the creator's reference + one per model dealt over the set: nlh_device_set_destroy
};                                     // only drops the creator's, the handles go when the last model has gone too

int nlh_device_set_create(nlh_device_set **out, const int32_t *devices, int32_t ndev)
{
    if (!out) return NLH_ERR_BAD_HANDLE;
    *out = nullptr;
    const int visible = nlh_device_count();
    if (visible <= 0) return NLH_ERR_NO_DEVICE;
    std::vector<int32_t> ids;
    if (!devices || ndev <= 0) for (int d = 0; d < visible; ++d) ids.push_back(d);
    else ids.assign(devices, devices + ndev);
    for (int32_t d : ids) if (d < 0 || d >= visible) return NLH_INVALID_INPUT_ERROR;
    nlh_device_set *set = new nlh_device_set();
    for (int32_t d : ids) {
        nlh_handle *h = nullptr;
        hipStream_t st = nullptr;
        int rc = hipSetDevice(d) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess ? 0 : NLH_ERR_HIP;
        if (!rc) rc = nlh_create(&h, d, st);
        if (rc) {
            if (st) hipStreamDestroy(st);
            nlh_device_set_destroy(set);
            return rc;
        }
        h->own_stream = true;
        set->handles.push_back(h);
    }
    *out = set;
    return 0;
}

static void device_set_release(nlh_device_set *set)
{
    if (!set || set->refs.fetch_sub(1) != 1) return;
    for (auto *h : set->handles) nlh_destroy(h);
    delete set;
}

void nlh_device_set_destroy(nlh_device_set *set) { device_set_release(set); }

int32_t nlh_device_set_size(const nlh_device_set *set) { return set ? (int32_t)set->handles.size() : 0; }

nlh_handle *nlh_device_set_handle(nlh_device_set *set, int32_t i)
{
    return (set && i >= 0 && i < (int32_t)set->handles.size()) ? set->handles[i] : nullptr;
}

const char *nlh_device_set_last_error(const nlh_device_set *set) { return set ? set->err.c_str() : "null device set"; }

// ---- device residual models behind host arrays ------------------------------------------------------------------------
struct DqPart {                        // the share of one device: problems first, first + stride, ... (cnt of them)
    int32_t device = 0, cnt = 0, first = 0, stride = 1;
    nlh_handle *h = nullptr;           // the set's handle for this share; NULL: the caller's handle (single-device model)
    double *dA = nullptr, *db = nullptr, *dx = nullptr, *df = nullptr;
};

struct nlh_dq_model {
    int32_t nprob, m, n;
    double gamma;
    nlh_device_set *set = nullptr;     // not owned
    std::vector<DqPart> parts;
    // a USER'S device residual instead of the dense-quadratic family (nlh_device_fcn_model_create): launchers + context,
    // no data of the library's own; the solves go through the *_batch_device_h entry points on the caller's handle
    nlh_device_vecfcn ufcn = nullptr;
    nlh_device_jacfcn ujac = nullptr;
    void *uctx = nullptr;
    // The launcher-backed kinds the library makes itself: uctx is the kind's context below, which the model owns
    // together with the device copy of the host arrays behind it -- one allocation, owned, on owned_device.
    void *owned = nullptr;
    int owned_device = 0;
    // a built-in curve model (nlh_curve_model_create): t, y, w
    nlh_curve_ctx *curve = nullptr;
    // a formula model (nlh_expr_model_create): t, y, w, and a copy of the program
    nlh_expr_ctx *expr = nullptr;
    nlh_expr *expr_prog = nullptr;
    // a model around another model's launchers (nlh_{pmap,loss,pois,conv,group,sep}_model_create): uctx is this layer, the
    // wrapping context of its kind; owned: the arrays behind it -- full parameters, scales, counts and mask, data and taps
    WrapCtx *layer = nullptr;
};

// Host arrays, one after the other, into one device allocation on the handle's device; synchronised (nlh_internal.h).
int nlh_upload(nlh_handle *h, const char *what, std::initializer_list<HostPart> parts, void **base)
{
    *base = nullptr;
    HIPCHK(h, hipSetDevice(h->device));
    size_t bytes = 0;
    for (const HostPart &p : parts) bytes += p.bytes;
    char *d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) {
        h->err = std::string("hipMalloc (") + what + ")";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    hipError_t e = hipSuccess;
    size_t at = 0;
    for (const HostPart &p : parts) {
        if (e == hipSuccess && p.bytes) e = hipMemcpyAsync(d + at, p.p, p.bytes, hipMemcpyHostToDevice, h->stream);
        at += p.bytes;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        hipFree(d);
        h->err = std::string("hipMemcpy (") + what + "): " + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    *base = d;
    return 0;
}

int nlh_device_fcn_model_create(int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn, void *ctx,
                                nlh_dq_model **out)
{
    if (!out || nprob < 1 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    *out = nullptr;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_dq_model *md = new nlh_dq_model();
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = 0.0;
    md->ufcn = fcn; md->ujac = jacfcn; md->uctx = ctx;
    *out = md;
    return 0;
}

static int model_part_upload(nlh_handle *h, const nlh_dq_model *md, DqPart &pt, const double *A, const double *b)
{
    const int m = md->m, n = md->n;
    const size_t mn = (size_t)m * n, cnt = (size_t)pt.cnt;
    HIPCHK(h, hipSetDevice(pt.device));
    double *base = nullptr;
    if (hipMalloc(&base, sizeof(double) * cnt * (mn + 2 * (size_t)m + n)) != hipSuccess) {
        h->err = "hipMalloc (device model)";
        return NLH_OUT_OF_MEMORY_ERROR;
    }
    pt.dA = base; pt.db = base + cnt * mn; pt.df = pt.db + cnt * m; pt.dx = pt.df + cnt * m;
    hipError_t e = hipSuccess;
    if (pt.stride == 1) {
        e = hipMemcpyAsync(pt.dA, A + (size_t)pt.first * mn, sizeof(double) * cnt * mn, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(pt.db, b + (size_t)pt.first * m, sizeof(double) * cnt * m, hipMemcpyHostToDevice, h->stream);
    } else {
        for (size_t i = 0; i < cnt && e == hipSuccess; ++i) {
            const size_t k = (size_t)pt.first + i * pt.stride;
            e = hipMemcpyAsync(pt.dA + i * mn, A + k * mn, sizeof(double) * mn, hipMemcpyHostToDevice, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(pt.db + i * m, b + k * m, sizeof(double) * m, hipMemcpyHostToDevice, h->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        hipFree(base);
        pt.dA = nullptr;
        h->err = std::string("hipMemcpy (device model): ") + hipGetErrorString(e);
        return NLH_ERR_HIP;
    }
    return 0;
}

int nlh_dq_model_create(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, const double *A, const double *b,
                        double gamma, nlh_dq_model **out)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !A || !b || nprob < 1 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    *out = nullptr;
    nlh_dq_model *md = new nlh_dq_model();
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = gamma;
    DqPart pt;
    pt.device = h->device; pt.cnt = nprob;
    const int rc = model_part_upload(h, md, pt, A, b);
    if (rc) { delete md; return rc; }
    md->parts.push_back(pt);
    *out = md;
    return 0;
}

int nlh_dq_model_create_on(nlh_device_set *set, int32_t nprob, int32_t m, int32_t n, const double *A, const double *b,
                           double gamma, nlh_dq_model **out)
{
    if (!set || set->handles.empty()) return NLH_ERR_BAD_HANDLE;
    if (!out || !A || !b || nprob < 1 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    *out = nullptr;
    nlh_dq_model *md = new nlh_dq_model();
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = gamma; md->set = set;
    set->refs.fetch_add(1);                                      // released by nlh_dq_model_destroy
    const int nd = (int)set->handles.size();
    for (int d = 0; d < nd; ++d) {
        DqPart pt;
        pt.h = set->handles[d];
        pt.device = pt.h->device; pt.first = d; pt.stride = nd;
        pt.cnt = d < nprob ? (nprob - d + nd - 1) / nd : 0;
        if (pt.cnt > 0) {
            const int rc = model_part_upload(pt.h, md, pt, A, b);
            if (rc) { set->err = pt.h->err; nlh_dq_model_destroy(md); return rc; }
        }
        md->parts.push_back(pt);
    }
    *out = md;
    return 0;
}

// A built-in curve model: device copies of the host arrays t [nprob][m] (shared_t: [m]), y, w (NULL: no weights) and the
// context of the launchers nlh_curve_device_fcn / nlh_curve_device_jac (nlh_curve.hip), all owned by the model.
int nlh_curve_model_create(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *t,
                           int32_t shared_t, const double *y, const double *w, int32_t analytic, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t n = nlh_curve_nparams(kind, ncomp, nbase);
    if (!out || n < 0 || nprob < 1 || m < 1 || !t || !y) return NLH_INVALID_INPUT_ERROR;
    if (m < n) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    const size_t pm = (size_t)nprob * m, tm = shared_t ? (size_t)m : pm;
    double *base = nullptr;
    if (const int rc = nlh_upload(h, "curve model", {{t, sizeof(double) * tm}, {y, sizeof(double) * pm}, {w, w ? sizeof(double) * pm : 0}},
                                  (void **)&base)) return rc;
    nlh_curve_ctx *c = new nlh_curve_ctx();
    c->kind = kind; c->ncomp = ncomp; c->nbase = nbase; c->shared_t = shared_t != 0; c->m = m;
    c->dt = base; c->dy = base + tm; c->dw = w ? base + tm + pm : nullptr;
    nlh_dq_model *md = new nlh_dq_model();
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = 0.0;
    md->ufcn = nlh_curve_device_fcn; md->ujac = analytic ? nlh_curve_device_jac : nullptr; md->uctx = c;
    md->curve = c; md->owned = base; md->owned_device = h->device;
    *out = md;
    return 0;
}

// A formula model: the same, with a copy of the compiled program (the caller's nlh_expr may be destroyed at once).
int nlh_expr_model_create(nlh_handle *h, const nlh_expr *e, int32_t nprob, int32_t m, const double *t, int32_t shared_t, const double *y,
                          const double *w, int32_t analytic, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !e || nprob < 1 || m < 1 || !t || !y) return NLH_INVALID_INPUT_ERROR;
    const int32_t n = e->prog.nparams;
    if (m < n) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    const size_t pm = (size_t)nprob * m, stride = shared_t ? (size_t)m : pm, tm = stride * e->prog.nvar;
    double *base = nullptr;
    if (const int rc = nlh_upload(h, "formula model", {{t, sizeof(double) * tm}, {y, sizeof(double) * pm}, {w, w ? sizeof(double) * pm : 0}},
                                  (void **)&base)) return rc;
    nlh_dq_model *md = new nlh_dq_model();
    md->expr_prog = new nlh_expr(*e);
    nlh_expr_ctx *c = new nlh_expr_ctx();
    c->e = md->expr_prog; c->shared_t = shared_t != 0; c->m = m; c->dt_stride = (int64_t)stride;
    c->dt = base; c->dy = base + tm; c->dw = w ? base + tm + pm : nullptr;
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = 0.0;
    md->ufcn = nlh_expr_device_fcn; md->ujac = analytic ? nlh_expr_device_jac : nullptr; md->uctx = c;
    md->expr = c; md->owned = base; md->owned_device = h->device;
    *out = md;
    return 0;
}

// The model around an inner model's launchers: nprob problems of m rows over n unknowns through the wrapping pair (fcn, jac)
// on the context `layer`, which the model owns with `owned` on `device`.  It has a Jacobian launcher if the inner model has
// (a separable model's always has: nlh_sep_wrap refuses an inner model without).
static nlh_dq_model *layer_model(const nlh_dq_model *inner, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                                 void *layer, void *owned, int device)
{
    nlh_dq_model *md = new nlh_dq_model();
    md->nprob = nprob; md->m = m; md->n = n; md->gamma = 0.0;
    md->ufcn = fcn; md->ujac = inner->ujac ? jac : nullptr; md->uctx = layer;
    md->layer = wrap_layer(layer); md->owned = owned; md->owned_device = device;
    return md;
}

// A model of the free unknowns of a parameter map over a launcher-backed inner model (nlh_pmap.hip: the wrapping launchers).
int nlh_pmap_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_pmap *pm, const double *full, int32_t shared_full,
                          nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !pm || !full || !inner->ufcn) return NLH_INVALID_INPUT_ERROR;
    int32_t N, n;
    nlh_pmap_shape(pm, &N, &n, nullptr);
    if (N != inner->n) return NLH_INVALID_INPUT_ERROR;
    const size_t cnt = (shared_full ? 1 : (size_t)inner->nprob) * N;
    double *base = nullptr;
    if (const int urc = nlh_upload(h, "mapped model", {{full, sizeof(double) * cnt}}, (void **)&base)) return urc;
    nlh_pmap_ctx *pc = nullptr;
    const int rc = nlh_pmap_wrap(h, pm, inner->ufcn, inner->ujac, inner->uctx, base, shared_full, &pc);
    if (rc) { hipFree(base); return rc; }
    *out = layer_model(inner, inner->nprob, inner->m, n, nlh_pmap_device_fcn, nlh_pmap_device_jac, pc, base, h->device);
    return 0;
}

// A model with a robust loss over a launcher-backed inner model (nlh_loss.hip: the wrapping launchers).
int nlh_loss_model_create(nlh_handle *h, const nlh_dq_model *inner, int32_t kind, const double *scale, int32_t shared_scale,
                          nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !inner->ufcn || !nlh_loss_kind_ok(kind)) return NLH_INVALID_INPUT_ERROR;
    double *base = nullptr;
    const int urc = nlh_loss_scale_upload(h, kind, scale, shared_scale ? 1 : (size_t)inner->nprob, &base);
    if (urc) return urc;
    nlh_loss_ctx *lc = nullptr;
    const int rc = nlh_loss_wrap(h, kind, base, shared_scale, inner->ufcn, inner->ujac, inner->uctx, &lc);
    if (rc) { hipFree(base); return rc; }
    *out = layer_model(inner, inner->nprob, inner->m, inner->n, nlh_loss_device_fcn, nlh_loss_device_jac, lc, base, h->device);
    return 0;
}

// A convolved model over a launcher-backed inner model created WITHOUT weights (nlh_conv.hip: the wrapping launchers).
int nlh_conv_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_conv *cv, const double *y, const double *w, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !inner->ufcn || !y || !nlh_conv_ok(cv)) return NLH_INVALID_INPUT_ERROR;
    const size_t pm = (size_t)inner->nprob * inner->m, kd = (size_t)cv->L * (cv->shared_k ? 1 : (size_t)inner->nprob);
    if (!nlh_conv_data_ok(cv, y, (size_t)inner->nprob, (size_t)inner->m)) return NLH_INVALID_INPUT_ERROR;
    double *base = nullptr;
    if (const int urc = nlh_upload(h, "convolved model", {{y, sizeof(double) * pm}, {cv->k, sizeof(double) * kd}, {w, w ? sizeof(double) * pm : 0}},
                                   (void **)&base)) return urc;
    nlh_conv dcv = *cv;
    dcv.k = base + pm;
    nlh_conv_ctx *cc = nullptr;
    const int rc = nlh_conv_wrap(h, &dcv, base, w ? base + pm + kd : nullptr, inner->ufcn, inner->ujac, inner->uctx, &cc);
    if (rc) { hipFree(base); return rc; }
    *out = layer_model(inner, inner->nprob, inner->m, inner->n, nlh_conv_device_fcn, nlh_conv_device_jac, cc, base, h->device);
    return 0;
}

// A Poisson model over a launcher-backed inner model created WITHOUT weights (nlh_pois.hip: the wrapping launchers).
int nlh_pois_model_create(nlh_handle *h, const nlh_dq_model *inner, const double *y, const double *w, double mu_floor, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !inner->ufcn || !y || !nlh_pois_floor_ok(mu_floor)) return NLH_INVALID_INPUT_ERROR;
    const size_t pm = (size_t)inner->nprob * inner->m;
    if (!nlh_pois_data_ok(y, w, pm)) return NLH_INVALID_INPUT_ERROR;
    double *base = nullptr;
    if (const int urc = nlh_upload(h, "Poisson model", {{y, sizeof(double) * pm}, {w, w ? sizeof(double) * pm : 0}}, (void **)&base)) return urc;
    nlh_pois_ctx *qc = nullptr;
    const int rc = nlh_pois_wrap(h, base, w ? base + pm : nullptr, mu_floor, inner->ufcn, inner->ujac, inner->uctx, &qc);
    if (rc) { hipFree(base); return rc; }
    *out = layer_model(inner, inner->nprob, inner->m, inner->n, nlh_pois_device_fcn, nlh_pois_device_jac, qc, base, h->device);
    return 0;
}

// A model of the outer unknowns of a group over a launcher-backed inner model (nlh_group.hip: the wrapping launchers): every
// G consecutive problems of the inner model are one problem of G m rows.
int nlh_group_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_group *g, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !g || !inner->ufcn) return NLH_INVALID_INPUT_ERROR;
    int32_t N, G, n;
    nlh_group_shape(g, &N, nullptr, &G, &n);
    if (N != inner->n || inner->nprob % G != 0 || (int64_t)G * inner->m > 0x7fffffff) return NLH_INVALID_INPUT_ERROR;
    nlh_group_ctx *gc = nullptr;
    const int rc = nlh_group_wrap(h, g, inner->ufcn, inner->ujac, inner->uctx, &gc);
    if (rc) return rc;
    *out = layer_model(inner, inner->nprob / G, G * inner->m, n, nlh_group_device_fcn, nlh_group_device_jac, gc, nullptr, h->device);
    return 0;
}

// A model of the nonlinear unknowns of a separable object over a launcher-backed inner model that has a Jacobian launcher
// (nlh_sep.hip: the projecting launchers).
int nlh_sep_model_create(nlh_handle *h, const nlh_dq_model *inner, const nlh_sep *sp, nlh_dq_model **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !inner || !sp || !inner->ufcn) return NLH_INVALID_INPUT_ERROR;
    int32_t N, n;
    nlh_sep_shape(sp, &N, nullptr, &n);
    if (N != inner->n) return NLH_INVALID_INPUT_ERROR;
    nlh_sep_ctx *sc = nullptr;
    const int rc = nlh_sep_wrap(h, sp, inner->ufcn, inner->ujac, inner->uctx, &sc);
    if (rc) return rc;
    *out = layer_model(inner, inner->nprob, inner->m, n, nlh_sep_device_fcn, nlh_sep_device_jac, sc, nullptr, h->device);
    return 0;
}

void nlh_dq_model_destroy(nlh_dq_model *md)
{
    if (!md) return;
    wrap_release(md->layer);
    delete md->expr;
    delete md->expr_prog;
    if (md->owned) { hipSetDevice(md->owned_device); hipFree(md->owned); }
    delete md->curve;
    for (auto &pt : md->parts)
        if (pt.dA) { hipSetDevice(pt.device); hipFree(pt.dA); }
    device_set_release(md->set);
    delete md;
}

void nlh_dq_model_shape(const nlh_dq_model *md, int32_t *nprob, int32_t *m, int32_t *n)
{
    if (nprob) *nprob = md ? md->nprob : 0;
    if (m) *m = md ? md->m : 0;
    if (n) *n = md ? md->n : 0;
}

int32_t nlh_dq_model_device_count(const nlh_dq_model *md) { return md ? (int32_t)md->parts.size() : 0; }

// One operation on every share of a model.  x [nprob][n] goes in (and, when x_out, comes back), per_part works on the
// share's device buffers (pt.dx in / out, pt.df out) and fills the share's ib / status rows; f [nprob][m] comes back.
// A single-device model runs on the caller's handle and stream; a model on a device set runs one host thread per share.
typedef std::function<int(nlh_handle *, const DqPart &, nlh_iteration_behavior *, int32_t *)> PartOp;

static int model_part_run(nlh_handle *h, const nlh_dq_model *md, const DqPart &pt, double *x, bool x_out, double *f,
                          nlh_iteration_behavior *ib, int32_t *status, const PartOp &op)
{
    if (pt.cnt == 0) return 0;
    const size_t n = md->n, m = md->m, cnt = pt.cnt;
    HIPCHK(h, hipSetDevice(pt.device));
    if (pt.stride == 1) {                                        // contiguous share: straight from / to the caller's arrays
        double *xs = x + (size_t)pt.first * n, *fs = f + (size_t)pt.first * m;
        HIPCHK(h, hipMemcpyAsync(pt.dx, xs, sizeof(double) * cnt * n, hipMemcpyHostToDevice, h->stream));
        const int rc = op(h, pt, ib ? ib + pt.first : nullptr, status ? status + pt.first : nullptr);
        if (rc) return rc;
        if (x_out) HIPCHK(h, hipMemcpyAsync(xs, pt.dx, sizeof(double) * cnt * n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(fs, pt.df, sizeof(double) * cnt * m, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return 0;
    }
    // the broadcast / gather ends of the dealt batch, staged through a PINNED buffer of the share's handle (its own, apart
    // from the one the solvers keep their read-back state in: a pageable staging vector makes every one of these copies a
    // synchronous bounce through the runtime's own pinned pool)
    if (int rcp = ensure_staging(h, sizeof(double) * cnt * (n + m))) return rcp;
    double *xs = (double *)h->staging, *fs = xs + cnt * n;
    std::vector<nlh_iteration_behavior> ibs(ib ? cnt : 0);
    std::vector<int32_t> sts(status ? cnt : 0);
    for (size_t i = 0; i < cnt; ++i) memcpy(&xs[i * n], x + ((size_t)pt.first + i * pt.stride) * n, sizeof(double) * n);
    HIPCHK(h, hipMemcpyAsync(pt.dx, xs, sizeof(double) * cnt * n, hipMemcpyHostToDevice, h->stream));
    const int rc = op(h, pt, ib ? ibs.data() : nullptr, status ? sts.data() : nullptr);
    if (rc) return rc;
    if (x_out) HIPCHK(h, hipMemcpyAsync(xs, pt.dx, sizeof(double) * cnt * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(fs, pt.df, sizeof(double) * cnt * m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < cnt; ++i) {
        const size_t k = (size_t)pt.first + i * pt.stride;
        if (x_out) memcpy(x + k * n, &xs[i * n], sizeof(double) * n);
        memcpy(f + k * m, &fs[i * m], sizeof(double) * m);
        if (ib) ib[k] = ibs[i];
        if (status) status[k] = sts[i];
    }
    return 0;
}

static int model_run(nlh_handle *h, const nlh_dq_model *md, double *x, bool x_out, double *f, nlh_iteration_behavior *ib,
                     int32_t *status, const PartOp &op)
{
    if (!md || !x || !f) return NLH_INVALID_INPUT_ERROR;
    if (!md->set) {
        if (!h) return NLH_ERR_BAD_HANDLE;
        if (h->device != md->parts[0].device) {                  // the model's buffers live on the device of the handle that
            h->err = "device model used with a handle on another device";   // created it: another device's stream cannot run it
            return NLH_INVALID_INPUT_ERROR;
        }
        return model_part_run(h, md, md->parts[0], x, x_out, f, ib, status, op);
    }
    const int nd = (int)md->parts.size();
    std::vector<int> rcs(nd, 0);
    std::vector<std::thread> pool;
    for (int d = 0; d < nd; ++d)
        pool.emplace_back([&, d]() {
            rcs[d] = model_part_run(md->parts[d].h, md, md->parts[d], x, x_out, f, ib, status, op);
        });
    for (auto &t : pool) t.join();
    for (int d = 0; d < nd; ++d)
        if (rcs[d]) { md->set->err = md->parts[d].h->err; return rcs[d]; }
    return 0;
}

// vecfcn of the model: f = F(x) for every problem, host arrays x [nprob][n], f [nprob][m].
int nlh_dq_model_eval(nlh_handle *h, const nlh_dq_model *md, const double *x, double *f)
{
    if (!md) return NLH_INVALID_INPUT_ERROR;
    if (md->ufcn) {                                              // a user's device function: one point per problem
        if (!h) return NLH_ERR_BAD_HANDLE;
        if (!x || !f) return NLH_INVALID_INPUT_ERROR;
        const size_t xbytes = sizeof(double) * (size_t)md->nprob * md->n, fbytes = sizeof(double) * (size_t)md->nprob * md->m;
        return staged_call(h, {{const_cast<double *>(x), xbytes, true, false, &h->xdev}, {f, fbytes, false, true, &h->fdev}},
                           [&](void *const *d) {
                               return residual_eval(h, ResidualSource::launchers(md->ufcn, md->ujac, md->uctx), md->nprob, md->m, md->n,
                                                    (const double *)d[0], (double *)d[1], nullptr, nullptr, -1);
                           });
    }
    return model_run(h, md, const_cast<double *>(x), false, f, nullptr, nullptr,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *, int32_t *) -> int {
                         launch_dq_residual(ph, pt.cnt, md->m, md->n, pt.dA, pt.db, md->gamma, pt.dx, pt.df, nullptr, nullptr, -1);
                         HIPCHK(ph, hipGetLastError());          // a launch that failed must not return stale residuals as success
                         return 0;
                     });
}

// least_squares_solver%solve on every problem of the model (nlh_dq_lm_solve_batch behind host arrays).
int nlh_dq_model_lm_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, double *x, double *fvec,
                          nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    const nlh_options oq = silent_in_batch(*o, md->nprob);      // (a share of a dealt batch would print from its host thread)
    o = &oq;
    if (md->ufcn) return nlh_lm_solve_batch_device_h(h, o, md->nprob, md->m, md->n, md->ufcn, md->ujac, md->uctx, x, fvec, ib, status);
    return model_run(h, md, x, true, fvec, ib, status,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *pib, int32_t *pst) -> int {
                         return nlh_dq_lm_solve_batch(ph, o, pt.cnt, md->m, md->n, pt.dA, pt.db, md->gamma, pt.dx, pt.df, pib, pst);
                     });
}

// Parameter covariance at x for every problem of the model (nlh_lm_covariance_batch_device_h on each share; the built-in
// family through its launcher nlh_dq_device_fcn, forward differences as its LM solve uses).  Host arrays: x [nprob][n],
// cov [nprob][n][n], sigma [nprob][n], rank / chi2 [nprob]; sigma, rank, chi2 may be NULL.
int nlh_dq_model_lm_covariance(nlh_handle *h, const nlh_dq_model *md, const double *x, int32_t scaled, double tol, double *cov,
                               double *sigma, int32_t *rank, double *chi2)
{
    if (!md || !x || !cov) return NLH_INVALID_INPUT_ERROR;
    const int32_t m = md->m, n = md->n;
    if (md->ufcn)
        return nlh_lm_covariance_batch_device_h(h, md->nprob, m, n, md->ufcn, md->ujac, md->uctx, x, scaled, tol, cov, sigma, rank, chi2);
    if (!md->set && !h) return NLH_ERR_BAD_HANDLE;
    const size_t nn = (size_t)n * n;
    for (const DqPart &pt : md->parts) {                         // the shares one after the other: each on its own handle
        if (pt.cnt == 0) continue;
        nlh_handle *ph = pt.h ? pt.h : h;
        nlh_dq_device_ctx c;
        c.dA = pt.dA; c.db = pt.db; c.gamma = md->gamma;
        int rc;
        if (pt.stride == 1) {
            const size_t f = (size_t)pt.first;
            rc = nlh_lm_covariance_batch_device_h(ph, pt.cnt, m, n, nlh_dq_device_fcn, nullptr, &c, x + f * n, scaled, tol, cov + f * nn,
                                                  sigma ? sigma + f * n : nullptr, rank ? rank + f : nullptr, chi2 ? chi2 + f : nullptr);
        } else {
            const size_t cnt = (size_t)pt.cnt;
            std::vector<double> xs(cnt * n), cs(cnt * nn), ss(cnt * n), qs(cnt);
            std::vector<int32_t> rs(cnt);
            for (size_t i = 0; i < cnt; ++i) memcpy(&xs[i * n], x + ((size_t)pt.first + i * pt.stride) * n, sizeof(double) * n);
            rc = nlh_lm_covariance_batch_device_h(ph, pt.cnt, m, n, nlh_dq_device_fcn, nullptr, &c, xs.data(), scaled, tol, cs.data(),
                                                  ss.data(), rs.data(), qs.data());
            for (size_t i = 0; i < cnt && !rc; ++i) {
                const size_t k = (size_t)pt.first + i * pt.stride;
                memcpy(cov + k * nn, &cs[i * nn], sizeof(double) * nn);
                if (sigma) memcpy(sigma + k * n, &ss[i * n], sizeof(double) * n);
                if (rank) rank[k] = rs[i];
                if (chi2) chi2[k] = qs[i];
            }
        }
        if (rc) { if (md->set) md->set->err = ph->err; return rc; }
    }
    return 0;
}

// The model's values at x and their standard deviations under the parameter covariance cov (nlh_propagate_batch_device_h:
// the model's jacfcn if it has one, forward differences otherwise).  Host arrays: x [nprob][n], cov [nprob][n][n], noise
// [nprob] or NULL, val [nprob][m] or NULL, sd [nprob][m].  Launcher-backed models only: the built-in dense-quadratic family
// -- the only one a device set deals over several devices -- is refused, as the wrapping models refuse it.
int nlh_dq_model_propagate(nlh_handle *h, const nlh_dq_model *md, const double *x, const double *cov, const double *noise, double *val,
                           double *sd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!md || !md->ufcn || !x || !cov || !sd) return NLH_INVALID_INPUT_ERROR;
    return nlh_propagate_batch_device_h(h, md->nprob, md->m, md->n, md->ufcn, md->ujac, md->uctx, x, cov, noise, val, sd);
}

// newton_solver%solve on every (square) problem of the model; analytic != 0: the model's own Jacobian
// J(i,j) = (1 + 2 gamma u_i) A(i,j) plays the role of a jacobianfcn, otherwise forward differences.
int nlh_dq_model_newton_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, int32_t analytic, double *x,
                              double *fvec, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    const nlh_options oq = silent_in_batch(*o, md->nprob);
    o = &oq;
    if (md->m != md->n) return NLH_INVALID_INPUT_ERROR;         // src/nonlin_solve.f90:519
    if (md->ufcn)                                                // (analytic: whether to use the user's jacobianfcn launcher)
        return nlh_newton_solve_batch_device_h(h, o, md->nprob, md->n, md->ufcn, analytic ? md->ujac : nullptr, md->uctx, x, fvec, ib, status);
    return model_run(h, md, x, true, fvec, ib, status,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *pib, int32_t *pst) -> int {
                         return nlh_dq_newton_solve_batch(ph, o, pt.cnt, md->n, pt.dA, pt.db, md->gamma, analytic, pt.dx, pt.df, pib, pst);
                     });
}

// quasi_newton_solver%solve on every (square) problem of the model.
int nlh_dq_model_quasi_newton_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, int32_t jdelta,
                                    int32_t analytic, double *x, double *fvec, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    const nlh_options oq = silent_in_batch(*o, md->nprob);
    o = &oq;
    if (md->m != md->n) return NLH_INVALID_INPUT_ERROR;         // src/nonlin_solve.f90:241
    if (md->ufcn)
        return nlh_quasi_newton_solve_batch_device_h(h, o, jdelta, md->nprob, md->n, md->ufcn, analytic ? md->ujac : nullptr, md->uctx, x, fvec,
                                                     ib, status);
    return model_run(h, md, x, true, fvec, ib, status,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *pib, int32_t *pst) -> int {
                         return nlh_dq_quasi_newton_solve_batch(ph, o, jdelta, pt.cnt, md->n, pt.dA, pt.db, md->gamma, analytic, pt.dx, pt.df, pib, pst);
                     });
}

// constrained_least_squares_solver%solve on every problem of the model; xl / xu: n entries each (or NULL), the same box
// for every problem.
int nlh_dq_model_cls_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, double delta0, double stepscale0,
                           const double *xl, const double *xu, double *x, double *fvec, nlh_iteration_behavior *ib,
                           int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    const nlh_options oq = silent_in_batch(*o, md->nprob);
    o = &oq;
    if (md->ufcn) return nlh_cls_solve_batch_device_h(h, o, delta0, stepscale0, xl, xu, md->nprob, md->m, md->n, md->ufcn, md->ujac, md->uctx, x,
                                                      fvec, ib, status);
    return model_run(h, md, x, true, fvec, ib, status,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *pib, int32_t *pst) -> int {
                         return nlh_dq_cls_solve_batch(ph, o, delta0, stepscale0, xl, xu, pt.cnt, md->m, md->n, pt.dA, pt.db, md->gamma,
                                                       pt.dx, pt.df, pib, pst);
                     });
}

// nelder_mead%solve on every problem of a user's model of ONE function (the launcher is the fcnnvar, called with m = 1).
// The dense-quadratic family has no Nelder-Mead form, and a vector launcher is not nelder_mead's plugin.
int nlh_dq_model_nelder_mead_solve(nlh_handle *h, const nlh_options *o, double init_size, const nlh_dq_model *md, double *x,
                                   double *fout, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    if (!md->ufcn || md->m != 1) return NLH_INVALID_OPERATION_ERROR;
    return nlh_nm_solve_batch_device_h(h, o, init_size, md->nprob, md->n, md->ufcn, md->uctx, x, fout, ib, status);
}

// brent_solver%solve / newton_1var_solver%solve on every problem of a user's model of one equation in one unknown (the
// launcher is the fcn1var, called with n = m = 1; newton's derivative is the model's jacfcn launcher, or forward
// differences without one).  The dense-quadratic family has no such form.
int nlh_dq_model_brent_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, const double *lim, double *x,
                             double *fout, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    if (!md->ufcn || md->m != 1 || md->n != 1) return NLH_INVALID_OPERATION_ERROR;
    return nlh_root1v_solve_batch_device_h(h, o, 0, md->nprob, md->ufcn, nullptr, md->uctx, lim, x, fout, ib, status);
}

int nlh_dq_model_newton_1var_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, const double *lim, double *x,
                                   double *fout, nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    if (!md->ufcn || md->m != 1 || md->n != 1) return NLH_INVALID_OPERATION_ERROR;
    return nlh_root1v_solve_batch_device_h(h, o, 1, md->nprob, md->ufcn, md->ujac, md->uctx, lim, x, fout, ib, status);
}

// bfgs%solve on 0.5 ||F(x)||^2 of every problem of the model (forward-difference gradient); fout [nprob]: the objective
// at the solution, fvec [nprob][m]: F there.
int nlh_dq_model_bfgs_solve(nlh_handle *h, const nlh_options *o, const nlh_dq_model *md, double *x, double *fvec, double *fout,
                            nlh_iteration_behavior *ib, int32_t *status)
{
    if (!md || !o) return NLH_INVALID_INPUT_ERROR;
    const nlh_options oq = silent_in_batch(*o, md->nprob);
    o = &oq;
    if (md->ufcn) {
        // bfgs minimises a scalar fcnnvar: a user's model with ONE function is exactly that (its launcher is called with
        // m = 1, its jacobianfcn launcher is the gradient); a vector launcher is not bfgs's plugin
        if (md->m != 1) return NLH_INVALID_OPERATION_ERROR;
        const int rc = nlh_bfgs_solve_batch_device_h(h, o, md->nprob, md->n, md->ufcn, md->ujac, md->uctx, x, fout, ib, status);
        if (rc) return rc;
        if (fvec && fout)                                     // (the model's one "equation": f at the solution)
            for (int32_t p = 0; p < md->nprob; ++p) fvec[p] = fout[p];
        return 0;
    }
    return model_run(h, md, x, true, fvec, ib, status,
                     [&](nlh_handle *ph, const DqPart &pt, nlh_iteration_behavior *pib, int32_t *pst) -> int {
                         std::vector<double> fo(pt.cnt, 0.0);
                         const int rc = nlh_dq_bfgs_solve_batch(ph, o, pt.cnt, md->m, md->n, pt.dA, pt.db, md->gamma, pt.dx, fo.data(), pib, pst);
                         if (rc) return rc;
                         if (fout)
                             for (int i = 0; i < pt.cnt; ++i) fout[(size_t)pt.first + (size_t)i * pt.stride] = fo[i];
                         launch_dq_residual(ph, pt.cnt, md->m, md->n, pt.dA, pt.db, md->gamma, pt.dx, pt.df, nullptr, nullptr, -1);
                         HIPCHK(ph, hipGetLastError());
                         return 0;
                     });
}
