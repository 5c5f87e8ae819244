// nlh_pois.hip -- Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*): counting data for any device model, as a pair of
// wrapping launchers around any UNWEIGHTED inner launcher pair (kernels and arithmetic: nlh_kernels_pois.h; scratch, grid and
// slice loop: nlh_launch.h).  Here: the wrapping context, the launchers, nlh_pois_apply_batch, and the check of host counts
// and masks.  The one-call Poisson fits are the pipeline of nlh_fit.hip; the model object is nlh_pois_model_create
// (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_pois.h"

static const uint32_t POIS_MAGIC = 0x73696f70u;

struct nlh_pois_ctx : WrapCtx {
    const double *dy = nullptr, *dw = nullptr;
    double mu_floor = 0.0;
};

void pois_ctx_rebind(nlh_pois_ctx *c, const double *dy, const double *dw) { c->dy = dy; c->dw = dw; }

bool nlh_pois_floor_ok(double mu_floor) { return mu_floor > 0.0 && std::isfinite(mu_floor); }

// host counts and mask: w (when given) 0 or 1, every one; y finite and not negative on every row the mask keeps (a masked
// row may hold anything, as on device arrays)
bool nlh_pois_data_ok(const double *y, const double *w, size_t cnt)
{
    for (size_t i = 0; i < cnt; ++i) {
        if (w && w[i] != 0.0 && w[i] != 1.0) return false;
        if (w && w[i] == 0.0) continue;
        if (!(y[i] >= 0.0) || !std::isfinite(y[i])) return false;
    }
    return true;
}

int nlh_pois_wrap(nlh_handle *h, const double *dy, const double *dw, double mu_floor, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                  void *inner_ctx, nlh_pois_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !dy) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_pois_ctx *c = nullptr;
    if (const int rc = wrap_new(h, POIS_MAGIC, fcn, jac, inner_ctx, &c)) return rc;
    c->dy = dy; c->dw = dw; c->mu_floor = mu_floor;
    *out = c;
    return 0;
}

void nlh_pois_unwrap(nlh_pois_ctx *c)
{
    if (c && c->magic == POIS_MAGIC) wrap_release(c);
}

static void pois_launch_jac(const nlh_pois_ctx *c, const PoisArgs &A, int m, int n, int npoints, const double *R, double *J, hipStream_t s)
{
    const JacGrid g = jac_grid("NLH_POIS_FORM", "NLH_POIS_SPLIT", c->cus, m, n, npoints);
    if (g.flat) hipLaunchKernelGGL(k_pois_jac<true>, g.grid, dim3(256), 0, s, A, m, n, g.nblk, g.ppw, g.cpg, npoints, R, J);
    else hipLaunchKernelGGL(k_pois_jac<false>, g.grid, dim3(256), 0, s, A, m, n, g.nblk, g.ppw, g.cpg, npoints, R, J);
}

// Both launchers.  What they check themselves is refused before any launch; an inner error comes back as it is, with no
// further launch.  Scratch: the inner residual R of a Jacobian call, and a problem list -- for the inner launcher and for the
// rows of y and w -- when the caller passed none.
static int pois_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_pois_ctx *c = wrap_ctx<nlh_pois_ctx>(ctx, POIS_MAGIC);
    int end;
    if (wrap_refused(c, c && c->dy && n >= 1 && m >= 1 && dX && out, jac, npoints, &end)) return end;
    hipStream_t s = (hipStream_t)hip_stream;
    PoisArgs A;
    A.y = c->dy; A.w = c->dw; A.mu_floor = c->mu_floor;
    return wrap_slices(c->scratch, "NLH_POIS_SCRATCH", c->device, s, jac ? (size_t)m : 0, npoints, m, dprob,
                       [&](double *R, int, int q0, int cnt, const int32_t *lp) {
        A.dprob = lp;
        const double *Xs = dX + (size_t)q0 * n;
        int rc;
        if (!jac) {
            double *F = out + (size_t)q0 * m;
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, F))) return rc;
            hipLaunchKernelGGL(k_pois_fcn, dim3((unsigned)(((size_t)cnt * m + 255) / 256)), dim3(256), 0, s, A, m, cnt, F);
        } else {
            double *J = out + (size_t)q0 * m * n;
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, R))) return rc;
            if ((rc = c->jac(c->inner, hip_stream, cnt, lp, n, Xs, m, J))) return rc;
            pois_launch_jac(c, A, m, n, cnt, R, J, s);
        }
        return 0;
    });
}

int nlh_pois_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return pois_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_pois_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return pois_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

int nlh_pois_apply_batch(nlh_handle *h, int32_t nprob, int32_t m, const double *dy, const double *dw, double mu_floor, const double *dr,
                         double *dout, double *dg, double *ddev)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)nprob * m + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0 || (!dout && !dg && !ddev)) return 0;
    if (!dr || !dy) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    PoisArgs A;
    A.y = dy; A.w = dw; A.dprob = nullptr; A.mu_floor = mu_floor;
    hipLaunchKernelGGL(k_pois_apply, dim3((unsigned)(((size_t)nprob * m + 255) / 256)), dim3(256), 0, h->stream, A, m, nprob, dr, dout, dg, ddev);
    HIPCHK(h, hipGetLastError());
    return 0;
}
