// nlh_pin.hip -- the pin pair (include/nonlin_hip_profile.h: nlh_pin_*): one parameter per wrapped problem held at its own value,
// the data shared, as a pair of wrapping launchers around any inner launcher pair (kernels: nlh_kernels_pin.h; scratch, grid and
// slice loop: nlh_launch.h).  The three tables are the caller's device arrays; the context holds their addresses only, so
// nlh_pin_set swaps them between solves without touching the scratch.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_pin.h"

static const uint32_t PIN_MAGIC = 0x6e695070u;

struct nlh_pin_ctx : WrapCtx {
    PinTables T;
};

static bool pin_tables_ok(int32_t nend, const int32_t *dsrc, const int32_t *dpos, const double *dtheta)
{
    return nend >= 0 && dsrc && dpos && dtheta;
}

int nlh_pin_wrap(nlh_handle *h, int32_t N, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, int32_t nend,
                 const int32_t *dsrc, const int32_t *dpos, const double *dtheta, nlh_pin_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || N < 2 || !pin_tables_ok(nend, dsrc, dpos, dtheta)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_pin_ctx *c = nullptr;
    const int rc = wrap_new(h, PIN_MAGIC, fcn, jac, inner_ctx, &c);
    if (rc) return rc;
    c->T = {N, nend, dsrc, dpos, dtheta};
    *out = c;
    return 0;
}

int nlh_pin_set(nlh_pin_ctx *c, int32_t nend, const int32_t *dsrc, const int32_t *dpos, const double *dtheta)
{
    if (!c || c->magic != PIN_MAGIC || !pin_tables_ok(nend, dsrc, dpos, dtheta)) return NLH_INVALID_INPUT_ERROR;
    c->T.nend = nend; c->T.src = dsrc; c->T.pos = dpos; c->T.theta = dtheta;
    return 0;
}

void nlh_pin_unwrap(nlh_pin_ctx *c)
{
    if (c && c->magic == PIN_MAGIC) wrap_release(c);
}

static void pin_launch_jac(const nlh_pin_ctx *c, int N, const int32_t *pp, int m, int npoints, const double *Jf, double *J, hipStream_t s)
{
    const JacGrid g = jac_grid("NLH_PIN_FORM", "NLH_PIN_SPLIT", c->cus, m, N - 1, npoints);
    if (g.flat) hipLaunchKernelGGL(k_pin_jac<true>, g.grid, dim3(256), 0, s, N, pp, m, g.nblk, g.ppw, g.cpg, npoints, Jf, J);
    else hipLaunchKernelGGL(k_pin_jac<false>, g.grid, dim3(256), 0, s, N, pp, m, g.nblk, g.ppw, g.cpg, npoints, Jf, J);
}

// Both launchers.  What they check themselves is refused before any launch; the inner launcher can refuse only once it is
// called, after the expansion of its slice has been enqueued: then only the context's scratch has been written.
static int pin_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                    double *out)
{
    nlh_pin_ctx *c = wrap_ctx<nlh_pin_ctx>(ctx, PIN_MAGIC);
    int end;
    if (wrap_refused(c, c && n == c->T.N - 1 && m >= 1 && dX && out, jac, npoints, &end)) return end;
    const PinTables T = c->T;          // (one reading of the tables per call)
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t N = (size_t)T.N;
    // scratch per point: the inner parameters P, for a Jacobian call the inner Jacobian Jf over them, and -- in the two halves
    // of the last double -- the point's entry of the inner problem list and its pos
    const size_t pj = N * (jac ? (size_t)m + 1 : 1);
    return wrap_slices(c->scratch, "NLH_PIN_SCRATCH", c->device, s, pj + 1, npoints, m, dprob,
                       [&](double *P, int slice, int q0, int cnt, const int32_t *lp) {
        double *Jf = P + (size_t)slice * N;
        int32_t *sp = (int32_t *)(P + (size_t)slice * pj), *pp = sp + slice;
        hipLaunchKernelGGL(k_pin_expand, dim3((unsigned)(((size_t)cnt * N + 255) / 256)), dim3(256), 0, s, T, cnt, lp, dX + (size_t)q0 * n, P, sp,
                           pp);
        if (!jac) return c->fcn(c->inner, hip_stream, cnt, sp, T.N, P, m, out + (size_t)q0 * m);
        if (const int rc = c->jac(c->inner, hip_stream, cnt, sp, T.N, P, m, Jf)) return rc;
        pin_launch_jac(c, T.N, pp, m, cnt, Jf, out + (size_t)q0 * m * n, s);
        return 0;
    });
}

int nlh_pin_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return pin_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_pin_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return pin_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}
