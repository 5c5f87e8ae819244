// nlh_bin.hip -- bin-integrated fits (include/nonlin_hip_bin.h: nlh_bin_*): any device model integrated or averaged over the
// bins of its data by a quadrature rule, as a pair of wrapping launchers around any inner launcher pair bound on the rule's
// nodes (kernel and arithmetic: nlh_kernels_bin.h; scratch, grid and slice loop: nlh_launch.h).  Here: the Gauss-Legendre
// rules, the check of a transform, the wrapping context, the launch, the launchers and nlh_bin_apply_batch.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_bin.h"

static const uint32_t BIN_MAGIC = 0x5f6e6962u;

struct nlh_bin_ctx : WrapCtx {
    nlh_bin bn{};
    const double *dy = nullptr, *dw = nullptr;
};

// Gauss-Legendre on [-1, 1], Q = 1 .. 8.  The nodes, ascending: each the double nearest the exact value.  The weights: the
// doubles numpy.polynomial.legendre.leggauss gives (numpy 2.2, x86-64), the reference the rule is held to within 2^-52; they
// are symmetric, sum to 2 within an ulp of 2, and lie within 1e-15 of the exact weights (up to 34 ulp of the smallest ones)
static const double BIN_XI[8][8] = {
    {0.0},
    {-0.5773502691896257, 0.5773502691896257},
    {-0.7745966692414834, 0.0, 0.7745966692414834},
    {-0.8611363115940526, -0.33998104358485626, 0.33998104358485626, 0.8611363115940526},
    {-0.906179845938664, -0.5384693101056831, 0.0, 0.5384693101056831, 0.906179845938664},
    {-0.932469514203152, -0.6612093864662645, -0.2386191860831969, 0.2386191860831969, 0.6612093864662645, 0.932469514203152},
    {-0.9491079123427585, -0.7415311855993945, -0.4058451513773972, 0.0, 0.4058451513773972, 0.7415311855993945, 0.9491079123427585},
    {-0.9602898564975363, -0.7966664774136267, -0.525532409916329, -0.1834346424956498, 0.1834346424956498, 0.525532409916329,
     0.7966664774136267, 0.9602898564975363}};
static const double BIN_C[8][8] = {
    {2.0},
    {1.0, 1.0},
    {0.5555555555555557, 0.8888888888888888, 0.5555555555555557},
    {0.3478548451374537, 0.6521451548625462, 0.6521451548625462, 0.3478548451374537},
    {0.23692688505618942, 0.4786286704993662, 0.568888888888889, 0.4786286704993662, 0.23692688505618942},
    {0.17132449237916975, 0.36076157304813894, 0.46791393457269137, 0.46791393457269137, 0.36076157304813894, 0.17132449237916975},
    {0.12948496616887065, 0.2797053914892766, 0.3818300505051183, 0.41795918367346896, 0.3818300505051183, 0.2797053914892766,
     0.12948496616887065},
    {0.10122853629037669, 0.22238103445337434, 0.31370664587788705, 0.36268378337836177, 0.36268378337836177, 0.31370664587788705,
     0.22238103445337434, 0.10122853629037669}};

int nlh_bin_rule(int32_t Q, double *xi, double *c)
{
    if (Q < 1 || Q > 8 || !xi || !c) return NLH_INVALID_INPUT_ERROR;
    for (int q = 0; q < Q; ++q) { xi[q] = BIN_XI[Q - 1][q]; c[q] = BIN_C[Q - 1][q]; }
    return 0;
}

static bool nlh_bin_ok(const nlh_bin *bn) { return bn && bn->Q >= 1 && bn->Q <= NLH_BIN_MAX_Q; }

int nlh_bin_wrap(nlh_handle *h, const nlh_bin *bn, const double *dy, const double *dw, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                 void *inner_ctx, nlh_bin_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !dy || !nlh_bin_ok(bn)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_bin_ctx *c = nullptr;
    if (const int rc = wrap_new(h, BIN_MAGIC, fcn, jac, inner_ctx, &c)) return rc;
    c->bn = *bn; c->dy = dy; c->dw = dw;
    *out = c;
    return 0;
}

void nlh_bin_unwrap(nlh_bin_ctx *c)
{
    if (c && c->magic == BIN_MAGIC) wrap_release(c);
}

static BinArgs bin_args(const nlh_bin &bn, const double *y, const double *w)
{
    BinArgs A;
    A.s = bn.s; A.y = y; A.w = w; A.dprob = nullptr; A.Q = bn.Q; A.shared_s = bn.shared_s != 0;
    for (int q = 0; q < NLH_BIN_MAX_Q; ++q) A.c[q] = q < bn.Q ? bn.c[q] : 0.0;
    return A;
}

// One launch: V [npoints][ncol][Q m] -> O [npoints][ncol][m], out of place, in the form and with the column split of jac_grid
// (gridDim.y holds 65535 groups at most: beyond that a group takes more columns, whatever the split asked for).
static int bin_launch(int cus, const BinArgs &A, int mode, int m, int ncol, int npoints, const double *V, double *O, hipStream_t s)
{
    const int nblk = (m + 255) / 256;
    if ((size_t)npoints * nblk > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    JacGrid g = jac_grid("NLH_BIN_FORM", "NLH_BIN_SPLIT", cus, m, ncol, npoints);
    if (g.grid.y > 65535u) {
        g.cpg = (ncol + 65534) / 65535;
        g.grid.y = (unsigned)((ncol + g.cpg - 1) / g.cpg);
    }
    if (g.flat) hipLaunchKernelGGL(k_bin<true>, g.grid, dim3(256), 0, s, A, mode, m, ncol, g.nblk, g.ppw, g.cpg, npoints, V, O);
    else hipLaunchKernelGGL(k_bin<false>, g.grid, dim3(256), 0, s, A, mode, m, ncol, g.nblk, g.ppw, g.cpg, npoints, V, O);
    return 0;
}

// Both launchers.  What they check themselves is refused before any launch; an inner error comes back as it is, with no
// further launch.  Scratch: the inner model values V [Q m] or the inner Jacobian Jf [n][Q m] of a point, and a problem list --
// for the inner launcher and for the rows of y, w and s -- when the caller passed none.
static int bin_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                    double *out)
{
    nlh_bin_ctx *c = wrap_ctx<nlh_bin_ctx>(ctx, BIN_MAGIC);
    int end;
    if (wrap_refused(c, c && c->dy && nlh_bin_ok(&c->bn) && n >= 1 && m >= 1 && dX && out, jac, npoints, &end)) return end;
    const int64_t rows = (int64_t)c->bn.Q * m;
    if (rows > 0x7fffffff) return NLH_ARRAY_SIZE_ERROR;
    const int qm = (int)rows;
    hipStream_t s = (hipStream_t)hip_stream;
    BinArgs A = bin_args(c->bn, jac ? nullptr : c->dy, c->dw);
    const size_t per = jac ? (size_t)qm * n : (size_t)qm;
    return wrap_slices(c->scratch, "NLH_BIN_SCRATCH", c->device, s, per, npoints, qm, dprob,
                       [&](double *S, int, int q0, int cnt, const int32_t *lp) {
        A.dprob = lp;
        const double *Xs = dX + (size_t)q0 * n;
        int rc;
        if (!jac) {
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, qm, S))) return rc;
            return bin_launch(c->cus, A, BIN_FCN, m, 1, cnt, S, out + (size_t)q0 * m, s);
        }
        if ((rc = c->jac(c->inner, hip_stream, cnt, lp, n, Xs, qm, S))) return rc;
        return bin_launch(c->cus, A, BIN_JAC, m, n, cnt, S, out + (size_t)q0 * m * n, s);
    });
}

int nlh_bin_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return bin_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_bin_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return bin_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

int nlh_bin_apply_batch(nlh_handle *h, const nlh_bin *bn, int32_t nprob, int32_t m, int32_t ncol, const double *dv, double *dout)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || m < 1 || ncol < 1 || !nlh_bin_ok(bn)) return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)bn->Q * m > 0x7fffffff || (size_t)nprob * ((size_t)(m + 255) / 256) > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    if (!dv || !dout || dv == dout) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    const BinArgs A = bin_args(*bn, nullptr, nullptr);
    if (const int rc = bin_launch(device_cus(h->device), A, BIN_JAC, m, ncol, nprob, dv, dout, h->stream)) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}
