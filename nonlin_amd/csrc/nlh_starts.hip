// nlh_starts.hip -- starts: the batched box scan (include/nonlin_hip_starts.h: nlh_starts_*; kernels: nlh_kernels_starts.h).
// The candidates are made on the host and uploaded once; the scan then walks them in chunks, and the problems in slices, so
// that one launcher call's residuals stay inside STARTS_F_BYTES: points, the caller's launcher, costs, merge into the kept.
#include "nlh_internal.h"
#include "nlh_kernels_starts.h"

static const int STARTS_PRIMES[NLH_STARTS_MAX_N] = {2,  3,  5,  7,  11, 13, 17, 19, 23, 29, 31,  37,  41,  43,  47,  53,
                                                    59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131};

// What nlh_starts_candidates refuses; cand is looked at by the caller.
static bool starts_box_ok(int32_t n, int32_t first, int32_t count, const double *xl, const double *xu, const int32_t *logscale)
{
    if (n < 1 || n > NLH_STARTS_MAX_N || !xl || !xu || count < 0 || first < 0) return false;
    if ((int64_t)first + count > NLH_STARTS_MAX_CAND) return false;
    for (int d = 0; d < n; ++d) {
        if (!std::isfinite(xl[d]) || !std::isfinite(xu[d]) || xl[d] > xu[d]) return false;
        if (logscale && logscale[d] && !(xl[d] > 0.0)) return false;
    }
    return true;
}

static void starts_fill(int32_t n, int32_t first, int32_t count, const double *xl, const double *xu, const int32_t *logscale, double *cand)
{
    for (int d = 0; d < n; ++d) {
        const double lo = xl[d], hi = xu[d];
        const bool lg = logscale && logscale[d];
        const double span = lg ? log(hi / lo) : hi - lo;
        const int p = STARTS_PRIMES[d];
        for (int32_t c = 0; c < count; ++c) {
            int64_t i = (int64_t)first + c + 1;
            double f = 1.0 / p, r = 0.0;
            while (i > 0) {
                r = r + f * (double)(i % p);
                i = i / p;
                f = f / p;
            }
            double v = lg ? lo * exp(r * span) : lo + r * span;
            if (v < lo) v = lo;
            if (v > hi) v = hi;
            cand[(size_t)c * n + d] = v;
        }
    }
}

int nlh_starts_candidates(int32_t n, int32_t first, int32_t count, const double *xl, const double *xu, const int32_t *logscale,
                          double *cand)
{
    if (!starts_box_ok(n, first, count, xl, xu, logscale) || (count > 0 && !cand)) return NLH_INVALID_INPUT_ERROR;
    starts_fill(n, first, count, xl, xu, logscale, cand);
    return 0;
}

// The residuals F [points][m] of one launcher call stay inside this many bytes.
static const size_t STARTS_F_BYTES = (size_t)256 << 20;

// The most points of one launcher call: NLH_STARTS_POINTS (tests; read per call) or what STARTS_F_BYTES holds, and never more
// than a launcher's 31-bit point counts take (slice_points).
static int64_t starts_points(int32_t m, int32_t n)
{
    int64_t P = (int64_t)std::max<size_t>(1, STARTS_F_BYTES / (sizeof(double) * (size_t)m));
    if (const char *e = getenv("NLH_STARTS_POINTS")) {
        const long long v = atoll(e);
        if (v >= 1) P = v;
    }
    return std::min<int64_t>(P, ((int64_t)1 << 30) / n);
}

static int starts_refused(const nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, const double *xl,
                          const double *xu, const int32_t *logscale, int32_t ncand, int32_t keep, const double *x0, const double *cost,
                          const int32_t *index)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn || !x0 || !cost || !index || nprob < 0 || m < 1 || ncand < 1 || keep < 1 || keep > NLH_STARTS_MAX_KEEP || keep > ncand)
        return NLH_INVALID_INPUT_ERROR;
    if (!starts_box_ok(n, 0, ncand, xl, xu, logscale)) return NLH_INVALID_INPUT_ERROR;
    return 0;
}

static inline unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

int nlh_starts_search_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, void *ctx,
                                   const double *xl, const double *xu, const int32_t *logscale, int32_t ncand, int32_t keep,
                                   double *dx0, double *dcost, int32_t *dindex)
{
    int rc;
    if ((rc = starts_refused(h, nprob, m, n, fcn, xl, xu, logscale, ncand, keep, dx0, dcost, dindex))) return rc;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // the chunk rule: every candidate of as many problems as fit, or one problem and as many candidates as fit
    const int64_t P = starts_points(m, n);
    const int32_t C = (int32_t)std::min<int64_t>(ncand, P);
    const int32_t slice = P >= ncand ? (int32_t)std::min<int64_t>(nprob, P / ncand) : 1;
    const size_t pts = (size_t)slice * C;
    if ((rc = ensure(h, h->startsC, sizeof(double) * (size_t)ncand * n))) return rc;
    if ((rc = ensure(h, h->startsX, sizeof(double) * pts * n + sizeof(int32_t) * pts))) return rc;
    if ((rc = ensure(h, h->startsF, sizeof(double) * pts * m))) return rc;
    if ((rc = ensure(h, h->startsS, sizeof(double) * pts))) return rc;
    double *cand = (double *)h->startsC.p, *X = (double *)h->startsX.p, *F = (double *)h->startsF.p, *S = (double *)h->startsS.p;
    int32_t *prob = (int32_t *)(X + pts * n);
    {
        std::vector<double> table((size_t)ncand * n);
        starts_fill(n, 0, ncand, xl, xu, logscale, table.data());
        HIPCHK(h, hipMemcpyAsync(cand, table.data(), sizeof(double) * table.size(), hipMemcpyHostToDevice, s));
        HIPCHK(h, hipStreamSynchronize(s));                         // (the table goes with this block)
    }
    const size_t kept = (size_t)nprob * keep;
    hipLaunchKernelGGL(k_starts_clear, dim3(blocks256(kept)), dim3(256), 0, s, kept, dcost, dindex);
    for (int32_t p0 = 0; p0 < nprob; p0 += slice) {
        const int32_t cnt = std::min(slice, nprob - p0);
        for (int32_t c0 = 0; c0 < ncand; c0 += C) {
            const int32_t Cc = std::min(C, ncand - c0);
            const int32_t np = cnt * Cc;                            // (<= pts <= 2^30 / n)
            hipLaunchKernelGGL(k_starts_points, dim3(blocks256((size_t)np * n)), dim3(256), 0, s, n, p0, cnt, c0, Cc, cand, X, prob);
            if (const int e = fcn(ctx, s, np, prob, n, X, m, F)) {
                h->err = "starts: the user's launcher returned " + std::to_string(e);
                return e;
            }
            hipLaunchKernelGGL(k_starts_cost, dim3((np + 3) / 4), dim3(256), 0, s, np, m, F, S);
            hipLaunchKernelGGL(k_starts_merge, dim3((cnt + 3) / 4), dim3(256), 0, s, cnt, p0, Cc, c0, keep, S, dcost, dindex);
        }
    }
    hipLaunchKernelGGL(k_starts_finish, dim3(blocks256(kept * n)), dim3(256), 0, s, kept * n, n, cand, dindex, dx0);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_starts_search_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, void *ctx,
                                     const double *xl, const double *xu, const int32_t *logscale, int32_t ncand, int32_t keep,
                                     double *x0, double *cost, int32_t *index)
{
    int rc;
    if ((rc = starts_refused(h, nprob, m, n, fcn, xl, xu, logscale, ncand, keep, x0, cost, index))) return rc;
    if (nprob == 0) return 0;
    const size_t kept = (size_t)nprob * keep, xb = sizeof(double) * kept * n, cb = sizeof(double) * kept, ib = sizeof(int32_t) * kept;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->startsH, xb + cb + ib))) return rc;
    char *base = (char *)h->startsH.p;
    double *dx0 = (double *)base, *dcost = (double *)(base + xb);
    int32_t *dindex = (int32_t *)(base + xb + cb);
    if ((rc = nlh_starts_search_batch_device(h, nprob, m, n, fcn, ctx, xl, xu, logscale, ncand, keep, dx0, dcost, dindex))) return rc;
    HIPCHK(h, hipMemcpyAsync(x0, dx0, xb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cost, dcost, cb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(index, dindex, ib, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int nlh_starts_cost_batch(nlh_handle *h, int32_t npoints, int32_t m, const double *dF, double *dcost)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (npoints < 0 || m < 1 || !dF || !dcost) return NLH_INVALID_INPUT_ERROR;
    if (npoints == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_starts_cost, dim3(((unsigned)npoints + 3) / 4), dim3(256), 0, h->stream, npoints, m, dF, dcost);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_starts_pick_batch(nlh_handle *h, int32_t nprob, int32_t keep, const double *dcost, int32_t *dwhich)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || keep < 1 || keep > NLH_STARTS_MAX_KEEP || !dcost || !dwhich) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_starts_pick, dim3(blocks256((size_t)nprob)), dim3(256), 0, h->stream, nprob, keep, dcost, dwhich);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_starts_take_batch(nlh_handle *h, int32_t nprob, int32_t keep, int32_t width, const double *dsrc, const int32_t *dwhich,
                          double *ddst)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || keep < 1 || keep > NLH_STARTS_MAX_KEEP || width < 1 || !dsrc || !dwhich || !ddst) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    const size_t total = (size_t)nprob * width;
    if ((total + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_starts_take, dim3(blocks256(total)), dim3(256), 0, h->stream, total, nprob, keep, width, dsrc, dwhich, ddst);
    HIPCHK(h, hipGetLastError());
    return 0;
}
