// A user's device fcn1var family, as a user of nlh_brent_solve_batch_device / nlh_newton_1var_solve_batch_device would
// write it: a per-problem cubic f(x) = c0 + x (c1 + x (c2 + x c3)) and its derivative c1 + x (2 c2 + x (3 c3)), as
// launchers (include/nonlin_hip.h: nlh_device_vecfcn / nlh_device_jacfcn, called with n = m = 1), with host twins of the
// same arithmetic, and a counting wrapper that records every point list it is handed.  Test / bench infrastructure.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

struct CubicCtx {
    int32_t nprob;
    double *dc;                         // [nprob][4], device
};

static __host__ __device__ inline double cubic_f(const double *c, double x) { return c[0] + x * (c[1] + x * (c[2] + x * c[3])); }
static __host__ __device__ inline double cubic_df(const double *c, double x) { return c[1] + x * (2.0 * c[2] + x * (3.0 * c[3])); }

static __global__ void k_cubic(int npoints, const int32_t *__restrict__ dprob, const double *__restrict__ c,
                               const double *__restrict__ x, double *__restrict__ f, int deriv)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= npoints) return;
    const double *cp = c + 4 * (size_t)dprob[q];
    f[q] = deriv ? cubic_df(cp, x[q]) : cubic_f(cp, x[q]);
}

static int cubic_run(void *ctx, void *stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *dF, int deriv)
{
    CubicCtx *c = (CubicCtx *)ctx;
    if (!c || n != 1 || m != 1) return 1;
    if (npoints <= 0) return 0;
    hipLaunchKernelGGL(k_cubic, dim3((unsigned)((npoints + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)npoints, dprob,
                       (const double *)c->dc, dX, dF, deriv);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

struct CountCtx {
    void *inner;
    std::vector<double> xs;             // every point of every fcn call, in call order
    std::vector<int32_t> probs;         // their problem indices
    std::vector<int64_t> sizes;         // the length of each call's list
    int64_t calls = 0, dcalls = 0;
};

extern "C" {

void *cubic_create(int32_t nprob, const double *c)
{
    CubicCtx *ctx = new CubicCtx();
    ctx->nprob = nprob;
    if (hipMalloc(&ctx->dc, sizeof(double) * 4 * (size_t)nprob) != hipSuccess) { delete ctx; return nullptr; }
    if (hipMemcpy(ctx->dc, c, sizeof(double) * 4 * (size_t)nprob, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(ctx->dc); delete ctx; return nullptr;
    }
    return ctx;
}

void cubic_destroy(void *ctx)
{
    CubicCtx *c = (CubicCtx *)ctx;
    if (!c) return;
    (void)hipFree(c->dc);
    delete c;
}

int cubic_launch(void *ctx, void *stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return cubic_run(ctx, stream, npoints, dprob, n, dX, m, dF, 0);
}

int cubic_launch_diff(void *ctx, void *stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                      double *dJ)
{
    return cubic_run(ctx, stream, npoints, dprob, n, dX, m, dJ, 1);
}

// host twins: the same arithmetic, the same bits
double cubic_host_f(const double *c, double x) { return cubic_f(c, x); }
double cubic_host_df(const double *c, double x) { return cubic_df(c, x); }

// the counting wrapper around a cubic context: records the points (synchronously: test use only), then evaluates
void *counting_create(void *inner)
{
    CountCtx *c = new CountCtx();
    c->inner = inner;
    return c;
}

void counting_destroy(void *ctx) { delete (CountCtx *)ctx; }

int counting_launch(void *ctx, void *stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                    double *dF)
{
    CountCtx *c = (CountCtx *)ctx;
    const size_t at = c->xs.size();
    c->xs.resize(at + (size_t)npoints);
    c->probs.resize(at + (size_t)npoints);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(c->xs.data() + at, dX, sizeof(double) * npoints, hipMemcpyDeviceToHost, s) != hipSuccess) return 3;
    if (hipMemcpyAsync(c->probs.data() + at, dprob, sizeof(int32_t) * npoints, hipMemcpyDeviceToHost, s) != hipSuccess) return 3;
    if (hipStreamSynchronize(s) != hipSuccess) return 3;
    c->calls++;
    c->sizes.push_back(npoints);
    return cubic_launch(c->inner, stream, npoints, dprob, n, dX, m, dF);
}

int counting_launch_diff(void *ctx, void *stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                         double *dJ)
{
    CountCtx *c = (CountCtx *)ctx;
    c->dcalls++;
    return cubic_launch_diff(c->inner, stream, npoints, dprob, n, dX, m, dJ);
}

int64_t counting_size(void *ctx) { return (int64_t)((CountCtx *)ctx)->xs.size(); }
int64_t counting_calls(void *ctx, int32_t deriv) { return deriv ? ((CountCtx *)ctx)->dcalls : ((CountCtx *)ctx)->calls; }

void counting_call_sizes(void *ctx, int64_t *sizes)
{
    CountCtx *c = (CountCtx *)ctx;
    for (size_t k = 0; k < c->sizes.size(); ++k) sizes[k] = c->sizes[k];
}

void counting_get(void *ctx, double *xs, int32_t *probs)
{
    CountCtx *c = (CountCtx *)ctx;
    for (size_t k = 0; k < c->xs.size(); ++k) { xs[k] = c->xs[k]; probs[k] = c->probs[k]; }
}

}  // extern "C"
