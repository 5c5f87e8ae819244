// The device library's log on an array, for tests/test_gpu_pois.py::test_log_accuracy: the library function the Poisson
// kernels carry besides log1p (nonlin_amd/csrc/nlh_kernels_pois.h: the e < -0.5 path), measured against numpy.longdouble.
// Its own shared object, nothing of libnonlin_hip.so linked in.
#include <hip/hip_runtime.h>

static __global__ void __launch_bounds__(256) k_log(int n, const double *__restrict__ u, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log(u[i]);
}

extern "C" int probe_log(void *hip_stream, int n, const double *du, double *dout)
{
    if (n <= 0 || !du || !dout) return 1;
    hipLaunchKernelGGL(k_log, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, n, du, dout);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
