// The device library's log1p on an array, for tests/test_gpu_loss.py::test_log1p_accuracy: the one library function the Cauchy
// loss carries (nonlin_amd/csrc/nlh_kernels_loss.h), measured against numpy.longdouble.  Its own shared object, nothing of
// libnonlin_hip.so linked in.
#include <hip/hip_runtime.h>

static __global__ void __launch_bounds__(256) k_log1p(int n, const double *__restrict__ z, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log1p(z[i]);
}

extern "C" int probe_log1p(void *hip_stream, int n, const double *dz, double *dout)
{
    if (n <= 0 || !dz || !dout) return 1;
    hipLaunchKernelGGL(k_log1p, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, n, dz, dout);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
