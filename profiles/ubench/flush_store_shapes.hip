// flush_store_shapes.hip -- which shape should the stores of the exact pass's flush have, and does writing to a second
// matrix pay, AT THE HEADLINE'S OCCUPANCY?  (rw_stream.hip asked the same at 1024 problems with one wave per workgroup
// and as many waves per SIMD as fit.)  Here: 2048 problems of 4096 x 256 (ld 320), the read pattern of
// k_qrx_pass<9,true,true> -- row-blocked matrix, a lane per column, four 16-byte loads per lane and 8-row block, 16 rows
// per load group, two groups in flight, the four windows of a problem as the waves of one workgroup with an LDS-only
// barrier per 64-row tile -- and two workgroups per CU (two waves per SIMD; LDS padding enforces it).
// Store shapes, each in place and out of place (read A, write B):
//   (a) four 16-byte stores per lane at a 64-byte lane stride: a lane writes its own sector in four instructions;
//   (b) whole sectors per lane quad: a 4 x 4 exchange of 16-byte pieces inside each quad (DPP, no LDS), after which every
//       store instruction writes 16 complete 64-byte sectors;
//   (c) 1 KB contiguous per store instruction: the 8-row x 64-column block turned through LDS (4 KB per wave, swizzled).
// Every out-of-place variant is checked against the values (a) writes.
// hipcc --offload-arch=gfx950 -O3 -o flush_store_shapes flush_store_shapes.hip ; ./flush_store_shapes [nprob] [LDS pad KB]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define NWIN 4
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <int CTRL> __device__ __forceinline__ unsigned dpp(unsigned x)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
// 4 x 4 transpose of 16-byte pieces inside each lane quad: on return r[q] of lane l holds what r[l & 3] of lane
// (l & ~3) + q held.  Two butterfly stages (partner lane ^ 2, then ^ 1), eight DPP moves each.
__device__ __forceinline__ void quad_transpose(u32x4 (&v)[4], int lane)
{
    const bool h2 = lane & 2, h1 = lane & 1;
    unsigned r[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { r[i][0] = v[i].x; r[i][1] = v[i].y; r[i][2] = v[i].z; r[i][3] = v[i].w; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned y = dpp<0x4E>(h2 ? r[i][c] : r[i + 2][c]);      // quad_perm [2,3,0,1]
            r[i][c] = h2 ? y : r[i][c];
            r[i + 2][c] = h2 ? r[i + 2][c] : y;
        }
#pragma unroll
    for (int i = 0; i < 4; i += 2)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned y = dpp<0xB1>(h1 ? r[i][c] : r[i + 1][c]);      // quad_perm [1,0,3,2]
            r[i][c] = h1 ? y : r[i][c];
            r[i + 1][c] = h1 ? r[i + 1][c] : y;
        }
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i].x = r[i][0]; v[i].y = r[i][1]; v[i].z = r[i][2]; v[i].w = r[i][3]; }
}

// SHAPE: -1 = read only, 0 = (a), 1 = (b), 2 = (c).  OOP: stores go to B.
template <int SHAPE, bool OOP>
__global__ void __launch_bounds__(64 * NWIN) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_flush(double *__restrict__ A, double *__restrict__ B, int m, int ld, size_t tst, double *__restrict__ out, int ldspad)
{
    constexpr int G = 2;                                            // 8-row blocks per load group (16 rows, as the flush)
    extern __shared__ double pad[];
    __shared__ __attribute__((aligned(16))) u32x4 xst[NWIN][256];
    const int p = blockIdx.x, lane = threadIdx.x & 63;
    const int win = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double *Ap = A + (size_t)p * tst, *Bp = (OOP ? B : A) + (size_t)p * tst;
    const int nblk = m / 8;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(Ap, 0, (int)((size_t)nblk * ld * 64), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(Bp, 0, (int)((size_t)nblk * ld * 64), 0x00020000);
    const unsigned wo = (unsigned)(ld - 64 * (win + 1)) * 64u;     // the window's first column, bytes inside a row block
    const unsigned so = wo + (unsigned)lane * 64u, ldb = (unsigned)ld * 64u;
    const unsigned qo = wo + (unsigned)(lane & ~3) * 64u + (unsigned)(lane & 3) * 16u;   // (b): + 64 q
    const unsigned co = wo + (unsigned)lane * 16u;                                        // (c): + 1024 q
    u32x4 *xs = xst[win];
    double acc = 0.0;
    u32x4 v0[4 * G], v1[4 * G];
    auto load = [&](u32x4 (&v)[4 * G], int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[g * 4 + q] = __builtin_amdgcn_raw_buffer_load_b128(ra, so + 16u * q, (unsigned)(blk + g) * ldb, 0);
    };
    auto work = [&](u32x4 (&v)[4 * G], int blk) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4 * G; ++i) {
            double x = __hiloint2double((int)v[i].y, (int)v[i].x), y = __hiloint2double((int)v[i].w, (int)v[i].z);
            acc = acc + x; acc = acc + y;
            x = x * 1.0000001; y = y * 0.9999999;
            v[i].x = (unsigned)__double2loint(x); v[i].y = (unsigned)__double2hiint(x);
            v[i].z = (unsigned)__double2loint(y); v[i].w = (unsigned)__double2hiint(y);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const unsigned boff = (unsigned)(blk + g) * ldb;
            if (SHAPE == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) __builtin_amdgcn_raw_buffer_store_b128(v[g * 4 + q], rb, so + 16u * q, boff, 1);
            } else if (SHAPE == 1) {
                u32x4 r[4] = {v[g * 4], v[g * 4 + 1], v[g * 4 + 2], v[g * 4 + 3]};
                quad_transpose(r, lane);
#pragma unroll
                for (int q = 0; q < 4; ++q) __builtin_amdgcn_raw_buffer_store_b128(r[q], rb, qo + 64u * q, boff, 1);
            } else if (SHAPE == 2) {
                // piece q of column c sits at xs[c * 4 + (q ^ ((c >> 2) & 3))]: both sides free of bank conflicts
#pragma unroll
                for (int q = 0; q < 4; ++q) xs[lane * 4 + (q ^ ((lane >> 2) & 3))] = v[g * 4 + q];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = q * 16 + (lane >> 2);
                    const u32x4 w = xs[c * 4 + ((lane & 3) ^ ((c >> 2) & 3))];
                    __builtin_amdgcn_raw_buffer_store_b128(w, rb, co + 1024u * q, boff, 1);
                }
            }
        }
    };
    load(v0, 0);
    for (int blk = 0; blk < nblk; blk += 2 * G) {
        load(v1, blk + G);
        work(v0, blk);
        load(v0, blk + 2 * G);                                     // past the end: out of range, returns zero
        work(v1, blk + G);
        if (((blk + 2 * G) & 7) == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the pass's tile barrier
    }
    if (acc == 123.456) out[p] = acc + pad[ldspad ? 1 : 0];
}

__global__ void k_fill(double *A, size_t nd)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += (size_t)gridDim.x * blockDim.x)
        A[i] = 1.0 + (double)(i % 1000003) * 1e-7;
}
// B against what shape (a) writes from A, live columns only (the last 64 NWIN of a row block)
__global__ void k_check(const double *A, const double *B, int m, int ld, size_t tst, int nprob, unsigned long long *bad)
{
    const size_t per = (size_t)(m / 8) * 64 * NWIN * 8, total = per * nprob;
    unsigned long long nb = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t p = i / per, r = i % per, blk = r / (64 * NWIN * 8), e = r % (64 * NWIN * 8);
        const size_t at = p * tst + (blk * ld + (ld - 64 * NWIN)) * 8 + e;
        const double want = A[at] * ((e & 1) ? 0.9999999 : 1.0000001);
        if (B[at] != want) ++nb;
    }
    if (nb) atomicAdd(bad, nb);
}

int main(int argc, char **argv)
{
    const int nprob = argc > 1 ? atoi(argv[1]) : 2048, m = 4096, ld = 320;
    const int ldskb = argc > 2 ? atoi(argv[2]) : 48;              // + 16 KB static: two workgroups per CU
    const size_t tst = (size_t)m * ld, nd = tst * nprob;
    double *A, *B, *out;
    unsigned long long *bad, hbad = 0;
    CK(hipMalloc(&A, sizeof(double) * nd + (1 << 20)));
    CK(hipMalloc(&B, sizeof(double) * nd + (1 << 20)));
    CK(hipMalloc(&out, sizeof(double) * nprob));
    CK(hipMalloc(&bad, sizeof(*bad)));
    hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double gb = 8.0 * m * 64.0 * NWIN * nprob / 1e9;        // bytes one direction
    printf("%s, nprob %d of %d x %d (ld %d), %d windows per workgroup, %d KB LDS pad per workgroup\n", prop.name, nprob, m,
           64 * NWIN, ld, NWIN, ldskb);
    double base = 0.0;
    auto run = [&](const char *name, auto kern, double dirs, bool check, bool is_base) -> int {
        const int NREP = 7;
        std::vector<float> ms(NREP);
        hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, A, nd);
        if (check) CK(hipMemsetAsync(B, 0, sizeof(double) * nd));
        for (int rep = 0; rep < NREP; ++rep) {
            if (rep == 1 && check) {                               // rep 0 wrote B from the freshly filled A
                CK(hipMemset(bad, 0, sizeof(*bad)));
                hipLaunchKernelGGL(k_check, dim3(4096), dim3(256), 0, 0, A, B, m, ld, tst, nprob, bad);
                CK(hipMemcpy(&hbad, bad, sizeof(hbad), hipMemcpyDeviceToHost));
            }
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(kern, dim3(nprob), dim3(64 * NWIN), ldskb * 1024, 0, A, B, m, ld, tst, out, ldskb);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            CK(hipEventElapsedTime(&ms[rep], e0, e1));
        }
        CK(hipGetLastError());
        std::sort(ms.begin() + 1, ms.end());                       // rep 0 is the warm-up
        const double med = ms[1 + (NREP - 1) / 2], best = ms[1], gbs = dirs * gb / (med * 1e-3);
        if (is_base) base = gbs;
        printf("%-44s median %7.3f ms  best %7.3f ms  %7.1f GB/s", name, med, best, gbs);
        if (dirs > 1.0 && base > 0.0) printf("  %+5.1f %% vs (a) in place", 100.0 * (gbs / base - 1.0));
        if (check) printf("  %s", hbad ? "WRONG VALUES" : "values ok");
        printf("\n");
        return hbad ? 3 : 0;
    };
    int rc = 0;
    rc |= run("read only", (k_flush<-1, false>), 1.0, false, false);
    rc |= run("(a) 4 x 16 B per lane, in place", (k_flush<0, false>), 2.0, false, true);
    rc |= run("(a) 4 x 16 B per lane, A -> B", (k_flush<0, true>), 2.0, true, false);
    rc |= run("(b) whole sectors per quad (DPP), in place", (k_flush<1, false>), 2.0, false, false);
    rc |= run("(b) whole sectors per quad (DPP), A -> B", (k_flush<1, true>), 2.0, true, false);
    rc |= run("(c) 1 KB contiguous (LDS), in place", (k_flush<2, false>), 2.0, false, false);
    rc |= run("(c) 1 KB contiguous (LDS), A -> B", (k_flush<2, true>), 2.0, true, false);
    return rc;
}
