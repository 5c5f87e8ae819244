// nlh_kernels_specfun2.h -- the second set of special functions of the formula models (include/nonlin_hip.h: the
// instructions J0 J1 I0E I1E LGAMMA EXPM1 LOG1P): the exponentially scaled modified Bessel functions i0e and i1e and the
// digamma function that is LGAMMA's tangent, written here; j0, j1, lgamma, expm1 and log1p are the device library's.
//
// THE ARITHMETIC IS PART OF THE INTERFACE; the table is in include/nonlin_hip.h and the functions below are it, line for
// line: one IEEE operation per step (-ffp-contract=off).  i0e and i1e use + - * / and sqrt only, so a formula whose only
// functions they are stays in the bit-exact class; digamma calls log and is in the library class, as lgamma is.
//
// i0e, i1e: Chebyshev series summed by Clenshaw's recurrence, |a| <= 8 in y = |a|/2 - 2 and |a| > 8 in y = 32/|a| - 2 over
// sqrt(|a|) (the arrangement of Cephes' i0e and i1e; the coefficients are derived again, at 40 digits, by
// tests/golden/make_specfun2_tables.py, which printed the literals below).  i1e departs from it below 8: Cephes' series of
// exp(-x) I1(x)/x on [0, 8] cancels to a thirtieth of its terms near 8 and the product with x is 10 ulp off there, so the
// quotient is kept to |a| <= 1, next to the zero, and 1 < |a| <= 8 has a series of exp(-x) I1(x) itself, which varies by 1.7.
// The kernels read a table with a uniform index, so the loads are scalar.
#pragma once
#include <math.h>

// exp(-x) I0(x) on 0 <= x <= 8, in T_k(y/2), y = x/2 - 2; highest degree first
static constexpr double NLH_SF2_I0E_A[30] = {
    -0x1.45cb72134d0efp-58, 0x1.33362977da589p-55, -0x1.184eb721ebbb4p-52, 0x1.ee6d893f65ebap-50,
    -0x1.a5022c297fbebp-47, 0x1.59b464b262627p-44, -0x1.1164c62ee1af0p-41, 0x1.9fe2fe19bd324p-39,
    -0x1.2fc957a946abcp-36, 0x1.a98becc743c10p-34, -0x1.1d4fe13ae9556p-31, 0x1.6d903a454cb34p-29,
    -0x1.beaf68c0b30abp-27, 0x1.03b769d4d6435p-24, -0x1.1ec638f227f8dp-22, 0x1.2bf24978cf4acp-20,
    -0x1.2866fcba56427p-18, 0x1.13f58be9a2859p-16, -0x1.e2b2659c41d5ap-15, 0x1.8b51b74107cabp-13,
    -0x1.2e2fd1f15eb52p-11, 0x1.adc758a12100ep-10, -0x1.1b65e201aa849p-8, 0x1.59961f3dde3ddp-7,
    -0x1.84e9ef121b6f0p-6, 0x1.93e8acea8a32dp-5, -0x1.84b70342d06eap-4, 0x1.5f7ac77ac88c0p-3,
    -0x1.37febc057cd8dp-2, 0x1.5a84e9035a22ap-1,
};
// sqrt(x) exp(-x) I0(x) on x >= 8, in T_k(y/2), y = 32/x - 2
static constexpr double NLH_SF2_I0E_B[25] = {
    -0x1.0adb754ca8b19p-57, -0x1.646da66119130p-58, 0x1.9be1812d98421p-55, 0x1.3f3dd076041cdp-55,
    -0x1.4600babd21fe4p-52, -0x1.8aee7d908de38p-52, 0x1.fee7da3eafb1fp-50, 0x1.12a919094e6d7p-48,
    -0x1.583fe7e65629ap-47, -0x1.75d99cf68bb32p-45, 0x1.156ff0d5fc545p-46, 0x1.b1c8c6b83c073p-42,
    0x1.94347fa268cecp-41, -0x1.f904303178d66p-40, -0x1.d0fd7357e7bf2p-37, -0x1.1511d08397425p-35,
    0x1.a24feabe8004fp-37, 0x1.0f9ccc0f46f75p-31, 0x1.d2c64a9225b87p-29, 0x1.8569280d6d56dp-26,
    0x1.b8007d9cd616ep-23, 0x1.8412bc101c586p-19, 0x1.20fa378999e52p-14, 0x1.b998ca2e59049p-9,
    0x1.9be62aca809cbp-1,
};
// exp(-x) I1(x)/x on 0 <= x <= 1, y = x*4 - 2
static constexpr double NLH_SF2_I1E_A[15] = {
    0x1.7cec2db187285p-57, -0x1.7237f96834e46p-52, 0x1.50bb830d17b75p-47, -0x1.1d48a49755aa2p-42,
    0x1.bfd46f9bed1cbp-38, -0x1.4396657ae9b3cp-33, 0x1.ab4d622e41c6cp-29, -0x1.ff01fcb434e5fp-25,
    0x1.11b468693d58cp-20, -0x1.030dc18649cd8p-16, 0x1.a999415d3048fp-13, -0x1.2822a9da1083dp-9,
    0x1.50c931cd756efp-6, -0x1.2670dd1fc00bfp-3, 0x1.553130fd36b0ap-1,
};
// exp(-x) I1(x) on 1 <= x <= 8, y = (x - 4.5)/1.75
static constexpr double NLH_SF2_I1E_M[28] = {
    0x1.341a9e4567edap-59, -0x1.34cf57a7ba1e6p-56, 0x1.2ab592d3ef91ap-53, -0x1.167fd6b18cb28p-50,
    0x1.f3e0cb302fefdp-48, -0x1.af342327635e9p-45, 0x1.64f94e52ff15ep-42, -0x1.1b23d2c6aaf22p-39,
    0x1.ad8f4c8a1c5d7p-37, -0x1.370675b689ab6p-34, 0x1.acff924c92859p-32, -0x1.19267d6a5c7e4p-29,
    0x1.5d4e0bf7c4eafp-27, -0x1.9a37889088869p-25, 0x1.c5f81ce8ff7f7p-23, -0x1.d7ca694355559p-21,
    0x1.caaab7dcaa367p-19, -0x1.9f46b100f0dc5p-17, 0x1.5c5441866551ap-15, -0x1.0cf0154c327d8p-13,
    0x1.7b020071a581ep-12, -0x1.e15a34ac81499p-11, 0x1.0d692b21c9c96p-9, -0x1.f97b8a302d41fp-9,
    0x1.4dbc7f3dfde8cp-8, 0x1.f998700f0c15ep-11, -0x1.6c0a234c41eb2p-5, 0x1.665b03d233307p-2,
};
// sqrt(x) exp(-x) I1(x) on x >= 8
static constexpr double NLH_SF2_I1E_B[25] = {
    0x1.1556db352e8e6p-57, 0x1.45b8aea87b950p-58, -0x1.acea3b2532277p-55, -0x1.2806c9c773320p-55,
    0x1.55915fceb588ap-52, 0x1.7d68e5f04a2d1p-52, -0x1.0efcd8bc4d22ap-49, -0x1.12db5138afbc7p-48,
    0x1.776e1762d31e8p-47, 0x1.80d3c26b3281ep-45, -0x1.7a9482e6d22a0p-46, -0x1.cbc458e73e255p-42,
    -0x1.953e1076ab493p-41, 0x1.1e7d3f6439fa3p-39, 0x1.f101f653c457bp-37, 0x1.1e1a1f1587865p-35,
    -0x1.4dcf9d4504c0cp-36, -0x1.334ca5423dd80p-31, -0x1.0790b9ad53528p-28, -0x1.c415394bb46c1p-26,
    -0x1.0dbfd2e9e5443p-22, -0x1.048df49ca0373p-18, -0x1.cfd7f804aa9a6p-14, -0x1.3fda053fcdb4cp-7,
    0x1.8ea18b55b1514p-1,
};
// B_2k/(2k), k = 1 .. 7: 1/12, -1/120, 1/252, -1/240, 1/132, -691/32760, 1/12
static constexpr double NLH_SF2_DIGAMMA_B[7] = {
    0x1.5555555555555p-4, -0x1.1111111111111p-7, 0x1.0410410410410p-8, -0x1.1111111111111p-8,
    0x1.f07c1f07c1f08p-8, -0x1.5995995995996p-6, 0x1.5555555555555p-4,
};

// Clenshaw's recurrence over c[0 .. N - 1], highest degree first:
//   b0 = c[0]; b1 = 0; b2 = 0;  for k = 1 .. N - 1:  b2 = b1;  b1 = b0;  b0 = (y*b1 - b2) + c[k];   result 0.5*(b0 - b2)
template <int N>
__host__ __device__ static inline double sf2_chebyshev(double y, const double (&c)[N])
{
    double b0 = c[0], b1 = 0.0, b2 = 0.0;
#pragma unroll 1
    for (int k = 1; k < N; ++k) {
        b2 = b1;
        b1 = b0;
        b0 = (y * b1 - b2) + c[k];
    }
    return 0.5 * (b0 - b2);
}

// exp(-|a|) I0(a): even.  NaN stays NaN (it fails a <= 8 and goes through 32/x).
__host__ __device__ static inline double sf2_i0e(double a)
{
    const double x = fabs(a);
    if (x <= 8.0) return sf2_chebyshev(x / 2.0 - 2.0, NLH_SF2_I0E_A);
    return sf2_chebyshev(32.0 / x - 2.0, NLH_SF2_I0E_B) / sqrt(x);
}

// exp(-|a|) I1(a): odd; i1e(-0.0) is +0.0 (the sign test is a < 0.0)
__host__ __device__ static inline double sf2_i1e(double a)
{
    const double x = fabs(a);
    double v;
    if (x <= 1.0) v = sf2_chebyshev(x * 4.0 - 2.0, NLH_SF2_I1E_A) * x;
    else if (x <= 8.0) v = sf2_chebyshev((x - 4.5) / 1.75, NLH_SF2_I1E_M);
    else v = sf2_chebyshev(32.0 / x - 2.0, NLH_SF2_I1E_B) / sqrt(x);
    return a < 0.0 ? -v : v;
}

// digamma(a) for a > 0, NaN otherwise (a NaN a included): the recurrence psi(a) = psi(a + 1) - 1/a up to a >= 10, ten steps at
// most, then the asymptotic series to B_14, the shift subtracted last:
//   r = 0;  while a < 10.0:  r = r + 1.0/a;  a = a + 1.0
//   z = 1.0/(a*a);  p = B[6];  for k = 5 .. 0:  p = p*z + B[k];   p = p*z
//   ((log(a) - 0.5/a) - p) - r
__host__ __device__ static inline double sf2_digamma(double a)
{
    if (!(a > 0.0)) return NAN;
    double r = 0.0;
    while (a < 10.0) {
        r = r + 1.0 / a;
        a = a + 1.0;
    }
    const double z = 1.0 / (a * a);
    double p = NLH_SF2_DIGAMMA_B[6];
#pragma unroll
    for (int k = 5; k >= 0; --k) p = p * z + NLH_SF2_DIGAMMA_B[k];
    p = p * z;
    return ((log(a) - 0.5 / a) - p) - r;
}
