// any_extent.h -- what the any-extent kernels of iproduct_generic.hip, mass_generic.hip and helmholtz_generic.hip share:
// the scalar FMA, the ascending strided dot product of their sweeps, and the launch of one of their two LDS classes.
#pragma once

#include "sf_dispatch.h"

namespace sf
{

__device__ __forceinline__ double sfma(double a, double b, double c)
{
    return __builtin_fma(a, b, c);
}
__device__ __forceinline__ float sfma(float a, float b, float c)
{
    return __builtin_fmaf(a, b, c);
}

// a = sum_{m < n} u[m*us] * b[m*bs], ascending m, the first product a multiply
template <typename T> __device__ __forceinline__ T dot_strided(const T *u, int us, const T *b, int bs, int n)
{
    T a = u[0] * b[0];
    for (int m = 1; m < n; ++m)
        a = sfma(u[m * us], b[m * bs], a);
    return a;
}

// One workgroup per element up to 2^22 of them (the kernels' grid-stride loop takes the rest): the instantiation of the
// small LDS class with 64 threads when the images fit it, that of the large class with 256 otherwise.
template <class KS, class KL, class... A>
inline int launch_lds_class(bool small, KS small_kern, KL large_kern, uint64_t nelmt, hipStream_t s, A... args)
{
    const unsigned grid = nelmt < (1ull << 22) ? (unsigned)nelmt : (1u << 22);
    if (small)
        small_kern<<<grid, 64, 0, s>>>(args...);
    else
        large_kern<<<grid, 256, 0, s>>>(args...);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

// b2 of the descriptor, null in 2D
template <typename T> inline const T *basis2(const HexArgsT<T> &a)
{
    return a.b2;
}
template <typename T> inline const T *basis2(const QuadArgsT<T> &)
{
    return nullptr;
}

} // namespace sf
