// any_extent.h -- what the any-extent kernels of iproduct_generic.hip, mass_generic.hip, helmholtz_generic.h (with
// helmholtz_generic.hip and affine_generic.hip), physderiv_generic.hip, iprodderiv_generic.hip and the units built on
// them (geom_, advect_, affine_advect_ and vecgrad_generic.hip) share: the scalar FMA, the ascending strided dot product
// of their sweeps, and the guarded launch of one of their two LDS classes.
// The kernel text they share is in frag/ae_*.inc, #included in place (each fragment opens with its contract):
//   ae_prologue.inc                      the element constants
//   ae_forward_{2d,3d}.inc               modes staged, forward sweeps p -> i, q -> j, r -> k   (mass, Helmholtz, physderiv)
//   ae_deriv_{2d,3d}.inc                 du_a of a point                                       (Helmholtz, physderiv)
//   ae_deriv_transposed_{2d,3d}.inc      D_a^T of a point's terms                              (Helmholtz, iprodderiv)
//   ae_transposed_{2d,3d}.inc            transposed sweeps k -> r', j -> q', i -> p'           (mass, Helmholtz, iprodderiv)
// and, stringing those together for the kernels over several fields:
//   ae_fields_forward.inc                d fields forward into the images R0 .. R(d-1)         (geom, vecgrad)
//   ae_jacobian.inc                      J[a][b] = D_b u_a of a point                          (geom, vecgrad)
//   ae_advect_field.inc                  one field of the advection term, modes in to modes out (advect, affine advect)
// The names the kernels agree on, which the fragments take from the scope: T, DIM, NT; nq0 nq1 nq2; nm0 nm1 nm2, nz, n01,
// nqt, nmt, tid (ae_prologue.inc); b0 b1 b2, d0 d1 d2; src, dst of the element; x, the index of a loop over points; P0 ..
// P3, the point images of the derivative kernels.  The kernels over several fields add: e, the element; x0 x1 x2, the
// modes of the fields; R0 .. R3, the four regions of geom and vecgrad, and J[DIM][DIM]; A, B, the two regions of the
// advection kernels, with a (the field), out0 out1 out2 and ce0 ce1 ce2 (the planes of c of the element).  The images of
// a sweep are parameters: AE_* macros that the kernel defines just before the #include and the fragment undefines, so
// that a definition left out does not compile.
// iproduct_generic.hip sweeps in the other order and keeps its own text; only its launch is shared.
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

// The launch of every any-extent operator: extents that are not built answer SF_ENOTBUILT, an empty batch is done.
// Otherwise one workgroup per element up to 2^22 of them (the kernels' grid-stride loop takes the rest): the
// instantiation of the small LDS class with 64 threads when the images fit it, that of the large class with 256 otherwise.
template <class KS, class KL, class... A>
inline int launch_any_extent(bool built, bool small, KS small_kern, KL large_kern, uint64_t nelmt, hipStream_t s, A... args)
{
    if (!built)
        return SF_ENOTBUILT;
    if (nelmt == 0)
        return SF_OK;
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
