// affine_deriv_generic.hip -- the gradient and the weak divergence on affine elements for any extents: the fallbacks of
// the wave kernels of affine_deriv_wave.h.
//
//   gradient:         out_a = sum_b dfe[e][a*d + b] D_b B x_e
//   weak divergence:  out_e = sum_b B^T D_b^T ((je[e] q) sum_a dfe[e][a*d + b] in_a),  q = qw2[k] (qw1[j] qw0[i])
//
// The kernels of physderiv_generic.hip and iprodderiv_generic.hip with the d*d constants of the element read once per
// element in the place of the planes, and the weight formed from je[e] and the one-dimensional quadrature weights: one
// workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value of a
// sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the wave
// kernels, hence on planes filled with the constants the bits of the deformed fallbacks.  The LDS regions, the
// fragments (frag/ae_*.inc), the bounds and the LDS classes are those of the two deformed fallbacks.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `je` and
// `qw_d` are not dereferenced when has_w is false.  Latency-bound, not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void affine_physderiv_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ dfe, const T *__restrict__ in,
    T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *P0 = lds, *P1 = lds + nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        T dd[DIM * DIM]; // the constants of the element
#pragma unroll
        for (int c = 0; c < DIM * DIM; ++c)
            dd[c] = dfe[e * (uint64_t)(DIM * DIM) + c];
        T *o0 = out0 + e * (uint64_t)nqt, *o1 = out1 + e * (uint64_t)nqt;
        if constexpr (DIM == 2)
        {
            T *W1 = P1 + nmt; // w1 behind the modes in P1 (nmt + nm1 nq0 <= nqt + nq0 nq1)
#define AE_MODES P1
#define AE_W1 W1
#define AE_POINTS P0
#define AE_POINT_VALUE(s) s
#include "frag/ae_forward_2d.inc"
            // out_a = sum_b dfe_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                T x0, x1;
#define AE_DU0 x0
#define AE_DU1 x1
#include "frag/ae_deriv_2d.inc"
                o0[x] = sfma(dd[1], x1, dd[0] * x0);
                o1[x] = sfma(dd[3], x1, dd[2] * x0);
            }
        }
        else
        {
#define AE_MODES P1
#define AE_W1 P0
#define AE_W2 P1
#define AE_POINTS P0
#define AE_POINT_VALUE(s) s
#include "frag/ae_forward_3d.inc"
            T *o2 = out2 + e * (uint64_t)nqt;
            // out_a = sum_b dfe_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                T x0, x1, x2;
#define AE_DU0 x0
#define AE_DU1 x1
#define AE_DU2 x2
#include "frag/ae_deriv_3d.inc"
                o0[x] = sfma(dd[2], x2, sfma(dd[1], x1, dd[0] * x0));
                o1[x] = sfma(dd[5], x2, sfma(dd[4], x1, dd[3] * x0));
                o2[x] = sfma(dd[8], x2, sfma(dd[7], x1, dd[6] * x0));
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void affine_iprodderiv_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ dfe, const T *__restrict__ je, bool has_w,
    const T *__restrict__ in0, const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out,
    uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *P0 = lds, *P1 = lds + nqt, *P2 = lds + 2 * nqt, *P3 = lds + (DIM == 3 ? 3 : 2) * nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *f0 = in0 + e * (uint64_t)nqt, *f1 = in1 + e * (uint64_t)nqt;
        T dd[DIM * DIM]; // the constants of the element
#pragma unroll
        for (int c = 0; c < DIM * DIM; ++c)
            dd[c] = dfe[e * (uint64_t)(DIM * DIM) + c];
        const T jee = has_w ? je[e] : T(0);
        T *dst      = out + e * (uint64_t)nmt;
        if constexpr (DIM == 2)
        {
            // t_b = sum_a dfe_ab in_a, g_b = (je q) t_b (every thread touches its own points only)
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = f0[x], x1 = f1[x];
                T t0 = sfma(dd[2], x1, dd[0] * x0);
                T t1 = sfma(dd[3], x1, dd[1] * x0);
                if (has_w)
                {
                    const T ww = jee * (qw1[x / nq0] * qw0[x % nq0]);
                    t0 = ww * t0, t1 = ww * t1;
                }
                P1[x] = t0;
                P2[x] = t1;
            }
            __syncthreads();
            // v = D_0^T g_0 + D_1^T g_1
            for (int x = tid; x < nqt; x += NT)
            {
#include "frag/ae_deriv_transposed_2d.inc"
                P0[x] = t0 + t1;
            }
            __syncthreads();
#define AE_POINTS P0
#define AE_T1 P1
#include "frag/ae_transposed_2d.inc"
        }
        else
        {
            const T *f2 = in2 + e * (uint64_t)nqt;
            // t_b = sum_a dfe_ab in_a, g_b = (je q) t_b (every thread touches its own points only)
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = f0[x], x1 = f1[x], x2 = f2[x];
                T t0 = sfma(dd[6], x2, sfma(dd[3], x1, dd[0] * x0));
                T t1 = sfma(dd[7], x2, sfma(dd[4], x1, dd[1] * x0));
                T t2 = sfma(dd[8], x2, sfma(dd[5], x1, dd[2] * x0));
                if (has_w)
                {
                    const int kj = x / nq0;
                    const T ww   = jee * (qw2[kj / nq1] * (qw1[kj % nq1] * qw0[x % nq0]));
                    t0 = ww * t0, t1 = ww * t1, t2 = ww * t2;
                }
                P1[x] = t0;
                P2[x] = t1;
                P3[x] = t2;
            }
            __syncthreads();
            // v = (D_0^T g_0 + D_1^T g_1) + D_2^T g_2
            for (int x = tid; x < nqt; x += NT)
            {
#include "frag/ae_deriv_transposed_3d.inc"
                P0[x] = (t0 + t1) + t2;
            }
            __syncthreads();
#define AE_POINTS P0
#define AE_T1 P1
#define AE_T2 P2
#include "frag/ae_transposed_3d.inc"
        }
        __syncthreads(); // the next element overwrites the images
    }
}

template <int DIM, typename T>
int launch_affine_physderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffinePhysDerivArgsT<T> &x,
                                    hipStream_t s)
{
    // the classes of physderiv_generic.hip: 2 nqt scalars in 3D, fewer than 3 nqt in 2D
    return launch_any_extent(affine_deriv_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             affine_physderiv_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             affine_physderiv_generic_kernel<T, DIM, kHelmLargeCap / 2, 256>, a.nelmt, s, a.b0, a.b1,
                             basis2(a), x.d0, x.d1, x.d2, x.dfe, a.in, x.out0, x.out1, x.out2, a.nelmt, (int)nq[0],
                             (int)nq[1], (int)nq[2]);
}
template int launch_affine_physderiv_generic<3, double>(const unsigned (&)[3], const HexArgs &,
                                                        const AffinePhysDerivArgsT<double> &, hipStream_t);
template int launch_affine_physderiv_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                       const AffinePhysDerivArgsT<float> &, hipStream_t);
template int launch_affine_physderiv_generic<2, double>(const unsigned (&)[3], const QuadArgs &,
                                                        const AffinePhysDerivArgsT<double> &, hipStream_t);
template int launch_affine_physderiv_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                       const AffinePhysDerivArgsT<float> &, hipStream_t);

template <int DIM, typename T>
int launch_affine_iprodderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineIprodDerivArgsT<T> &x,
                                     hipStream_t s)
{
    // the images and the classes of the Helmholtz fallback: 4 (2D: 3) nqt scalars
    return launch_any_extent(affine_deriv_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             affine_iprodderiv_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             affine_iprodderiv_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1,
                             basis2(a), x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.dfe, x.je, x.je != nullptr, x.in0, x.in1,
                             x.in2, a.out, a.nelmt, (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_affine_iprodderiv_generic<3, double>(const unsigned (&)[3], const HexArgs &,
                                                         const AffineIprodDerivArgsT<double> &, hipStream_t);
template int launch_affine_iprodderiv_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                        const AffineIprodDerivArgsT<float> &, hipStream_t);
template int launch_affine_iprodderiv_generic<2, double>(const unsigned (&)[3], const QuadArgs &,
                                                         const AffineIprodDerivArgsT<double> &, hipStream_t);
template int launch_affine_iprodderiv_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                        const AffineIprodDerivArgsT<float> &, hipStream_t);

// the bounds of the Helmholtz any-extent kernel
bool affine_deriv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
