// iprodderiv_generic.hip -- IProductWRTDerivBase, out = sum_b B^T D_b^T (w sum_a df_ab in_a), for any extents: the
// fallback of the wave kernels of iprodderiv_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: t_b = sum_a df_ab in_a (a ascending; no df: t_b = in_b); g_b = w t_b (no w: g_b = t_b);
// v = (D_0^T g_0 + D_1^T g_1) [+ D_2^T g_2]; transposed k -> r', j -> q', i -> p'.
// Four (2D: three) LDS regions of one point image each, P0 .. P3:
//   3D: in_0, in_1, in_2 (HBM) -> g_0, g_1, g_2 (P1, P2, P3) -> v (P0) -> t1 (P1) -> t2 (P2) -> out (HBM)
//   2D: in_0, in_1 (HBM) -> g_0, g_1 (P1, P2) -> v (P0) -> t1 (P1) -> out (HBM)
// The transposed derivatives of a point and the back sweeps are the text of helm_generic_body (helmholtz_generic.h): the
// fragments frag/ae_deriv_transposed_*.inc and frag/ae_transposed_*.inc; the bounds and the LDS classes are shared with
// that body too.  Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only: every launch is a single kernel node that
// needs no function attribute, capture-safe from the first call.  `df` / `w` are not dereferenced when has_df / has_w is
// false.  Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per
// direction in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void iprodderiv_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, bool has_df, const T *__restrict__ w,
    bool has_w, const T *__restrict__ in0, const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out,
    uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *P0 = lds, *P1 = lds + nqt, *P2 = lds + 2 * nqt, *P3 = lds + (DIM == 3 ? 3 : 2) * nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *f0  = in0 + e * (uint64_t)nqt, *f1 = in1 + e * (uint64_t)nqt;
        const T *dfe = has_df ? df + e * (uint64_t)(DIM * DIM * nqt) : nullptr;
        const T *we  = has_w ? w + e * (uint64_t)nqt : nullptr;
        T *dst       = out + e * (uint64_t)nmt;
        if constexpr (DIM == 2)
        {
            // t_b = sum_a df_ab in_a, g_b = w t_b (every thread touches its own points only)
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = f0[x], x1 = f1[x];
                T t0 = x0, t1 = x1;
                if (has_df)
                {
                    t0 = sfma(dfe[2 * nqt + x], x1, dfe[0 * nqt + x] * x0);
                    t1 = sfma(dfe[3 * nqt + x], x1, dfe[1 * nqt + x] * x0);
                }
                if (has_w)
                {
                    const T ww = we[x];
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
            // t_b = sum_a df_ab in_a, g_b = w t_b (every thread touches its own points only)
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = f0[x], x1 = f1[x], x2 = f2[x];
                T t0 = x0, t1 = x1, t2 = x2;
                if (has_df)
                {
                    t0 = sfma(dfe[6 * nqt + x], x2, sfma(dfe[3 * nqt + x], x1, dfe[0 * nqt + x] * x0));
                    t1 = sfma(dfe[7 * nqt + x], x2, sfma(dfe[4 * nqt + x], x1, dfe[1 * nqt + x] * x0));
                    t2 = sfma(dfe[8 * nqt + x], x2, sfma(dfe[5 * nqt + x], x1, dfe[2 * nqt + x] * x0));
                }
                if (has_w)
                {
                    const T ww = we[x];
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
int launch_iprodderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const IprodDerivArgsT<T> &x, hipStream_t s)
{
    // the images and the classes of the Helmholtz fallback: 4 (2D: 3) nqt scalars
    return launch_any_extent(iprodderiv_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             iprodderiv_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             iprodderiv_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                             x.d1, x.d2, x.df, x.df != nullptr, x.w, x.w != nullptr, x.in0, x.in1, x.in2, a.out, a.nelmt,
                             (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_iprodderiv_generic<3, double>(const unsigned (&)[3], const HexArgs &, const IprodDerivArgsT<double> &,
                                                  hipStream_t);
template int launch_iprodderiv_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                 const IprodDerivArgsT<float> &, hipStream_t);
template int launch_iprodderiv_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const IprodDerivArgsT<double> &,
                                                  hipStream_t);
template int launch_iprodderiv_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                 const IprodDerivArgsT<float> &, hipStream_t);

bool iprodderiv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
