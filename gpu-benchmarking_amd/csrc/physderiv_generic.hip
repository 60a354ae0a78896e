// physderiv_generic.hip -- BwdTrans fused with the physical-space gradient, out_a = sum_b df_ab D_b B x, for any
// extents: the fallback of the wave kernels of physderiv_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; out_a = sum_b df_ab du_b (b ascending; no df: out_a = du_a).
// Two LDS regions of one point image each, P0 and P1 -- the derivatives go from the image of u to HBM through registers:
//   3D: in (P1) -> w1 (P0) -> w2 (P1) -> u (P0) -> du_0, du_1, du_2 (registers) -> out_0, out_1, out_2 (HBM)
//   2D: in (P1) -> w1 (P1, behind in) -> u (P0) -> du_0, du_1 (registers) -> out_0, out_1 (HBM)
// The forward sweeps and the derivatives of a point are the text of helm_generic_body (helmholtz_generic.h): the
// fragments frag/ae_forward_*.inc and frag/ae_deriv_*.inc; the bounds and the LDS classes are shared with that body too.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only: every launch is a single kernel node that
// needs no function attribute, capture-safe from the first call.  `df` is not dereferenced when has_df is false.
// Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void physderiv_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, bool has_df, const T *__restrict__ in,
    T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *P0 = lds, *P1 = lds + nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        const T *dfe = has_df ? df + e * (uint64_t)(DIM * DIM * nqt) : nullptr;
        T *o0 = out0 + e * (uint64_t)nqt, *o1 = out1 + e * (uint64_t)nqt;
        if constexpr (DIM == 2)
        {
            T *W1 = P1 + nmt; // w1 behind the modes in P1 (nmt + nm1 nq0 <= nqt + nq0 nq1)
#define AE_MODES P1
#define AE_W1 W1
#define AE_POINTS P0
#define AE_POINT_VALUE(s) s
#include "frag/ae_forward_2d.inc"
            // out_a = sum_b df_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                T x0, x1;
#define AE_DU0 x0
#define AE_DU1 x1
#include "frag/ae_deriv_2d.inc"
                if (has_df)
                {
                    o0[x] = sfma(dfe[1 * nqt + x], x1, dfe[0 * nqt + x] * x0);
                    o1[x] = sfma(dfe[3 * nqt + x], x1, dfe[2 * nqt + x] * x0);
                }
                else
                {
                    o0[x] = x0;
                    o1[x] = x1;
                }
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
            T *o2 = out2 + e * (uint64_t)nqt; // after the sweeps: named before them it moves instructions
            // out_a = sum_b df_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                T x0, x1, x2;
#define AE_DU0 x0
#define AE_DU1 x1
#define AE_DU2 x2
#include "frag/ae_deriv_3d.inc"
                if (has_df)
                {
                    o0[x] = sfma(dfe[2 * nqt + x], x2, sfma(dfe[1 * nqt + x], x1, dfe[0 * nqt + x] * x0));
                    o1[x] = sfma(dfe[5 * nqt + x], x2, sfma(dfe[4 * nqt + x], x1, dfe[3 * nqt + x] * x0));
                    o2[x] = sfma(dfe[8 * nqt + x], x2, sfma(dfe[7 * nqt + x], x1, dfe[6 * nqt + x] * x0));
                }
                else
                {
                    o0[x] = x0;
                    o1[x] = x1;
                    o2[x] = x2;
                }
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

template <int DIM, typename T>
int launch_physderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x, hipStream_t s)
{
    // The classes of the Helmholtz fallback by extents (64 threads up to 8^3 / 26^2).  This kernel needs 2 nqt scalars in
    // 3D and fewer than 3 nqt in 2D (nqt + nmt + nm1 nq0), where helm_need() is 4 nqt and 3 nqt: the small class keeps
    // its size, the large one holds 2 * 12^3 = 3456 >= 3 * 32^2.
    return launch_any_extent(physderiv_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             physderiv_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             physderiv_generic_kernel<T, DIM, kHelmLargeCap / 2, 256>, a.nelmt, s, a.b0, a.b1, basis2(a),
                             x.d0, x.d1, x.d2, x.df, x.df != nullptr, a.in, x.out0, x.out1, x.out2, a.nelmt, (int)nq[0],
                             (int)nq[1], (int)nq[2]);
}
template int launch_physderiv_generic<3, double>(const unsigned (&)[3], const HexArgs &, const PhysDerivArgsT<double> &,
                                                 hipStream_t);
template int launch_physderiv_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                const PhysDerivArgsT<float> &, hipStream_t);
template int launch_physderiv_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const PhysDerivArgsT<double> &,
                                                 hipStream_t);
template int launch_physderiv_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                const PhysDerivArgsT<float> &, hipStream_t);

bool physderiv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
