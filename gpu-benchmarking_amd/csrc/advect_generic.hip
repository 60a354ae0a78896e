// advect_generic.hip -- the weak advection term out_a = B^T [w (c . grad) B in_a] for any extents: the fallback of the wave
// kernels of advect_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: per field a the forward sweeps p -> i, q -> j, r -> k of in_a; J[a][b] = D_b u_a; beta_b = sum_j c_j
// df[j*d + b]; r_a = w (sum_b beta_b J[a][b]); the transposed sweeps k -> r', j -> q', i -> p'.  The fields go through
// one after the other, each through two LDS regions A and B of one point image:
//   3D: in_a (B) -> w1 (A) -> w2 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> t2 (B) -> out_a (HBM)
//   2D: in_a (A) -> w1 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> out_a (HBM)
// so beta of a point is formed once per field here (the same arithmetic on the same values: the same bits), where the
// wave kernels form it once.  The body of the loop over the fields is frag/ae_advect_field.inc (any_extent.h), shared with
// affine_advect_generic.hip: it strings frag/ae_forward_*.inc, frag/ae_deriv_*.inc and frag/ae_transposed_*.inc together
// around the point step.  This unit's own: where df comes from (AE_ADV_DF, the planes) and the value a point stores
// (AE_ADV_VALUE, the weight plane times the sum).  The LDS classes are in advect_args.h.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.
// Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D, the bounds of the Helmholtz fallback; beyond, SF_ENOTBUILT.
#include "advect_args.h"
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void advect_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ w,
    const T *__restrict__ c0, const T *__restrict__ c1, const T *__restrict__ c2, const T *__restrict__ x0,
    const T *__restrict__ x1, const T *__restrict__ x2, T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2,
    uint64_t nelmt, int nf, int nq0, int nq1, int nq2)
{
    constexpr int DD = DIM * DIM;
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *A = lds, *B = lds + nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *dfe = df + e * (uint64_t)(DD * nqt);
        const T *we  = w + e * (uint64_t)nqt;
        const T *ce0 = c0 + e * (uint64_t)nqt, *ce1 = c1 + e * (uint64_t)nqt;
        const T *ce2 = DIM == 3 ? c2 + e * (uint64_t)nqt : nullptr;
        for (int a = 0; a < nf; ++a)
        {
#define AE_ADV_DF(c) dfe[(c) * nqt + x]
#define AE_ADV_VALUE(r, i, j, k) B[x] = we[x] * (r);
#include "frag/ae_advect_field.inc"
        }
    }
}

template <int DIM, typename T>
int launch_advect_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s)
{
    return launch_any_extent(advect_generic_built(DIM, nq[0], nq[1], nq[2]),
                             advect_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kAdvSmallCap,
                             advect_generic_kernel<T, DIM, kAdvSmallCap, 64>,
                             advect_generic_kernel<T, DIM, kAdvLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                             x.d1, x.d2, x.df, x.w, x.c0, x.c1, x.c2, x.in0, x.in1, x.in2, x.out0, x.out1, x.out2, a.nelmt,
                             x.nf, (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_advect_generic<3, double>(const unsigned (&)[3], const HexArgs &, const AdvectArgsT<double> &,
                                              hipStream_t);
template int launch_advect_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const AdvectArgsT<float> &,
                                             hipStream_t);
template int launch_advect_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const AdvectArgsT<double> &,
                                              hipStream_t);
template int launch_advect_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const AdvectArgsT<float> &,
                                             hipStream_t);

// within the extent bounds of the Helmholtz fallback AND two point images fit the large LDS class (true for every extent
// within the bounds: 3D 12^3 needs 3456, 2D 32^2 2048; derived all the same, not assumed)
bool advect_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2) &&
           advect_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kAdvLargeCap;
}

} // namespace sf
