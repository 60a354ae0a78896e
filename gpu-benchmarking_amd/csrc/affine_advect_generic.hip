// affine_advect_generic.hip -- the weak advection term on affine elements, out_a = B^T [(je q) (c . grad) B in_a], for any
// extents: the fallback of the wave kernels of affine_advect_wave.h.
//
// The kernel of advect_generic.hip with the d*d constants of the element read once per element in the place of the
// planes, and the weight formed from je[e] and the one-dimensional quadrature weights as je * (qw2 * (qw1 * qw0)): one
// workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value of a
// sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the wave
// kernels, hence their bits, and on planes filled with the constants the bits of the deformed fallback.  The fields go
// through one after the other, each through the two LDS regions A and B of advect_generic.hip:
//   3D: in_a (B) -> w1 (A) -> w2 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> t2 (B) -> out_a (HBM)
//   2D: in_a (A) -> w1 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> out_a (HBM)
// so beta and the weight of a point are formed once per field here (the same arithmetic on the same values: the same
// bits), where the wave kernels form them once.  The body of the loop over the fields is frag/ae_advect_field.inc
// (any_extent.h), the text advect_generic.hip includes.  This unit's own: the element set-up, where df comes from
// (AE_ADV_DF, the constants) and the value a point stores (AE_ADV_VALUE, with the weight formed from je and qw_d).  The
// LDS classes are those of advect_generic.hip, in advect_args.h.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `je` and
// `qw_d` are not dereferenced when has_w is false.  Latency-bound, not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D, the bounds of the Helmholtz fallback; beyond, SF_ENOTBUILT.
#include "advect_args.h"
#include "affine_advect_args.h"
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void affine_advect_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ dfe, const T *__restrict__ je, bool has_w,
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
        T dd[DD]; // the constants of the element
#pragma unroll
        for (int c = 0; c < DD; ++c)
            dd[c] = dfe[e * (uint64_t)DD + c];
        const T jee   = has_w ? je[e] : T(0);
        const T *ce0 = c0 + e * (uint64_t)nqt, *ce1 = c1 + e * (uint64_t)nqt;
        const T *ce2 = DIM == 3 ? c2 + e * (uint64_t)nqt : nullptr;
        for (int a = 0; a < nf; ++a)
        {
#define AE_ADV_DF(c) dd[c]
#define AE_ADV_VALUE(r, i, j, k)                                                                                       \
    T v = (r);                                                                                                         \
    if (has_w)                                                                                                         \
        v = (jee * (DIM == 3 ? qw2[k] * (qw1[j] * qw0[i]) : qw1[j] * qw0[i])) * v;                                     \
    B[x] = v;
#include "frag/ae_advect_field.inc"
        }
    }
}

template <int DIM, typename T>
int launch_affine_advect_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x,
                                 hipStream_t s)
{
    return launch_any_extent(affine_advect_generic_built(DIM, nq[0], nq[1], nq[2]),
                             advect_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kAdvSmallCap,
                             affine_advect_generic_kernel<T, DIM, kAdvSmallCap, 64>,
                             affine_advect_generic_kernel<T, DIM, kAdvLargeCap, 256>, a.nelmt, s, a.b0, a.b1,
                             basis2(a), x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.dfe, x.je, x.je != nullptr, x.c0, x.c1,
                             x.c2, x.in0, x.in1, x.in2, x.out0, x.out1, x.out2, a.nelmt, x.nf, (int)nq[0], (int)nq[1],
                             (int)nq[2]);
}
template int launch_affine_advect_generic<3, double>(const unsigned (&)[3], const HexArgs &,
                                                     const AffineAdvectArgsT<double> &, hipStream_t);
template int launch_affine_advect_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                    const AffineAdvectArgsT<float> &, hipStream_t);
template int launch_affine_advect_generic<2, double>(const unsigned (&)[3], const QuadArgs &,
                                                     const AffineAdvectArgsT<double> &, hipStream_t);
template int launch_affine_advect_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                    const AffineAdvectArgsT<float> &, hipStream_t);

// within the extent bounds of the Helmholtz fallback AND two point images fit the large LDS class (true for every extent
// within the bounds; derived all the same, not assumed)
bool affine_advect_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2) &&
           advect_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kAdvLargeCap;
}

} // namespace sf
