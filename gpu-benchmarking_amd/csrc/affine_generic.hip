// affine_generic.hip -- the fused Helmholtz operator on affine elements, B^T [lambda je_e diag(q) + sum_ab ge_ab D_a^T
// diag(q) D_b] B with q the tensor product of the one-dimensional quadrature weights, for any extents: the fallback of
// the wave kernels of affine_wave.h.
//
// The kernel body of helmholtz_generic.h (helm_generic_body) with the AffineGeneric policy below for the metric: one
// workgroup per element (a grid-stride loop over elements), the same images in static LDS (four regions of one point
// image in 3D, three in 2D), one thread per
// output value of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of
// operations of the wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; q = qw2[k] (qw1[j] qw0[i]) (2D: qw1[j]
// qw0[i]); f_a = q (sum_b ge_ab du_b), b ascending; v = (((lambda je_e) q) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2];
// transposed k -> r', j -> q', i -> p'.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `je` is not
// dereferenced when has_j is false.  Latency-bound, not a roofline target.  Extents up to 12 per direction in 3D and 32
// in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM> struct AffineGeneric
{
    static constexpr bool SCALED = true;
    static constexpr int NCOMP   = DIM == 3 ? 6 : 3;
    const T *__restrict__ qw0, *__restrict__ qw1, *__restrict__ qw2, *__restrict__ ge, *__restrict__ je;
    const T lam;
    const bool has_j;
    const T *gc; // of the element
    T lj;

    __device__ __forceinline__ void element(uint64_t e, int)
    {
        gc = ge + e * (uint64_t)NCOMP;
        lj = has_j ? lam * je[e] : T(0);
    }
    __device__ __forceinline__ void coef(int, int, T (&gg)[NCOMP]) const
    {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
            gg[c] = gc[c];
    }
    __device__ __forceinline__ T scale(int x, int nq0, int nq1) const
    {
        const int i = x % nq0, kj = x / nq0;
        if constexpr (DIM == 3)
            return qw2[kj / nq1] * (qw1[kj % nq1] * qw0[i]);
        else
            return qw1[kj] * qw0[i];
    }
    __device__ __forceinline__ T mass(int, T q, T u) const { return has_j ? (lj * q) * u : T(0); }
};

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void affine_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ ge, const T *__restrict__ je, T lam, bool has_j,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
    AffineGeneric<T, DIM> met{qw0, qw1, qw2, ge, je, lam, has_j, nullptr, T(0)};
    helm_generic_body<T, DIM, NT>(lds, b0, b1, b2, d0, d1, d2, met, in, out, nelmt, nq0, nq1, nq2);
}

template <int DIM, typename T>
int launch_affine_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
    return launch_any_extent(affine_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             affine_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             affine_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                             x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.ge, x.je, x.lam, x.je != nullptr, a.in, a.out, a.nelmt,
                             (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_affine_generic<3, double>(const unsigned (&)[3], const HexArgs &, const AffineArgsT<double> &,
                                              hipStream_t);
template int launch_affine_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const AffineArgsT<float> &,
                                             hipStream_t);
template int launch_affine_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const AffineArgsT<double> &,
                                              hipStream_t);
template int launch_affine_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const AffineArgsT<float> &,
                                             hipStream_t);

// the bounds of the Helmholtz any-extent kernel
bool affine_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
