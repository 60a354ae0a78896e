// helmholtz_generic.hip -- the fused Helmholtz operator B^T [lambda diag(w) + sum_ab D_a^T diag(G_ab) D_b] B for any
// extents: the fallback of the wave kernels of helmholtz_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; f_a = sum_b G_ab du_b (b ascending);
// v = ((lambda w) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]; transposed k -> r', j -> q', i -> p'.
// Four (2D: three) LDS regions of one point image each, P0 .. P3:
//   3D: in (P1) -> w1 (P0) -> w2 (P1) -> u (P0) -> du_0, du_1, du_2 (P1, P2, P3) -> f_0, f_1, f_2 in place and
//       (lambda w) u over u (P0) -> v over it (P0) -> t1 (P1) -> t2 (P2) -> out (HBM)
//   2D: in (P1) -> w1 (P2) -> u (P0) -> du_0, du_1 (P1, P2) -> f_0, f_1 in place, (lambda w) u (P0) -> v (P0) -> t1 (P1)
//       -> out (HBM)
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `w` is not
// dereferenced when has_w is false.  Latency-bound (a barrier per sweep, one element per workgroup), not a roofline
// target.  Extents up to 12 per direction in 3D (four images of 12^3 doubles: 55 296 bytes of the 64 KB of static LDS)
// and 32 in 2D; beyond, SF_ENOTBUILT.
// The kernel body, helm_generic_body, is in helmholtz_generic.h and shared with affine_generic.hip; the metric of this
// unit is the PlaneGeneric policy below: the planes g and the weight w per point.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM> struct PlaneGeneric
{
    static constexpr bool SCALED = false;
    static constexpr int NCOMP   = DIM == 3 ? 6 : 3;
    const T *__restrict__ g, *__restrict__ w;
    const T lam;
    const bool has_w;
    const T *ge, *wt; // of the element

    __device__ __forceinline__ void element(uint64_t e, int nqt)
    {
        ge = g + e * (uint64_t)(NCOMP * nqt);
        wt = has_w ? w + e * (uint64_t)nqt : nullptr;
    }
    __device__ __forceinline__ void coef(int x, int nqt, T (&gg)[NCOMP]) const
    {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
            gg[c] = ge[c * nqt + x];
    }
    __device__ __forceinline__ T scale(int, int, int) const { return T(1); }
    __device__ __forceinline__ T mass(int x, T, T u) const { return has_w ? (lam * wt[x]) * u : T(0); }
};

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void helmholtz_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ g, const T *__restrict__ w, T lam,
    bool has_w, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
    PlaneGeneric<T, DIM> met{g, w, lam, has_w, nullptr, nullptr};
    helm_generic_body<T, DIM, NT>(lds, b0, b1, b2, d0, d1, d2, met, in, out, nelmt, nq0, nq1, nq2);
}

template <int DIM, typename T>
int launch_helmholtz_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s)
{
    return launch_any_extent(helmholtz_generic_built(DIM, nq[0], nq[1], nq[2]),
                             helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             helmholtz_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             helmholtz_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                             x.d1, x.d2, x.g, x.w, x.lam, x.w != nullptr, a.in, a.out, a.nelmt, (int)nq[0], (int)nq[1],
                             (int)nq[2]);
}
template int launch_helmholtz_generic<3, double>(const unsigned (&)[3], const HexArgs &, const HelmArgsT<double> &,
                                                 hipStream_t);
template int launch_helmholtz_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const HelmArgsT<float> &,
                                                hipStream_t);
template int launch_helmholtz_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const HelmArgsT<double> &,
                                                 hipStream_t);
template int launch_helmholtz_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const HelmArgsT<float> &,
                                                hipStream_t);

bool helmholtz_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
