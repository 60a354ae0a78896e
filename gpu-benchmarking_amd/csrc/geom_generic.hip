// geom_generic.hip -- the geometric factors df, w, g, detj from the modal coordinates of every element, for any extents:
// the fallback of the wave kernels of geom_wave.h, and the affine form sf_geom_affine_* (the same kernel at one point).
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: per coordinate a the forward sweeps p -> i, q -> j, r -> k of X_a; J[a][b] = D_b X_a; then the point
// arithmetic of geom_point.h.  Four LDS regions of one point image each, R0 .. R3; the point images of the d coordinates
// stay in R0 .. R(d-1), the forward sweeps of coordinate a work in the regions behind its image:
//   3D, coordinate a: modes (R(a+1)) -> w1 (Ra) -> w2 (R(a+1)) -> X_a (Ra)
//   2D, coordinate a: modes (R(a+1)) -> w1 (behind the modes, fewer than 2 nqt scalars in all) -> X_a (Ra)
// so 4 nqt scalars in both dimensions, the classes of the Helmholtz fallback.  The d coordinates forward are
// frag/ae_fields_forward.inc and J of a point is frag/ae_jacobian.inc (any_extent.h), the text vecgrad_generic.hip
// includes too; they string frag/ae_forward_*.inc and frag/ae_deriv_*.inc together, the text of physderiv_generic.hip:
// a coordinate field goes through the arithmetic `in` goes through there.  This unit's own: the weight of the point
// (handed to ae_jacobian as AE_POINT_WITH), geom_point and the stores.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  An output that is null is not
// written (a run-time check per plane; the arithmetic is not compiled out here).  No workspace and static LDS only: every
// launch is a single kernel node that needs no function attribute, capture-safe from the first call.
// AFFINE: thread 0 evaluates the point (0, 0, 0) only and writes dfe[e][c], je[e] = |det|, ge[e][c] = je sum_x dfe dfe:
// the forward sweeps and the derivative sums are those of the deformed call, so dfe and je equal its point 0 bit for bit.
// Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "geom_args.h"
#include "geom_point.h"
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT, bool AFFINE>
__global__ __launch_bounds__(NT) void geom_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ x0, const T *__restrict__ x1, const T *__restrict__ x2,
    T *__restrict__ df, T *__restrict__ w, T *__restrict__ g, T *__restrict__ detj, uint64_t nelmt, int nq0, int nq1,
    int nq2)
{
    constexpr int DD = DIM * DIM, NC = DIM * (DIM + 1) / 2;
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *R0 = lds, *R1 = lds + nqt, *R2 = lds + 2 * nqt, *R3 = lds + 3 * nqt;
    const bool has_q = !AFFINE && (w != nullptr || g != nullptr); // qw_d are read only then
    const int npts   = AFFINE ? 1 : nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
#include "frag/ae_fields_forward.inc"
        // J[a][b] = D_b X_a of the point, then the factors of the point
        for (int x = tid; x < npts; x += NT)
        {
            T J[DIM][DIM];
            T q = T(0);
#define AE_POINT_WITH(i, j, k)                                                                                         \
    if (has_q)                                                                                                         \
        q = DIM == 3 ? qw2[k] * (qw1[j] * qw0[i]) : qw1[j] * qw0[i];
#include "frag/ae_jacobian.inc"
            GeomPoint<DIM, T> p;
            geom_point<DIM, kGeomAll, !AFFINE>(J, q, p);
            // AFFINE: one value per element and component; else one plane of nqt points per element and component
            const uint64_t ps = AFFINE ? 1 : (uint64_t)nqt, at = AFFINE ? 0 : (uint64_t)x;
            if (df)
                for (int c = 0; c < DD; ++c)
                    df[(e * DD + c) * ps + at] = p.df[c];
            if (w)
                w[e * ps + at] = p.w;
            if (g)
                for (int c = 0; c < NC; ++c)
                    g[(e * NC + c) * ps + at] = p.g[c];
            if (detj)
                detj[e * ps + at] = p.det;
        }
        __syncthreads(); // the next element overwrites the images
    }
}

// LDS the extents need: four point images in both dimensions
static inline unsigned geom_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return 4 * nq0 * nq1 * (dim == 3 ? nq2 : 1);
}

template <int DIM, typename T, bool AFFINE>
static int launch_geom_any(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    // the classes of the Helmholtz fallback: 64 threads while four images fit the small class, else 256 threads and the
    // large one (3D 12^3 needs 6912 = kHelmLargeCap, 2D 32^2 4096)
    return launch_any_extent(geom_generic_built(DIM, nq[0], nq[1], nq[2]),
                             geom_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             geom_generic_kernel<T, DIM, kHelmSmallCap, 64, AFFINE>,
                             geom_generic_kernel<T, DIM, kHelmLargeCap, 256, AFFINE>, a.nelmt, s, a.b0, a.b1, basis2(a),
                             x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.x0, x.x1, x.x2, x.df, x.w, x.g, x.detj, a.nelmt,
                             (int)nq[0], (int)nq[1], (int)nq[2]);
}

template <int DIM, typename T>
int launch_geom_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    return launch_geom_any<DIM, T, false>(nq, a, x, s);
}
template <int DIM, typename T>
int launch_geom_affine(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    return launch_geom_any<DIM, T, true>(nq, a, x, s);
}
#define SF_GEOM_GENERIC(DIM, T)                                                                                        \
    template int launch_geom_generic<DIM, T>(const unsigned (&)[3], const ArgsT<DIM, T> &, const GeomArgsT<T> &,       \
                                             hipStream_t);                                                             \
    template int launch_geom_affine<DIM, T>(const unsigned (&)[3], const ArgsT<DIM, T> &, const GeomArgsT<T> &,        \
                                            hipStream_t);
SF_GEOM_GENERIC(3, double)
SF_GEOM_GENERIC(3, float)
SF_GEOM_GENERIC(2, double)
SF_GEOM_GENERIC(2, float)
#undef SF_GEOM_GENERIC

bool geom_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2) &&
           geom_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kHelmLargeCap;
}

} // namespace sf
