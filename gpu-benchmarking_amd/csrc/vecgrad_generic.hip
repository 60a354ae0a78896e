// vecgrad_generic.hip -- the gradient, divergence and curl of a vector field at the quadrature points for any extents: the
// fallback of the wave kernels of vecgrad_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: per field a the forward sweeps p -> i, q -> j, r -> k of in_a; J[a][b] = D_b u_a; grad[a][j] = sum_b
// df[j*d + b] J[a][b], b ascending; div and curl plain sums and differences of the rounded entries: in float64 the
// result is that of the wave kernels bit for bit.  The four LDS regions of geom_generic.hip, R0 .. R3, of one point image
// each: the point images of the d fields stay in R0 .. R(d-1) while the point step gathers J, the forward sweeps of
// field a work in the regions behind its image:
//   3D, field a: modes (R(a+1)) -> w1 (Ra) -> w2 (R(a+1)) -> u_a (Ra)
//   2D, field a: modes (R(a+1)) -> w1 (behind the modes, fewer than 2 nqt scalars in all) -> u_a (Ra)
// The d fields forward are frag/ae_fields_forward.inc and J of a point is frag/ae_jacobian.inc (any_extent.h), shared with
// geom_generic.hip; they string frag/ae_forward_*.inc and frag/ae_deriv_*.inc together, the text of
// physderiv_generic.hip: field a goes through the arithmetic `in` goes through there, so plane a*d + j of grad equals
// output j of that kernel on in_a bit for bit.  This unit's own: grad of the point and the stores.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  An output that is null is not
// written (a run-time check per output).  No workspace and static LDS only: every launch is a single kernel node that
// needs no function attribute, capture-safe from the first call.
// Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"
#include "vecgrad_args.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void vecgrad_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ x0,
    const T *__restrict__ x1, const T *__restrict__ x2, T *__restrict__ grad, T *__restrict__ div, T *__restrict__ curl0,
    T *__restrict__ curl1, T *__restrict__ curl2, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    constexpr int DD = DIM * DIM;
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *R0 = lds, *R1 = lds + nqt, *R2 = lds + 2 * nqt, *R3 = lds + 3 * nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
#include "frag/ae_fields_forward.inc"
        // J[a][b] = D_b u_a of the point, then grad of the point and what is asked for of it
        const T *dfe = df + e * (uint64_t)(DD * nqt);
        for (int x = tid; x < nqt; x += NT)
        {
            T J[DIM][DIM], g[DIM][DIM];
#define AE_POINT_WITH(i, j, k)
#include "frag/ae_jacobian.inc"
            if constexpr (DIM == 2)
            {
                for (int a = 0; a < 2; ++a)
                    for (int j = 0; j < 2; ++j)
                        g[a][j] = sfma(dfe[(2 * j + 1) * nqt + x], J[a][1], dfe[(2 * j) * nqt + x] * J[a][0]);
            }
            else
            {
                for (int a = 0; a < 3; ++a)
                    for (int j = 0; j < 3; ++j)
                        g[a][j] = sfma(dfe[(3 * j + 2) * nqt + x], J[a][2],
                                       sfma(dfe[(3 * j + 1) * nqt + x], J[a][1], dfe[(3 * j) * nqt + x] * J[a][0]));
            }
            if (grad)
                for (int c = 0; c < DD; ++c)
                    grad[(e * DD + c) * (uint64_t)nqt + x] = g[c / DIM][c % DIM];
            if constexpr (DIM == 2)
            {
                if (div)
                    div[e * (uint64_t)nqt + x] = g[0][0] + g[1][1];
                if (curl0)
                    curl0[e * (uint64_t)nqt + x] = g[1][0] - g[0][1];
            }
            else
            {
                if (div)
                    div[e * (uint64_t)nqt + x] = (g[0][0] + g[1][1]) + g[2][2];
                if (curl0)
                {
                    curl0[e * (uint64_t)nqt + x] = g[2][1] - g[1][2];
                    curl1[e * (uint64_t)nqt + x] = g[0][2] - g[2][0];
                    curl2[e * (uint64_t)nqt + x] = g[1][0] - g[0][1];
                }
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

// LDS the extents need: four point images in both dimensions, as geom_generic.hip
static inline unsigned vecgrad_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return 4 * nq0 * nq1 * (dim == 3 ? nq2 : 1);
}

template <int DIM, typename T>
int launch_vecgrad_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s)
{
    // the classes of the Helmholtz fallback: 64 threads while four images fit the small class, else 256 threads and the
    // large one (3D 12^3 needs 6912 = kHelmLargeCap, 2D 32^2 4096)
    return launch_any_extent(vecgrad_generic_built(DIM, nq[0], nq[1], nq[2]),
                             vecgrad_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                             vecgrad_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                             vecgrad_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                             x.d1, x.d2, x.df, x.in0, x.in1, x.in2, x.grad, x.div, x.curl0, x.curl1, x.curl2, a.nelmt,
                             (int)nq[0], (int)nq[1], (int)nq[2]);
}
#define SF_VECGRAD_GENERIC(DIM, T)                                                                                     \
    template int launch_vecgrad_generic<DIM, T>(const unsigned (&)[3], const ArgsT<DIM, T> &, const VecgradArgsT<T> &, \
                                                hipStream_t);
SF_VECGRAD_GENERIC(3, double)
SF_VECGRAD_GENERIC(3, float)
SF_VECGRAD_GENERIC(2, double)
SF_VECGRAD_GENERIC(2, float)
#undef SF_VECGRAD_GENERIC

bool vecgrad_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2) &&
           vecgrad_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kHelmLargeCap;
}

} // namespace sf
