// mass_generic.hip -- the fused mass operator B^T diag(w) B for any extents: the fallback of the wave kernels of
// mass_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index.  Sweep order of the wave kernels: forward p -> i, q -> j, r -> k, one
// multiply by the weight per point, then transposed k -> r', j -> q', i -> p'.  The images ping-pong between two LDS
// regions A and B:
//   3D: in (B) -> w1 (A) -> w2 (B) -> weighted points (A) -> t1 (B) -> t2 (A) -> out (HBM)
//   2D: in (A) -> w1 (B) -> weighted points (A) -> t1 (B) -> out (HBM)
// The sweeps are the fragments frag/ae_forward_*.inc and frag/ae_transposed_*.inc, which the Helmholtz body shares; the
// multiply by the weight is the value that the last forward sweep stores.
// A holds nq0*nq1[*nq2] scalars (the point image is the largest it sees), B nq0*nq1*nm2 in 3D and nq0*nm1 in 2D; the
// launcher derives both from the extents and refuses what does not fit the large class.  `in`, `w` and the bases are
// read from global memory with scalar loads, `out` is written with scalar stores: buffers that are only 8-byte
// (fp32: 4-byte) aligned are fine.  No workspace: every launch is a single kernel node, capture-safe from the first
// call.  Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 16 per
// direction in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "any_extent.h"

namespace sf
{

// LDS classes in scalars (those of iproduct_generic.hip).  3D 16^3: 4096 + 3840 = 7936; 2D 32^2: 1024 + 992.
constexpr int kMassSmallCap = 2048, kMassLargeCap = 7936;
constexpr unsigned kMassMax3D = 16, kMassMax2D = 32;

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void mass_generic_kernel(const T *__restrict__ b0, const T *__restrict__ b1,
                                                          const T *__restrict__ b2, const T *__restrict__ w,
                                                          const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt,
                                                          int nq0, int nq1, int nq2, int sizeA)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    T *A = lds, *B = lds + sizeA;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        const T *wt  = w + e * (uint64_t)nqt;
        T *dst       = out + e * (uint64_t)nmt;
        if constexpr (DIM == 2)
        {
#define AE_MODES A
#define AE_W1 B
#define AE_POINTS A
#define AE_POINT_VALUE(s) s * wt[x] // the weight: v = w u
#include "frag/ae_forward_2d.inc"
#define AE_POINTS A
#define AE_T1 B
#include "frag/ae_transposed_2d.inc"
        }
        else
        {
#define AE_MODES B
#define AE_W1 A
#define AE_W2 B
#define AE_POINTS A
#define AE_POINT_VALUE(s) s * wt[x] // the weight: v = w u
#include "frag/ae_forward_3d.inc"
#define AE_POINTS A
#define AE_T1 B
#define AE_T2 A
#include "frag/ae_transposed_3d.inc"
        }
        __syncthreads(); // the next element overwrites the images
    }
}

// region sizes in scalars: A the point image, B the larger of the images that alternate with it
static void mass_regions(int dim, unsigned nq0, unsigned nq1, unsigned nq2, unsigned &sizeA, unsigned &sizeB)
{
    if (dim == 3)
    {
        sizeA = nq0 * nq1 * nq2;       // >= w1 (nq0 nm1 nm2), t2 (nq0 nm1 nm2)
        sizeB = nq0 * nq1 * (nq2 - 1); // >= in (nm0 nm1 nm2); w2 and t1 have exactly this size
    }
    else
    {
        sizeA = nq0 * nq1;       // >= in (nm0 nm1)
        sizeB = nq0 * (nq1 - 1); // w1 and t1
    }
}

template <int DIM, typename T>
int launch_mass_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const T *w, hipStream_t s)
{
    unsigned sizeA, sizeB;
    mass_regions(DIM, nq[0], nq[1], nq[2], sizeA, sizeB);
    return launch_any_extent(mass_generic_built(DIM, nq[0], nq[1], nq[2]), sizeA + sizeB <= (unsigned)kMassSmallCap,
                             mass_generic_kernel<T, DIM, kMassSmallCap, 64>,
                             mass_generic_kernel<T, DIM, kMassLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), w, a.in,
                             a.out, a.nelmt, (int)nq[0], (int)nq[1], (int)nq[2], (int)sizeA);
}
template int launch_mass_generic<3, double>(const unsigned (&)[3], const HexArgs &, const double *, hipStream_t);
template int launch_mass_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const float *, hipStream_t);
template int launch_mass_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const double *, hipStream_t);
template int launch_mass_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const float *, hipStream_t);

// within the extent bounds AND the two regions fit the large LDS class (true for every extent within the bounds:
// 3D 16^3 needs 4096 + 3840, 2D 32^2 1024 + 992; derived all the same, not assumed)
bool mass_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kMassMax3D : kMassMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    unsigned sizeA, sizeB;
    mass_regions(dim, nq0, nq1, dim == 3 ? nq2 : 0, sizeA, sizeB);
    return sizeA + sizeB <= (unsigned)kMassLargeCap;
}

} // namespace sf
