// helmholtz_generic.h -- the any-extent kernel body of the fused Helmholtz operator, shared by helmholtz_generic.hip (a
// metric per point) and affine_generic.hip (constants per element).  What the kernels do, their order of operations and
// their LDS images are described at the top of those two units; the body is that of helmholtz_generic.hip with the
// flux-and-mass step taken out into flux_points(), and its sweeps and derivative steps are the fragments frag/ae_*.inc
// (listed in any_extent.h), which mass_generic.hip, physderiv_generic.hip and iprodderiv_generic.hip include as well.
// flux_points() asks a policy MET:
//   MET::SCALED, MET::NCOMP   the fluxes and the mass term carry a factor q per point; metric components per point
//   element(e, nqt)           once per element
//   coef(x, nqt, gg)          the NCOMP coefficients of point x, in the order of the planes of g
//   scale(x, nq0, nq1)        q of point x (read only if SCALED)
//   mass(x, q, u)             the mass term of the point value u
#pragma once

#include "any_extent.h"

namespace sf
{

constexpr unsigned kHelmMax3D = 12, kHelmMax2D = 32;
constexpr int kHelmSmallCap = 2048, kHelmLargeCap = 4 * 12 * 12 * 12; // scalars; 2D 32^2 needs 3 * 1024

// fluxes in place (P1 .. P3), the mass term over u (P0): every thread touches its own points only
template <int DIM, int NT, class MET, typename T>
__device__ __forceinline__ void flux_points(const MET &met, int tid, int nq0, int nq1, int nqt, T *P0, T *P1, T *P2, T *P3)
{
    for (int x = tid; x < nqt; x += NT)
    {
        T gg[MET::NCOMP];
        met.coef(x, nqt, gg);
        const T q = met.scale(x, nq0, nq1);
        T f0, f1, f2 = T(0);
        if constexpr (DIM == 3)
        {
            const T x0 = P1[x], x1 = P2[x], x2 = P3[x];
            f0 = sfma(gg[2], x2, sfma(gg[1], x1, gg[0] * x0));
            f1 = sfma(gg[4], x2, sfma(gg[3], x1, gg[1] * x0));
            f2 = sfma(gg[5], x2, sfma(gg[4], x1, gg[2] * x0));
        }
        else
        {
            const T x0 = P1[x], x1 = P2[x];
            f0 = sfma(gg[1], x1, gg[0] * x0);
            f1 = sfma(gg[2], x1, gg[1] * x0);
        }
        if constexpr (MET::SCALED)
            f0 = q * f0, f1 = q * f1, f2 = q * f2;
        P1[x] = f0;
        P2[x] = f1;
        if constexpr (DIM == 3)
            P3[x] = f2;
        P0[x] = met.mass(x, q, P0[x]);
    }
}

// the whole operator on the elements of this workgroup; lds: the images, 4 (2D: 3) nq0 nq1 nq2 scalars
template <typename T, int DIM, int NT, class MET>
__device__ __forceinline__ void helm_generic_body(T *lds, const T *b0, const T *b1, const T *b2, const T *d0, const T *d1,
                                                  const T *d2, MET &met, const T *in, T *out, uint64_t nelmt, int nq0,
                                                  int nq1, int nq2)
{
#include "frag/ae_prologue.inc"
    T *P0 = lds, *P1 = lds + nqt, *P2 = lds + 2 * nqt, *P3 = lds + (DIM == 3 ? 3 : 2) * nqt;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        T *dst       = out + e * (uint64_t)nmt;
        met.element(e, nqt);
        if constexpr (DIM == 2)
        {
#define AE_MODES P1
#define AE_W1 P2
#define AE_POINTS P0
#define AE_POINT_VALUE(s) s
#include "frag/ae_forward_2d.inc"
            // du_a = D_a u, to P1 ..
            for (int x = tid; x < nqt; x += NT)
            {
#define AE_DU0 P1[x]
#define AE_DU1 P2[x]
#include "frag/ae_deriv_2d.inc"
            }
            __syncthreads();
            // fluxes in place, the mass term over u (every thread touches its own points only)
            flux_points<DIM, NT>(met, tid, nq0, nq1, nqt, P0, P1, P2, P3);
            __syncthreads();
            // v = ((lambda w) u + D_0^T f_0) + D_1^T f_1, over the mass term
            for (int x = tid; x < nqt; x += NT)
            {
#include "frag/ae_deriv_transposed_2d.inc"
                P0[x] = (P0[x] + t0) + t1;
            }
            __syncthreads();
#define AE_POINTS P0
#define AE_T1 P1
#include "frag/ae_transposed_2d.inc"
        }
        else
        {
#define AE_MODES P1
#define AE_W1 P0
#define AE_W2 P1
#define AE_POINTS P0
#define AE_POINT_VALUE(s) s
#include "frag/ae_forward_3d.inc"
            // du_a = D_a u, to P1 ..
            for (int x = tid; x < nqt; x += NT)
            {
#define AE_DU0 P1[x]
#define AE_DU1 P2[x]
#define AE_DU2 P3[x]
#include "frag/ae_deriv_3d.inc"
            }
            __syncthreads();
            // fluxes in place, the mass term over u (every thread touches its own points only)
            flux_points<DIM, NT>(met, tid, nq0, nq1, nqt, P0, P1, P2, P3);
            __syncthreads();
            // v = (((lambda w) u + D_0^T f_0) + D_1^T f_1) + D_2^T f_2, over the mass term
            for (int x = tid; x < nqt; x += NT)
            {
#include "frag/ae_deriv_transposed_3d.inc"
                P0[x] = ((P0[x] + t0) + t1) + t2;
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

// scalars of LDS the extents need: one point image per region
inline unsigned helm_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return dim == 3 ? 4 * nq0 * nq1 * nq2 : 3 * nq0 * nq1;
}

// within the extent bounds AND the images fit the large LDS class (true for every extent within the bounds: 3D 12^3
// needs 6912, 2D 32^2 3072; derived all the same, not assumed)
inline bool helm_extents_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kHelmMax3D : kHelmMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    return helm_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kHelmLargeCap;
}

} // namespace sf
