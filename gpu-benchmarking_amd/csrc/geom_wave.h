// geom_wave.h -- the geometric factors of isoparametric elements from their modal coordinates, as wave-per-chunk kernels
// for gfx950.
//
//   X_a = B x_a,   J[a][b] = D_b X_a,   df = J^-1 laid out by c = a*d + b for d xi_b / d x_a,   detj = det J,
//   w = |det J| q,   G_ab = w sum_x df[x*d + a] df[x*d + b]                                   (a, b = 0 .. d-1)
//
// B the tensor-product BwdTrans basis, D_b the collocation derivative matrix of direction b, x_a the nm^d modes of
// coordinate a of the element (the layout of `in` everywhere), q the product of the one-dimensional quadrature weights.
// The front half of the gradient kernels (physderiv_wave.h: chunk_fetch / chunk_stage, the forward sweeps, the
// derivative steps -- the same text, csrc/frag/*.inc, up to point_values) runs d times per chunk, once per coordinate;
// the walk over the point columns then gathers the d x d entries of J, inverts (geom_point.h) and stores up to
// d*d + d(d+1)/2 + 2 planes.  No point image reaches HBM but the outputs.
// Shared text (csrc/frag/*.inc, the form mass_wave.h describes; vecgrad_wave.h, advect_wave.h and affine_advect_wave.h
// include the same files).  Each kernel is, in order: wave_open (the names of the geometry, the slab and its kept
// images, the chunks, the lane roles, the first request); per chunk chunk_head, fields_front_{2d,3d} (the unit of one
// coordinate with its prefetch, geom_coordinate_{2d,3d}, once per coordinate); in the walk walk_stores (the store mask and
// the output offsets), point_jacobian_{2d,3d} (J of the point out of the images and dk) and planes_store (df, g).  This
// header's own: the slab with the kept images (GeomGeom), the weight products, the arithmetic of the point and which
// planes it stores.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k of x_a                              (X_a, the point values)
//   2. J[a][b] = D_b X_a
//   3.-7. cofactors, determinant, reciprocal, df, w, G: geom_point.h
//
// The unit of work is (chunk, coordinate a).  The staging registers are refilled right after they are consumed, with the
// next coordinate's modes of the same chunk or, behind the last coordinate, with x_0 of the wave's next chunk: one
// stream of modes is always in flight under the sweeps.
// 3D.  Per coordinate point_values leaves d X_a / d xi_0 and d X_a / d xi_1 as two LDS point images and d X_a / d xi_2
//   as the k-pencil of lane (e, j, i) in registers.  The images of coordinates 0 and 1 are kept behind the front's slab
//   (four images); those of the last coordinate stay where the gradient kernels have them, over the dead forward
//   intermediates: six images and 3 NQ NPASS registers.  Lane (e, j, i) then walks k: six LDS reads, three registers,
//   the arithmetic of the point, its stores.
// 2D.  One image per coordinate (d X_a / d xi_0), the j-pencil d X_a / d xi_1 in registers; one kept image; lane (e, i)
//   walks j.
//
// Output.  Lane (e, j, i) stores its point of every requested plane: consecutive lanes write consecutive scalars of a
// plane, the planes of a column follow one another.  Plain stores (DESIGN s4.4).  Lanes without a point column and
// elements beyond the batch store nothing.  MASK names the outputs an instantiation can write (geom_point.h: kGeomDf,
// kGeomW, kGeomG, kGeomDet); the arithmetic of the others is not generated.  Every store of an instantiation is behind a
// wave-uniform null check of its pointer, so a request that is routed to a superset writes the requested planes only.
// qw_d are read only when w or g is written (they may be null otherwise).
#pragma once

#include "geom_point.h"
#include "helmholtz_wave.h"

namespace sf
{

// the slab of HelmGeom (front half and the point images of the last coordinate) and the kept images behind it
template <int NQ, int EC, int DIM, typename T = double> struct GeomGeom : HelmGeom<NQ, EC, DIM, T>
{
    using H = HelmGeom<NQ, EC, DIM, T>;
    static constexpr int KEPT      = (DIM == 3) ? 4 : 1; // images of the coordinates 0 .. d-2
    static constexpr int KEPT_BASE = H::SLAB;
    static constexpr int SLAB      = (H::SLAB + KEPT * H::IMG + H::VW - 1) / H::VW * H::VW;
};

template <int NQ, int EC, int DIM, int WPB, typename T = double> constexpr size_t geom_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * GeomGeom<NQ, EC, DIM, T>::SLAB;
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int MASK, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_geom_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ x0, const T *__restrict__ x1, const T *__restrict__ x2,
    T *__restrict__ df, T *__restrict__ w, T *__restrict__ g, T *__restrict__ detj, uint64_t nelmt)
{
    using G          = GeomGeom<NQ, EC, 3, T>;
    constexpr bool Q = (MASK & (kGeomW | kGeomG)) != 0;
#define OPEN_DIM 3
#define OPEN_KEPT_BASE G::KEPT_BASE // d X_0 / d xi_1, d X_0 / d xi_0, d X_1 / d xi_1, d X_1 / d xi_0
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    // q01 = qw1[j] qw0[i] of this lane's columns
    T q01[NPASS];
    const bool has_q = Q && (w != nullptr || g != nullptr);
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int j = colp[s] / NQ, i = colp[s] - j * NQ;
        q01[s]      = has_q ? qw1[j] * qw0[i] : T(0);
    }

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[3][NPASS][NQ]; // d X_a / d xi_2 over k
#define FRONT_PRIME
#include "frag/fields_front_3d.inc"
        // ---- the walk over k: J of the point, its factors, its stores -------------------------------
        {
#include "frag/walk_stores.inc"
#pragma unroll
            for (int k = 0; k < NQ; ++k)
            {
                T qk = T(0);
                if constexpr (Q)
                    qk = has_q ? qw2[k] : T(0);
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
#include "frag/point_jacobian_3d.inc"
                    GeomPoint<3, T> p;
                    geom_point<3, MASK, true>(J, qk * q01[s], p);
                    if (put[s])
                    {
                        const int oo = ooff[s] + k * NQ2;
                        if constexpr ((MASK & kGeomDf) != 0)
                            if (df)
#define PLANES_DST df
#define PLANES_N 9
#define PLANES_VAL(cc) p.df[cc]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kGeomW) != 0)
                            if (w)
                                w[e0 * NQT + oo] = p.w;
                        if constexpr ((MASK & kGeomG) != 0)
                            if (g)
#define PLANES_DST g
#define PLANES_N 6
#define PLANES_VAL(cc) p.g[cc]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kGeomDet) != 0)
                            if (detj)
                                detj[e0 * NQT + oo] = p.det;
                    }
                }
            }
            wave_lds_fence(); // the images of the last coordinate are rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int MASK, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_geom_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ qw0, const T *__restrict__ qw1, const T *__restrict__ x0, const T *__restrict__ x1,
    T *__restrict__ df, T *__restrict__ w, T *__restrict__ g, T *__restrict__ detj, uint64_t nelmt)
{
    using G          = GeomGeom<NQ, EC, 2, T>;
    constexpr bool Q = (MASK & (kGeomW | kGeomG)) != 0;
#define OPEN_DIM 2
#define OPEN_KEPT_BASE G::KEPT_BASE // d X_0 / d xi_0
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    T q0[NPASS]; // qw0[i] of this lane's columns
    const bool has_q = Q && (w != nullptr || g != nullptr);
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
        q0[s] = has_q ? qw0[colp[s]] : T(0);

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[2][NPASS][NQ]; // d X_a / d xi_1 over j
#define FRONT_PRIME
#include "frag/fields_front_2d.inc"
        // ---- the walk over j ----------------------------------------------------------------------
        {
#include "frag/walk_stores.inc"
#pragma unroll
            for (int j = 0; j < NQ; ++j)
            {
                T qj = T(0);
                if constexpr (Q)
                    qj = has_q ? qw1[j] : T(0);
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
#include "frag/point_jacobian_2d.inc"
                    GeomPoint<2, T> p;
                    geom_point<2, MASK, true>(J, qj * q0[s], p);
                    if (put[s])
                    {
                        const int oo = ooff[s] + j * NQ;
                        if constexpr ((MASK & kGeomDf) != 0)
                            if (df)
#define PLANES_DST df
#define PLANES_N 4
#define PLANES_VAL(cc) p.df[cc]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kGeomW) != 0)
                            if (w)
                                w[e0 * NQT + oo] = p.w;
                        if constexpr ((MASK & kGeomG) != 0)
                            if (g)
#define PLANES_DST g
#define PLANES_N 3
#define PLANES_VAL(cc) p.g[cc]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kGeomDet) != 0)
                            if (detj)
                                detj[e0 * NQT + oo] = p.det;
                    }
                }
            }
            wave_lds_fence(); // the image of the last coordinate is rewritten by the next chunk's staging
        }
    }
}

} // namespace sf
