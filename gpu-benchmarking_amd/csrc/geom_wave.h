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
// d*d + d(d+1)/2 + 2 planes.  No point image reaches HBM but the outputs.  This header's own: the kept images, the walk
// and its stores; the unit of one coordinate with its prefetch is frag/geom_coordinate_{2d,3d}.inc, included d times.
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
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    constexpr bool Q = (MASK & (kGeomW | kGeomG)) != 0;
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *kept = slab + G::KEPT_BASE; // d X_0 / d xi_1, d X_0 / d xi_0, d X_1 / d xi_1, d X_1 / d xi_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_3d.inc"
    const T *in = x0; // the stream the fragments fetch and stage: the coordinate at hand
#include "frag/chunk_fetch_first.inc"

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
#define GEOM_A 0
#define GEOM_X x0
#define GEOM_NEXT x1
#include "frag/geom_coordinate_3d.inc"
#define GEOM_A 1
#define GEOM_X x1
#define GEOM_NEXT x2
#include "frag/geom_coordinate_3d.inc"
#define GEOM_A 2
#define GEOM_X x2
#define GEOM_NEXT x0
#include "frag/geom_coordinate_3d.inc"
        // ---- the walk over k: J of the point, its factors, its stores -------------------------------
        {
            const uint64_t e0 = c * (uint64_t)EC;
            bool put[NPASS]; // this lane stores: it has a point column and the column's element is in the batch
            int ooff[NPASS];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                put[s]  = own[s] && ecol[s] < evalid;
                ooff[s] = ecol[s] * NQT + colp[s];
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
            {
                T qk = T(0);
                if constexpr (Q)
                    qk = has_q ? qw2[k] : T(0);
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const int o = colo[s] + k * PL;
                    const T J[3][3] = {{kept[G::IMG + o], kept[o], dk[0][s][k]},
                                       {kept[3 * G::IMG + o], kept[2 * G::IMG + o], dk[1][s][k]},
                                       {slab[G::IMG + o], slab[o], dk[2][s][k]}};
                    GeomPoint<3, T> p;
                    geom_point<3, MASK, true>(J, qk * q01[s], p);
                    if (put[s])
                    {
                        const int oo = ooff[s] + k * NQ2;
                        if constexpr ((MASK & kGeomDf) != 0)
                            if (df)
                            {
                                T *dst = df + e0 * (9 * NQT) + ecol[s] * (8 * NQT) + oo;
#pragma unroll
                                for (int cc = 0; cc < 9; ++cc)
                                    dst[cc * NQT] = p.df[cc];
                            }
                        if constexpr ((MASK & kGeomW) != 0)
                            if (w)
                                w[e0 * NQT + oo] = p.w;
                        if constexpr ((MASK & kGeomG) != 0)
                            if (g)
                            {
                                T *dst = g + e0 * (6 * NQT) + ecol[s] * (5 * NQT) + oo;
#pragma unroll
                                for (int cc = 0; cc < 6; ++cc)
                                    dst[cc * NQT] = p.g[cc];
                            }
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
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP;
    constexpr int ES = NQ * NQP; // element stride of the point image
    constexpr bool Q = (MASK & (kGeomW | kGeomG)) != 0;
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *kept = slab + G::KEPT_BASE; // d X_0 / d xi_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_2d.inc"
    const T *in = x0; // the stream the fragments fetch and stage: the coordinate at hand
#include "frag/chunk_fetch_first.inc"

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
#define GEOM_A 0
#define GEOM_X x0
#include "frag/geom_coordinate_2d.inc"
#define GEOM_A 1
#define GEOM_X x1
#include "frag/geom_coordinate_2d.inc"
        // ---- the walk over j ----------------------------------------------------------------------
        {
            const uint64_t e0 = c * (uint64_t)EC;
            bool put[NPASS];
            int ooff[NPASS];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                put[s]  = own[s] && ecol[s] < evalid;
                ooff[s] = ecol[s] * NQT + colp[s];
            }
#pragma unroll
            for (int j = 0; j < NQ; ++j)
            {
                T qj = T(0);
                if constexpr (Q)
                    qj = has_q ? qw1[j] : T(0);
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const int o     = colo[s] + j * NQP;
                    const T J[2][2] = {{kept[o], dk[0][s][j]}, {slab[o], dk[1][s][j]}};
                    GeomPoint<2, T> p;
                    geom_point<2, MASK, true>(J, qj * q0[s], p);
                    if (put[s])
                    {
                        const int oo = ooff[s] + j * NQ;
                        if constexpr ((MASK & kGeomDf) != 0)
                            if (df)
                            {
                                T *dst = df + e0 * (4 * NQT) + ecol[s] * (3 * NQT) + oo;
#pragma unroll
                                for (int cc = 0; cc < 4; ++cc)
                                    dst[cc * NQT] = p.df[cc];
                            }
                        if constexpr ((MASK & kGeomW) != 0)
                            if (w)
                                w[e0 * NQT + oo] = p.w;
                        if constexpr ((MASK & kGeomG) != 0)
                            if (g)
                            {
                                T *dst = g + e0 * (3 * NQT) + ecol[s] * (2 * NQT) + oo;
#pragma unroll
                                for (int cc = 0; cc < 3; ++cc)
                                    dst[cc * NQT] = p.g[cc];
                            }
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
