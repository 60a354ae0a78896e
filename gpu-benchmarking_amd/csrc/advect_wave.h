// advect_wave.h -- the weak advection term (c . grad) u tested against the basis, as wave-per-chunk kernels for gfx950.
//
//   u_a = B in_a,   J[a][b] = D_b u_a,   beta_b = sum_j c_j df[j*d + b],   r_a = w (sum_b beta_b J[a][b]),
//   out_a = B^T r_a                                                          (a = 0 .. NF-1, NF = 1 or d; b, j = 0 .. d-1)
//
// B the tensor-product BwdTrans basis, D_b the collocation derivative matrix of direction b, df the d*d planes of the
// inverse Jacobian (c = a*d + b for d xi_b / d x_a, the layout of physderiv_wave.h), w the weight plane of mass_wave.h,
// c_j the d planes of the advecting velocity at the points (each laid out like the output of BwdTrans), in_a / out_a the
// nm^d modes of field a of the element.  NF = 1 is scalar transport; NF = d advects a vector field and reads df, w and c
// once for all d fields.  No point image reaches HBM.
// The front is that of the gradient kernels, the same text, csrc/frag/*.inc: with NF = 1 the sequence physderiv_wave.h
// lists up to point_values over the slab of HelmGeom; with NF = d the unit of one coordinate of geom_wave.h,
// frag/geom_coordinate_{2d,3d}.inc, once per field with GEOM_X = in_a, over the slab of GeomGeom (the images of the fields
// 0 .. d-2 kept behind the front's slab).  Either way dk[a] is the register pencil d u_a / d xi_(d-1) of the column's lane.
// The back is that of the mass kernel, once per field out of dk[a]: frag/advect_field_back.inc strings
// transposed_last, transposed1 (3D) and transposed0 together.
// Shared text (csrc/frag/*.inc, the form mass_wave.h describes; affine_advect_wave.h includes the same files): wave_open;
// per chunk chunk_head, ring_offsets (the ring's clamped column offsets), then field_front_{2d,3d} (NF = 1) or
// fields_front_{2d,3d} (NF = d), either with the ring primed by ADV_PRIME where the front has its place for it; behind the
// walk advect_back (advect_field_back for every field).  This header's own: the ring of df, w, c and the arithmetic of
// the walk.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k of in_a                              (u_a, the point values)
//   2. J[a][b] = D_b u_a
//   3. beta_b = sum_j c_j df[j*d + b], j ascending                               (once per point, shared by the fields)
//   4. r_a = w * (sum_b beta_b J[a][b]), b ascending, then one multiply by w
//   5. transposed sweeps k -> r', j -> q', i -> p' of r_a
//
// The walk.  Lane (e, j, i) walks k (2D: lane (e, i) walks j).  Per slice it takes the d*d + d + 1 values of df, w, c of
// its point from a ring of kHelmRing slices, reads the image entries of J, forms beta and the r_a and writes r_a[k] over
// dk[a][s][k], which is dead once every r_a of the point is formed: no point image of r exists.  The loads of the ring
// are those of load_df_slice (physderiv_wave.h): non-temporal, unconditional, lanes without a point column and lanes
// whose element lies beyond the batch read the address of the chunk's last valid column (in bounds, the same lines), and
// what they compute never leaves the slab.  Nothing is read outside df, w or c_j; the three need only scalar alignment.
// With NF = d the first slices are requested in front of the last field's unit, in flight under its sweeps; with NF = 1
// right after the chunk is staged.
#pragma once

#include "geom_wave.h"
#include "physderiv_wave.h"

namespace sf
{

// the slab of the front: HelmGeom for one field, GeomGeom (with the kept images) for d fields
template <int NQ, int EC, int DIM, int NF, typename T>
using AdvectGeom = typename std::conditional<NF == 1, HelmGeom<NQ, EC, DIM, T>, GeomGeom<NQ, EC, DIM, T>>::type;

template <int NQ, int EC, int DIM, int NF, int WPB, typename T = double> constexpr size_t advect_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * AdvectGeom<NQ, EC, DIM, NF, T>::SLAB;
}

// one slice n of df (DD planes), w and c_0 .. c_(DIM-1) of this lane's point columns: av = df[0 .. DD-1], w, c_0 ..;
// src offsets are in bounds for every lane
template <int NPASS, int DIM, int PLANE, int NQT, typename T>
__device__ __forceinline__ void load_advect_slice(T (&av)[NPASS][DIM * DIM + DIM + 1], const T *__restrict__ dc,
                                                  const T *__restrict__ wc, const T *__restrict__ cc0,
                                                  const T *__restrict__ cc1, const T *__restrict__ cc2,
                                                  const int (&doff)[NPASS], const int (&woff)[NPASS], int n)
{
    constexpr int DD = DIM * DIM;
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
#pragma unroll
        for (int c = 0; c < DD; ++c)
            av[s][c] = __builtin_nontemporal_load(dc + doff[s] + c * NQT + n * PLANE);
        av[s][DD]     = __builtin_nontemporal_load(wc + woff[s] + n * PLANE);
        av[s][DD + 1] = __builtin_nontemporal_load(cc0 + woff[s] + n * PLANE);
        av[s][DD + 2] = __builtin_nontemporal_load(cc1 + woff[s] + n * PLANE);
        if constexpr (DIM == 3)
            av[s][DD + 3] = __builtin_nontemporal_load(cc2 + woff[s] + n * PLANE);
    }
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int NF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_advect_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ w,
    const T *__restrict__ c0, const T *__restrict__ c1, const T *__restrict__ c2, const T *__restrict__ x0,
    const T *__restrict__ x1, const T *__restrict__ x2, T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2,
    uint64_t nelmt)
{
    static_assert(NF == 1 || NF == 3, "one field or d");
    using G            = AdvectGeom<NQ, EC, 3, NF, T>;
    constexpr int RING = G::RING, NV = 13;
    // NF = d: the images of the fields 0 .. d-2 behind the front's slab; NF = 1: not used
#define OPEN_DIM 3
#define OPEN_KEPT_BASE (NF == 3 ? GeomGeom<NQ, EC, 3, T>::KEPT_BASE : 0)
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[3][NPASS][NQ]; // d u_a / d xi_2 over k, then r_a
        // the ring of df, w, c: every lane's offsets are in bounds
        const T *dc  = df + c * (uint64_t)(EC * 9 * NQT);
        const T *wc  = w + c * (uint64_t)(EC * NQT);
        const T *cc0 = c0 + c * (uint64_t)(EC * NQT), *cc1 = c1 + c * (uint64_t)(EC * NQT),
                *cc2 = c2 + c * (uint64_t)(EC * NQT);
#define RING_OFF doff[NPASS], woff[NPASS]
#define RING_SET doff[s] = e * (9 * NQT) + colp[s], woff[s] = e * NQT + colp[s];
#include "frag/ring_offsets.inc"
        T av[RING][NPASS][NV];
        // the first slices of the ring, requested by the front
#define ADV_PRIME                                                                                                      \
    _Pragma("unroll") for (int r = 0; r < RING; ++r)                                                                   \
        load_advect_slice<NPASS, 3, NQ2, NQT>(av[r], dc, wc, cc0, cc1, cc2, doff, woff, r);
        if constexpr (NF == 1)
        {
#define FRONT_PRIME ADV_PRIME
#include "frag/field_front_3d.inc"
        }
        else
        {
#define FRONT_PRIME ADV_PRIME
#include "frag/fields_front_3d.inc"
        }
#undef ADV_PRIME
        // ---- the walk over k: beta of the point, r_a over dk[a] ------------------------------------------
#pragma unroll
        for (int k = 0; k < NQ; ++k)
        {
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const T(&v)[NV] = av[k % RING][s];
                const int o     = colo[s] + k * PL;
                const T be0     = fma_t(v[12], v[6], fma_t(v[11], v[3], v[10] * v[0]));
                const T be1     = fma_t(v[12], v[7], fma_t(v[11], v[4], v[10] * v[1]));
                const T be2     = fma_t(v[12], v[8], fma_t(v[11], v[5], v[10] * v[2]));
                if constexpr (NF == 1)
                {
                    const T j0 = slab[G::IMG + o], j1 = slab[o];
                    dk[0][s][k] = v[9] * fma_t(be2, dk[0][s][k], fma_t(be1, j1, be0 * j0));
                }
                else
                {
                    const T j00 = kept[G::IMG + o], j01 = kept[o], j10 = kept[3 * G::IMG + o], j11 = kept[2 * G::IMG + o],
                            j20 = slab[G::IMG + o], j21 = slab[o];
                    dk[0][s][k] = v[9] * fma_t(be2, dk[0][s][k], fma_t(be1, j01, be0 * j00));
                    dk[1][s][k] = v[9] * fma_t(be2, dk[1][s][k], fma_t(be1, j11, be0 * j10));
                    dk[2][s][k] = v[9] * fma_t(be2, dk[2][s][k], fma_t(be1, j21, be0 * j20));
                }
            }
            if (k + RING < NQ)
                load_advect_slice<NPASS, 3, NQ2, NQT>(av[k % RING], dc, wc, cc0, cc1, cc2, doff, woff, k + RING);
            __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a slice
        }
        wave_lds_fence(); // the images are read: the back takes the slab
        // ---- the back, once per field: out_a = B^T r_a out of dk[a] --------------------------------------
#define ADV_BACK_DIM 3
#include "frag/advect_back.inc"
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int NF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_advect_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ df, const T *__restrict__ w, const T *__restrict__ c0, const T *__restrict__ c1,
    const T *__restrict__ x0, const T *__restrict__ x1, T *__restrict__ out0, T *__restrict__ out1, uint64_t nelmt)
{
    static_assert(NF == 1 || NF == 2, "one field or d");
    using G            = AdvectGeom<NQ, EC, 2, NF, T>;
    constexpr int RING = G::RING, NV = 7;
    // NF = d: the images of the fields 0 .. d-2 behind the front's slab; NF = 1: not used
#define OPEN_DIM 2
#define OPEN_KEPT_BASE (NF == 2 ? GeomGeom<NQ, EC, 2, T>::KEPT_BASE : 0)
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[2][NPASS][NQ]; // d u_a / d xi_1 over j, then r_a
        // the ring of df, w, c, as in the 3D kernel
        const T *dc  = df + c * (uint64_t)(EC * 4 * NQT);
        const T *wc  = w + c * (uint64_t)(EC * NQT);
        const T *cc0 = c0 + c * (uint64_t)(EC * NQT), *cc1 = c1 + c * (uint64_t)(EC * NQT);
#define RING_OFF doff[NPASS], woff[NPASS]
#define RING_SET doff[s] = e * (4 * NQT) + colp[s], woff[s] = e * NQT + colp[s];
#include "frag/ring_offsets.inc"
        T av[RING][NPASS][NV];
#define ADV_PRIME                                                                                                      \
    _Pragma("unroll") for (int r = 0; r < RING; ++r)                                                                   \
        load_advect_slice<NPASS, 2, NQ, NQT>(av[r], dc, wc, cc0, cc1, (const T *)nullptr, doff, woff, r);
        if constexpr (NF == 1)
        {
#define FRONT_PRIME ADV_PRIME
#include "frag/field_front_2d.inc"
        }
        else
        {
#define FRONT_PRIME ADV_PRIME
#include "frag/fields_front_2d.inc"
        }
#undef ADV_PRIME
        // ---- the walk over j ---------------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < NQ; ++j)
        {
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const T(&v)[NV] = av[j % RING][s];
                const int o     = colo[s] + j * NQP;
                const T be0     = fma_t(v[6], v[2], v[5] * v[0]);
                const T be1     = fma_t(v[6], v[3], v[5] * v[1]);
                if constexpr (NF == 1)
                {
                    const T j0  = slab[o];
                    dk[0][s][j] = v[4] * fma_t(be1, dk[0][s][j], be0 * j0);
                }
                else
                {
                    const T j00 = kept[o], j10 = slab[o];
                    dk[0][s][j] = v[4] * fma_t(be1, dk[0][s][j], be0 * j00);
                    dk[1][s][j] = v[4] * fma_t(be1, dk[1][s][j], be0 * j10);
                }
            }
            if (j + RING < NQ)
                load_advect_slice<NPASS, 2, NQ, NQT>(av[j % RING], dc, wc, cc0, cc1, (const T *)nullptr, doff, woff,
                                                     j + RING);
            __builtin_amdgcn_sched_barrier(0);
        }
        wave_lds_fence(); // the images are read: the back takes the slab
        // ---- the back, once per field --------------------------------------------------------------------
#define ADV_BACK_DIM 2
#include "frag/advect_back.inc"
    }
}

} // namespace sf
