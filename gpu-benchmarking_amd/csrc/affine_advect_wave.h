// affine_advect_wave.h -- the weak advection term (advect_wave.h) on affine elements as wave-per-chunk kernels for gfx950.
//
//   u_a = B in_a,   J[a][b] = D_b u_a,   beta_b = sum_j c_j dfe[e][j*d + b],   r_a = (je[e] q) (sum_b beta_b J[a][b]),
//   out_a = B^T r_a        with q = qw2[k] (qw1[j] qw0[i])  (2D: qw1[j] qw0[i]);  a = 0 .. NF-1, NF = 1 or d
//
// An affine element (parallelepiped, parallelogram) has a constant Jacobian: the d*d planes df of sf_advect_* hold the
// same d*d numbers at every point, dfe[e][c], c = a*d + b for d xi_b / d x_a (the array of affine_deriv_wave.h; not
// symmetric), and the weight plane is je[e] times the tensor product of the one-dimensional quadrature weights qw_d,
// which all elements share.  The kernels are those of advect_wave.h -- the same slabs (AdvectGeom), the same fronts (NF =
// 1: the gradient front over HelmGeom; NF = d: frag/geom_coordinate_{2d,3d}.inc once per field over GeomGeom with the
// kept images), the same back (frag/advect_field_back.inc once per field), the fragments unchanged in text -- with the
// df and w part of the ring taken out: per element the call moves d nq^d + 2 NF nm^d + d*d + 1 scalars where the
// deformed one moves (d*d + d + 1) nq^d + 2 NF nm^d.
// Shared text (csrc/frag/*.inc, the sequence advect_wave.h lists): wave_open, ring_offsets, field_front_{2d,3d} or
// fields_front_{2d,3d} with AFF_PRIME (the ring primed, the constants loaded), advect_back.  This header's own: the ring of
// c, the constants, the weight products and the arithmetic of the walk.  The weight product of the column goes into
// wave_open as its OPEN_LANE_SETUP: formed behind the opening, after the first request, it changed 44 of the 89 kernels
// of affine_advect_f32.hip.
//
// Order of operations.  That of advect_wave.h with df_ab replaced by the element's constant and w by (je_e q), q formed
// as qw2 * (qw1 * qw0): every sum in ascending index, the first product a multiply, then FMAs.  On a route the results
// are therefore bit for bit those of the deformed kernels on planes filled with the constants (the weight plane expanded
// as je * (qw2 * (qw1 * qw0))); HASW = false: those with w a plane of ones.
//   1. forward sweeps p -> i, q -> j, r -> k of in_a
//   2. J[a][b] = D_b u_a
//   3. beta_b = sum_j c_j dfe[j*d + b], j ascending                              (once per point, shared by the fields)
//   4. r_a = (je_e q) * (sum_b beta_b J[a][b]), b ascending, then one multiply   (HASW == false: no multiply)
//   5. transposed sweeps k -> r', j -> q', i -> p' of r_a
//
// The walk.  Lane (e, j, i) walks k (2D: lane (e, i) walks j).  Per slice it takes the d values of c of its point from a
// ring of kHelmRing slices, reads the image entries of J, forms beta and the r_a and writes r_a[k] over dk[a][s][k], as
// advect_wave.h does.  The loads of the ring are the c part of load_advect_slice: non-temporal, unconditional, lanes
// without a point column and lanes whose element lies beyond the batch read the address of the chunk's last valid column
// (in bounds, the same lines), and what they compute never leaves the slab.  The ring is still a ring, so the per-slice
// sched_barrier of advect_wave.h stays.
// Per-element constants.  load_element_constants of affine_wave.h, once per chunk: with NF = 1 right after the chunk is
// staged, with NF = d in front of the last field's unit, where the first ring slices are requested too.  Lane (e, j, i)
// loads the d*d constants (and je) of the element of each of its point columns, d*d (+ 1) values per pass that stay in
// registers over the walk where the deformed kernels hold a ring of (d*d + 1) values more per slice.  The element index
// is clamped to the chunk's last valid element: nothing is read outside dfe or je.  With one element per chunk (EC == 1)
// the index is the constant 0, the address is the same in every lane and the loads go through the scalar path.
// Weights (HASW).  The lane-constant product qw1[j] qw0[i] (2D: qw0[i]) is formed once per wave, before the chunk loop;
// qw2[k] (2D: qw1[j]) is read with the unrolled walk counter, the same in every lane.  HASW = false compiles every load
// of je and qw_d out: they are never dereferenced and may be null.
// Nothing is read outside dfe, je, qw_d or c_j; all of them need only scalar alignment.
#pragma once

#include "advect_wave.h"
#include "affine_wave.h"

namespace sf
{

// one slice n of c_0 .. c_(DIM-1) of this lane's point columns; offsets in bounds for every lane
template <int NPASS, int DIM, int PLANE, typename T>
__device__ __forceinline__ void load_c_slice(T (&cv)[NPASS][DIM], const T *__restrict__ cc0, const T *__restrict__ cc1,
                                             const T *__restrict__ cc2, const int (&coff)[NPASS], int n)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        cv[s][0] = __builtin_nontemporal_load(cc0 + coff[s] + n * PLANE);
        cv[s][1] = __builtin_nontemporal_load(cc1 + coff[s] + n * PLANE);
        if constexpr (DIM == 3)
            cv[s][2] = __builtin_nontemporal_load(cc2 + coff[s] + n * PLANE);
    }
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int NF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_affine_advect_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ dfe, const T *__restrict__ je, const T *__restrict__ c0,
    const T *__restrict__ c1, const T *__restrict__ c2, const T *__restrict__ x0, const T *__restrict__ x1,
    const T *__restrict__ x2, T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt)
{
    static_assert(NF == 1 || NF == 3, "one field or d");
    using G            = AdvectGeom<NQ, EC, 3, NF, T>;
    constexpr int RING = G::RING, NCOMP = 9;
    // NF = d: the images of the fields 0 .. d-2 behind the front's slab; NF = 1: not used
#define OPEN_DIM 3
#define OPEN_KEPT_BASE (NF == 3 ? GeomGeom<NQ, EC, 3, T>::KEPT_BASE : 0)
    // qji = qw1[j] qw0[i] of the column; unused without the weight
#define OPEN_LANE_SETUP                                                                                                \
    T qji[NPASS];                                                                                                      \
    (void)qji;                                                                                                         \
    if constexpr (HASW)                                                                                                \
    {                                                                                                                  \
        _Pragma("unroll") for (int s = 0; s < NPASS; ++s) qji[s] = qw1[colp[s] / NQ] * qw0[colp[s] % NQ];              \
    }
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[3][NPASS][NQ]; // d u_a / d xi_2 over k, then r_a
        // the ring of c: every lane's offsets are in bounds
        const T *cc0 = c0 + c * (uint64_t)(EC * NQT), *cc1 = c1 + c * (uint64_t)(EC * NQT),
                *cc2 = c2 + c * (uint64_t)(EC * NQT);
#define RING_OFF coff[NPASS]
#define RING_SET coff[s] = e * NQT + colp[s];
#include "frag/ring_offsets.inc"
        T cv[RING][NPASS][3];
        T dv[NPASS][NCOMP], lj[NPASS]; // the constants of this chunk's elements (lj = je_e)
        // the first slices of the ring and the constants, requested by the front
#define AFF_PRIME                                                                                                      \
    _Pragma("unroll") for (int r = 0; r < RING; ++r) load_c_slice<NPASS, 3, NQ2>(cv[r], cc0, cc1, cc2, coff, r);       \
    load_element_constants<NPASS, NCOMP, EC, HASW>(dv, lj, dfe, je, T(1), c * (uint64_t)EC, ecol, evalid);
        if constexpr (NF == 1)
        {
#define FRONT_PRIME AFF_PRIME
#include "frag/field_front_3d.inc"
        }
        else
        {
#define FRONT_PRIME AFF_PRIME
#include "frag/fields_front_3d.inc"
        }
#undef AFF_PRIME
        // ---- the walk over k: beta of the point, r_a over dk[a] ------------------------------------------
#pragma unroll
        for (int k = 0; k < NQ; ++k)
        {
            T qk = T(0);
            if constexpr (HASW)
                qk = qw2[k];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const T(&dd)[NCOMP] = dv[s];
                const T(&v)[3]      = cv[k % RING][s];
                const int o         = colo[s] + k * PL;
                const T be0         = fma_t(v[2], dd[6], fma_t(v[1], dd[3], v[0] * dd[0]));
                const T be1         = fma_t(v[2], dd[7], fma_t(v[1], dd[4], v[0] * dd[1]));
                const T be2         = fma_t(v[2], dd[8], fma_t(v[1], dd[5], v[0] * dd[2]));
                T ww                = T(0);
                if constexpr (HASW)
                    ww = lj[s] * (qk * qji[s]);
                if constexpr (NF == 1)
                {
                    const T j0 = slab[G::IMG + o], j1 = slab[o];
                    T r0 = fma_t(be2, dk[0][s][k], fma_t(be1, j1, be0 * j0));
                    if constexpr (HASW)
                        r0 = ww * r0;
                    dk[0][s][k] = r0;
                }
                else
                {
                    const T j00 = kept[G::IMG + o], j01 = kept[o], j10 = kept[3 * G::IMG + o], j11 = kept[2 * G::IMG + o],
                            j20 = slab[G::IMG + o], j21 = slab[o];
                    T r0 = fma_t(be2, dk[0][s][k], fma_t(be1, j01, be0 * j00));
                    T r1 = fma_t(be2, dk[1][s][k], fma_t(be1, j11, be0 * j10));
                    T r2 = fma_t(be2, dk[2][s][k], fma_t(be1, j21, be0 * j20));
                    if constexpr (HASW)
                        r0 = ww * r0, r1 = ww * r1, r2 = ww * r2;
                    dk[0][s][k] = r0;
                    dk[1][s][k] = r1;
                    dk[2][s][k] = r2;
                }
            }
            if (k + RING < NQ)
                load_c_slice<NPASS, 3, NQ2>(cv[k % RING], cc0, cc1, cc2, coff, k + RING);
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
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int NF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_affine_advect_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ qw0, const T *__restrict__ qw1, const T *__restrict__ dfe, const T *__restrict__ je,
    const T *__restrict__ c0, const T *__restrict__ c1, const T *__restrict__ x0, const T *__restrict__ x1,
    T *__restrict__ out0, T *__restrict__ out1, uint64_t nelmt)
{
    static_assert(NF == 1 || NF == 2, "one field or d");
    using G            = AdvectGeom<NQ, EC, 2, NF, T>;
    constexpr int RING = G::RING, NCOMP = 4;
    // NF = d: the images of the fields 0 .. d-2 behind the front's slab; NF = 1: not used
#define OPEN_DIM 2
#define OPEN_KEPT_BASE (NF == 2 ? GeomGeom<NQ, EC, 2, T>::KEPT_BASE : 0)
    // qi = qw0[i] of the column; unused without the weight
#define OPEN_LANE_SETUP                                                                                                \
    T qi[NPASS];                                                                                                       \
    (void)qi;                                                                                                          \
    if constexpr (HASW)                                                                                                \
    {                                                                                                                  \
        _Pragma("unroll") for (int s = 0; s < NPASS; ++s) qi[s] = qw0[colp[s]];                                        \
    }
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[2][NPASS][NQ]; // d u_a / d xi_1 over j, then r_a
        // the ring of c and the constants, as in the 3D kernel
        const T *cc0 = c0 + c * (uint64_t)(EC * NQT), *cc1 = c1 + c * (uint64_t)(EC * NQT);
#define RING_OFF coff[NPASS]
#define RING_SET coff[s] = e * NQT + colp[s];
#include "frag/ring_offsets.inc"
        T cv[RING][NPASS][2];
        T dv[NPASS][NCOMP], lj[NPASS];
#define AFF_PRIME                                                                                                      \
    _Pragma("unroll") for (int r = 0; r < RING; ++r)                                                                   \
        load_c_slice<NPASS, 2, NQ>(cv[r], cc0, cc1, (const T *)nullptr, coff, r);                                      \
    load_element_constants<NPASS, NCOMP, EC, HASW>(dv, lj, dfe, je, T(1), c * (uint64_t)EC, ecol, evalid);
        if constexpr (NF == 1)
        {
#define FRONT_PRIME AFF_PRIME
#include "frag/field_front_2d.inc"
        }
        else
        {
#define FRONT_PRIME AFF_PRIME
#include "frag/fields_front_2d.inc"
        }
#undef AFF_PRIME
        // ---- the walk over j ---------------------------------------------------------------------------
#pragma unroll
        for (int j = 0; j < NQ; ++j)
        {
            T qj = T(0);
            if constexpr (HASW)
                qj = qw1[j];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const T(&dd)[NCOMP] = dv[s];
                const T(&v)[2]      = cv[j % RING][s];
                const int o         = colo[s] + j * NQP;
                const T be0         = fma_t(v[1], dd[2], v[0] * dd[0]);
                const T be1         = fma_t(v[1], dd[3], v[0] * dd[1]);
                T ww                = T(0);
                if constexpr (HASW)
                    ww = lj[s] * (qj * qi[s]);
                if constexpr (NF == 1)
                {
                    const T j0 = slab[o];
                    T r0       = fma_t(be1, dk[0][s][j], be0 * j0);
                    if constexpr (HASW)
                        r0 = ww * r0;
                    dk[0][s][j] = r0;
                }
                else
                {
                    const T j00 = kept[o], j10 = slab[o];
                    T r0 = fma_t(be1, dk[0][s][j], be0 * j00);
                    T r1 = fma_t(be1, dk[1][s][j], be0 * j10);
                    if constexpr (HASW)
                        r0 = ww * r0, r1 = ww * r1;
                    dk[0][s][j] = r0;
                    dk[1][s][j] = r1;
                }
            }
            if (j + RING < NQ)
                load_c_slice<NPASS, 2, NQ>(cv[j % RING], cc0, cc1, (const T *)nullptr, coff, j + RING);
            __builtin_amdgcn_sched_barrier(0);
        }
        wave_lds_fence(); // the images are read: the back takes the slab
        // ---- the back, once per field --------------------------------------------------------------------
#define ADV_BACK_DIM 2
#include "frag/advect_back.inc"
    }
}

} // namespace sf
