// affine_deriv_wave.h -- the gradient (physderiv_wave.h) and the weak divergence (iprodderiv_wave.h) on affine elements
// as wave-per-chunk kernels for gfx950.
//
//   gradient:         u = B x_e,  du_b = D_b u,  out_a[e][k][j][i] = sum_b dfe[e][a*d + b] du_b[e][k][j][i]
//   weak divergence:  t_b = sum_a dfe[e][a*d + b] in_a,  g_b = (je[e] q) t_b,  out_e = sum_b B^T D_b^T g_b
//                     with q = qw2[k] (qw1[j] qw0[i])  (2D: qw1[j] qw0[i])
//
// An affine element (parallelepiped, parallelogram) has a constant Jacobian: the d*d planes df of sf_physderiv_* /
// sf_iprodderiv_* hold the same d*d numbers at every point, dfe[e][c], c = a*d + b for d xi_b / d x_a (the order of the
// planes; not symmetric), and the weight plane of sf_iprodderiv_* is je[e] times the tensor product of the
// one-dimensional quadrature weights qw_d, which all elements share.  The kernels are those of physderiv_wave.h and
// iprodderiv_wave.h -- the same geometry (HelmGeom), fragments (csrc/frag/*.inc, in the sequence those headers list),
// images, walks and stores -- with the df ring (and the w part of the ring) taken out: per element the gradient moves
// nm^d + d nq^d + d*d scalars, the weak divergence d nq^d + nm^d + d*d + 1.
//
// Order of operations.  That of physderiv_wave.h / iprodderiv_wave.h with df_ab replaced by the element's constant and
// w by (je_e q): every sum in ascending index, the first product a multiply, then FMAs.  On a route the results are
// therefore bit for bit those of the deformed kernels on planes filled with the constants (the weight plane expanded
// as je * (qw2 * (qw1 * qw0))).
//   gradient:         1. forward sweeps  2. du_a = D_a u  3. out_a = sum_b dfe_ab du_b, b ascending
//   weak divergence:  1. t_b = sum_a dfe_ab in_a, a ascending  2. g_b = (je_e q) t_b   (HASW == false: g_b = t_b)
//                     3. v = (D_0^T g_0 + D_1^T g_1) [+ D_2^T g_2]  4. transposed sweeps k -> r, j -> q, i -> p
//
// Per-element constants.  load_element_constants of affine_wave.h, right after the chunk is staged (the weak divergence
// has no staging: at the head of the chunk, with the first slices of the input ring): lane (e, j, i) loads the d*d
// constants (and je) of the element of each of its point columns, d*d (+ 1) values per pass that stay in registers
// over the walk where the deformed kernels hold a ring of 2 d*d (+ 2).  The element index is clamped to the chunk's
// last valid element: nothing is read outside dfe or je.  With one element per chunk (EC == 1) the index is the
// constant 0, the address is the same in every lane and the loads go through the scalar path.
// Weights (weak divergence, HASW).  The lane-constant product qw1[j] qw0[i] (2D: qw0[i]) is formed once per wave, before
// the chunk loop; qw2[k] (2D: qw1[j]) is read with the unrolled walk counter, the same in every lane.  HASW = false
// compiles every load of je and qw_d out: they are never dereferenced and may be null.
// Scheduling barrier.  The gradient walk has no vector load left (images from LDS, constants in registers, plain
// stores), so there is no ring to keep a ring and the per-slice sched_barrier of physderiv_wave.h is dropped, as in the
// walk of affine_wave.h: the order of LDS reads and stores is the compiler's.  The weak divergence keeps its input ring
// and with it the barrier of iprodderiv_wave.h, one per slice.
//
// Input streams of the weak divergence: as iprodderiv_wave.h (non-temporal, one scalar per lane, a ring of
// kIprodDerivRing slices, unconditional loads at clamped offsets).  Outputs of the gradient: as physderiv_wave.h (plain
// stores by the column's lane; lanes without a point column and elements beyond the batch store nothing).
#pragma once

#include "affine_wave.h"
#include "iprodderiv_wave.h"

namespace sf
{

// one slice n of the d inputs of this lane's point columns; offsets in bounds for every lane
template <int NPASS, int DIM, int PLANE, typename T>
__device__ __forceinline__ void load_in_slice(T (&fv)[NPASS][DIM], const T *const (&fc)[DIM], const int (&foff)[NPASS],
                                              int n)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
#pragma unroll
        for (int a = 0; a < DIM; ++a)
            fv[s][a] = __builtin_nontemporal_load(fc[a] + foff[s] + n * PLANE);
}

// ------------------------------------------------------------------------------------------------
// gradient, 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_affine_physderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ dfe, const T *__restrict__ in,
    T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, NCOMP = 9;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab;          // u, then du_1
    T *imgD = slab + G::IMG; // du_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_3d.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // the constants of this chunk's elements, requested once the staging registers are consumed
        T dv[NPASS][NCOMP], lj[NPASS];
        load_element_constants<NPASS, NCOMP, EC, false>(dv, lj, dfe, (const T *)nullptr, T(0), c * (uint64_t)EC, ecol,
                                                        evalid);
        (void)lj;
        int ooff[NPASS];
        bool put[NPASS]; // this lane stores: it has a point column and the column's element is in the batch
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            ooff[s]     = e * NQT + colp[s];
            put[s]      = own[s] && ecol[s] < evalid;
        }
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
#include "frag/forward1_3d.inc"
        // ---- forward 2 and everything at the points: lane (e,j,i) keeps its k-pencil in registers ---
        {
            T u[NPASS][NQ], dreg[NPASS][NQ];
#include "frag/point_values_3d.inc"
            // ---- the walk over k: out_a = sum_b dfe_ab du_b, stored by the column's lane ------------
            T *o0 = out0 + c * (uint64_t)(EC * NQT), *o1 = out1 + c * (uint64_t)(EC * NQT),
              *o2 = out2 + c * (uint64_t)(EC * NQT);
            T a0[2][NPASS], a1[2][NPASS];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                a0[0][s] = imgD[colo[s]];
                a1[0][s] = imgU[colo[s]];
            }
#pragma unroll
            for (int k = 0; k < NQ; ++k)
            {
                if (k + 1 < NQ)
                {
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        a0[(k + 1) % 2][s] = imgD[colo[s] + (k + 1) * PL];
                        a1[(k + 1) % 2][s] = imgU[colo[s] + (k + 1) * PL];
                    }
                }
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T(&dd)[NCOMP] = dv[s];
                    const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = dreg[s][k];
                    const T r0 = fma_t(dd[2], x2, fma_t(dd[1], x1, dd[0] * x0));
                    const T r1 = fma_t(dd[5], x2, fma_t(dd[4], x1, dd[3] * x0));
                    const T r2 = fma_t(dd[8], x2, fma_t(dd[7], x1, dd[6] * x0));
                    if (put[s])
                    {
                        o0[ooff[s] + k * NQ2] = r0;
                        o1[ooff[s] + k * NQ2] = r1;
                        o2[ooff[s] + k * NQ2] = r2;
                    }
                }
            }
            wave_lds_fence(); // the images are rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// gradient, 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_affine_physderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ dfe, const T *__restrict__ in, T *__restrict__ out0, T *__restrict__ out1, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, NCOMP = 4;
    constexpr int ES = NQ * NQP; // element stride of the point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab; // u, then du_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_2d.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // the constants of this chunk's elements, as in the 3D kernel
        T dv[NPASS][NCOMP], lj[NPASS];
        load_element_constants<NPASS, NCOMP, EC, false>(dv, lj, dfe, (const T *)nullptr, T(0), c * (uint64_t)EC, ecol,
                                                        evalid);
        (void)lj;
        int ooff[NPASS];
        bool put[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            ooff[s]     = e * NQT + colp[s];
            put[s]      = own[s] && ecol[s] < evalid;
        }
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
        // ---- forward 1 and everything at the points: lane (e,i) keeps its j-pencil in registers -----
        {
            T u[NPASS][NQ], dreg[NPASS][NQ];
#include "frag/point_values_2d.inc"
            // ---- the walk over j ----------------------------------------------------------------------
            T *o0 = out0 + c * (uint64_t)(EC * NQT), *o1 = out1 + c * (uint64_t)(EC * NQT);
            T a0[2][NPASS];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
                a0[0][s] = imgU[colo[s]];
#pragma unroll
            for (int j = 0; j < NQ; ++j)
            {
                if (j + 1 < NQ)
                {
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                        a0[(j + 1) % 2][s] = imgU[colo[s] + (j + 1) * NQP];
                }
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T(&dd)[NCOMP] = dv[s];
                    const T x0 = a0[j % 2][s], x1 = dreg[s][j];
                    const T r0 = fma_t(dd[1], x1, dd[0] * x0);
                    const T r1 = fma_t(dd[3], x1, dd[2] * x0);
                    if (put[s])
                    {
                        o0[ooff[s] + j * NQ] = r0;
                        o1[ooff[s] + j * NQ] = r1;
                    }
                }
            }
            wave_lds_fence(); // the image is rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// weak divergence, 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_affine_iprodderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ dfe, const T *__restrict__ je, const T *__restrict__ in0,
    const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, NCOMP = 9;
    constexpr int RING = NQ < kIprodDerivRing ? NQ : kIprodDerivRing;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab;          // g_1, then D_1^T g_1
    T *imgD = slab + G::IMG; // g_0, then D_0^T g_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_3d.inc"
    T qji[NPASS]; // qw1[j] qw0[i] of the column
    (void)qji;    // unused without the weight
    if constexpr (HASW)
    {
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
            qji[s] = qw1[colp[s] / NQ] * qw0[colp[s] % NQ];
    }

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"

        // the ring: the inputs of the first slices; the constants of this chunk's elements (lj = je_e)
        const T *const fc[3] = {in0 + c * (uint64_t)(EC * NQT), in1 + c * (uint64_t)(EC * NQT),
                                in2 + c * (uint64_t)(EC * NQT)};
        int foff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            foff[s]     = e * NQT + colp[s];
        }
        T fv[RING][NPASS][3];
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_in_slice<NPASS, 3, NQ2>(fv[r], fc, foff, r);
        T dv[NPASS][NCOMP], lj[NPASS];
        load_element_constants<NPASS, NCOMP, EC, HASW>(dv, lj, dfe, je, T(1), c * (uint64_t)EC, ecol, evalid);

        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
            // ---- the walk over k: t_b = sum_a dfe_ab f_a, g_b = (je q) t_b ---------------------------
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
                    const T x0 = fv[k % RING][s][0], x1 = fv[k % RING][s][1], x2 = fv[k % RING][s][2];
                    T t0 = fma_t(dd[6], x2, fma_t(dd[3], x1, dd[0] * x0));
                    T t1 = fma_t(dd[7], x2, fma_t(dd[4], x1, dd[1] * x0));
                    T t2 = fma_t(dd[8], x2, fma_t(dd[5], x1, dd[2] * x0));
                    if constexpr (HASW)
                    {
                        const T ww = lj[s] * (qk * qji[s]);
                        t0 = ww * t0, t1 = ww * t1, t2 = ww * t2;
                    }
                    dreg[s][k] = t2; // g_2
                    if (own[s])
                    {
                        imgD[colo[s] + k * PL] = t0;
                        imgU[colo[s] + k * PL] = t1;
                    }
                }
                if (k + RING < NQ)
                    load_in_slice<NPASS, 3, NQ2>(fv[k % RING], fc, foff, k + RING);
                __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a slice
            }
#include "frag/deriv_transposed_3d.inc"
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int k = 0; k < NQ; ++k)
                    u[s][k] = (imgD[colo[s] + k * PL] + imgU[colo[s] + k * PL]) + t2[s][k];
#include "frag/transposed_last_3d.inc"
        }
#include "frag/transposed1_3d.inc"
#include "frag/transposed0.inc"
    }
}

// ------------------------------------------------------------------------------------------------
// weak divergence, 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_affine_iprodderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ qw0, const T *__restrict__ qw1, const T *__restrict__ dfe, const T *__restrict__ je,
    const T *__restrict__ in0, const T *__restrict__ in1, T *__restrict__ out, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, NCOMP = 4;
    constexpr int RING = NQ < kIprodDerivRing ? NQ : kIprodDerivRing;
    constexpr int ES = NQ * NQP; // element stride of the point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab; // g_0, then D_0^T g_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_2d.inc"
    T qi[NPASS]; // qw0[i] of the column
    (void)qi;    // unused without the weight
    if constexpr (HASW)
    {
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
            qi[s] = qw0[colp[s]];
    }

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"

        // the ring and the constants, as in the 3D kernel
        const T *const fc[2] = {in0 + c * (uint64_t)(EC * NQT), in1 + c * (uint64_t)(EC * NQT)};
        int foff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            foff[s]     = e * NQT + colp[s];
        }
        T fv[RING][NPASS][2];
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_in_slice<NPASS, 2, NQ>(fv[r], fc, foff, r);
        T dv[NPASS][NCOMP], lj[NPASS];
        load_element_constants<NPASS, NCOMP, EC, HASW>(dv, lj, dfe, je, T(1), c * (uint64_t)EC, ecol, evalid);

        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
            // ---- the walk over j ----------------------------------------------------------------------
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
                    const T x0 = fv[j % RING][s][0], x1 = fv[j % RING][s][1];
                    T t0 = fma_t(dd[2], x1, dd[0] * x0);
                    T t1 = fma_t(dd[3], x1, dd[1] * x0);
                    if constexpr (HASW)
                    {
                        const T ww = lj[s] * (qj * qi[s]);
                        t0 = ww * t0, t1 = ww * t1;
                    }
                    dreg[s][j] = t1; // g_1
                    if (own[s])
                        imgU[colo[s] + j * NQP] = t0;
                }
                if (j + RING < NQ)
                    load_in_slice<NPASS, 2, NQ>(fv[j % RING], fc, foff, j + RING);
                __builtin_amdgcn_sched_barrier(0);
            }
#include "frag/deriv_transposed_2d.inc"
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    u[s][j] = imgU[colo[s] + j * NQP] + t1[s][j];
#include "frag/transposed_last_2d.inc"
        }
#include "frag/transposed0.inc"
    }
}

} // namespace sf
