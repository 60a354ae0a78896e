// iprodderiv_wave.h -- IProductWRTDerivBase, the weak divergence and the exact transpose of the kernels of
// physderiv_wave.h, as wave-per-chunk kernels for gfx950.
//
//   g_b = w * sum_a df[e][a*d + b] f_a   (per point; b = 0 .. d-1, a ascending),     out_e = sum_b B^T D_b^T g_b
//
// B the tensor-product BwdTrans basis, D_b the collocation derivative matrix of direction b (row-major nq x nq,
// (D_b u)[i] = sum_m deriv_b[i*nq + m] u[m]), df the d*d planes of sf_physderiv_* (c = a*d + b for d xi_b / d x_a; the
// sum here runs over the ROW index a), w one plane per element as in sf_mass_*, f_a d separate point arrays in the
// BwdTrans output layout (what sf_physderiv_* writes), out nm^d modes per element (the layout of sf_iproduct_*).
//
// Shared text.  The lane roles and everything after the walk -- the transposed derivative steps, the three transposed
// sweeps and chunk_flush -- are the back half of the Helmholtz kernels, the same text: csrc/frag/*.inc, included in
// place (helmholtz_wave.h lists the sequence; here it is wave_slab, [imgU, imgD], wave_chunks, lane_roles | per chunk:
// chunk_head, [the ring and the walk], deriv_transposed, [the sum of step 3], transposed_last, transposed1 (3D),
// transposed0).  HelmGeom, image_sweep and the pencil helpers are those of helmholtz_wave.h.
//
// This header's own: a kernel with NO front half (there are no modes to read: no chunk_fetch / chunk_stage, no forward
// sweeps), d input streams, and a ring that carries the inputs as well as the metric.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. t_b = sum_a df_ab f_a, a ascending                                      (HASDF == false: t_b = f_b)
//   2. g_b = w * t_b                                                           (HASW == false: g_b = t_b)
//   3. v = (D_0^T g_0 + D_1^T g_1) [+ D_2^T g_2]
//   4. transposed sweeps k -> r, j -> q, i -> p
//
// 3D.  Lane (e, j, i) walks k.  Per slice it takes f_0, f_1, f_2, the nine planes of df and w of its point (13 values
//   per pass), forms g_0 -> image D, g_1 -> image U (only lanes with a point column write) and keeps g_2 in registers.
//   After the walk D_2^T g_2 is a register contraction (contract(): the summed index is the row of deriv2), D_0^T and
//   D_1^T two in-place pencil sweeps over the images, the column owner adds the three terms in the order of step 3 and
//   the transposed sweeps follow.
// 2D.  Lane (e, i) walks j (7 values per pass), g_1 stays in registers, g_0 goes into the ONE image.
//
// Input streams.  Consecutive lanes read consecutive scalars of every plane, non-temporal, one scalar per lane (scalar
// alignment is enough for every input), through a ring of kIprodDerivRing slices.  The loads are unconditional: lanes
// without a point column and lanes whose element lies beyond the batch read the address of the chunk's last valid column
// (in bounds, the same lines) and what they compute never leaves the slab.  Nothing is read outside any input.  One
// sched_barrier per slice keeps the ring a ring.  HASDF / HASW = false compile the loads out: df / w are never
// dereferenced and may be null.
//
// Cold start.  The wave has nothing to hide its first loads under (no forward sweeps), so the ring depth is a constant
// of this header rather than kHelmRing; DESIGN s4.14 holds what is known about depth 2 against 3.
#pragma once

#include "helmholtz_wave.h"

namespace sf
{

#ifndef SF_IPRODDERIV_RING
#define SF_IPRODDERIV_RING 2 // -DSF_IPRODDERIV_RING=3 builds the other depth of the comparison in DESIGN s4.14
#endif
constexpr int kIprodDerivRing = SF_IPRODDERIV_RING; // slices in flight per lane

// one slice n of the inputs, the d*d planes and the weight of this lane's point columns; offsets in bounds for every lane
template <int NPASS, int DIM, int PLANE, int NQT, bool HASDF, bool HASW, typename T>
__device__ __forceinline__ void load_ipd_slice(T (&fv)[NPASS][DIM], T (&dv)[NPASS][DIM * DIM], T (&wv)[NPASS],
                                               const T *const (&fc)[DIM], const T *__restrict__ dc,
                                               const T *__restrict__ wc, const int (&foff)[NPASS],
                                               const int (&doff)[NPASS], int n)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
#pragma unroll
        for (int a = 0; a < DIM; ++a)
            fv[s][a] = __builtin_nontemporal_load(fc[a] + foff[s] + n * PLANE);
        if constexpr (HASDF)
        {
#pragma unroll
            for (int c = 0; c < DIM * DIM; ++c)
                dv[s][c] = __builtin_nontemporal_load(dc + doff[s] + c * NQT + n * PLANE);
        }
        if constexpr (HASW)
            wv[s] = __builtin_nontemporal_load(wc + foff[s] + n * PLANE);
    }
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_iprodderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ w,
    const T *__restrict__ in0, const T *__restrict__ in1, const T *__restrict__ in2, T *__restrict__ out, uint64_t nelmt)
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

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"

        // the ring: inputs, df and w of the first slices
        const T *const fc[3] = {in0 + c * (uint64_t)(EC * NQT), in1 + c * (uint64_t)(EC * NQT),
                                in2 + c * (uint64_t)(EC * NQT)};
        const T *dc          = HASDF ? df + c * (uint64_t)(EC * NCOMP * NQT) : nullptr;
        const T *wc          = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int foff[NPASS], doff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            foff[s]     = e * NQT + colp[s];
            doff[s]     = e * (NCOMP * NQT) + colp[s];
        }
        T fv[RING][NPASS][3], dv[RING][NPASS][NCOMP], wv[RING][NPASS];
        (void)dv, (void)wv, (void)dc, (void)wc, (void)doff; // unused without df / w
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_ipd_slice<NPASS, 3, NQ2, NQT, HASDF, HASW>(fv[r], dv[r], wv[r], fc, dc, wc, foff, doff, r);

        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
            // ---- the walk over k: t_b = sum_a df_ab f_a, g_b = w t_b --------------------------------
#pragma unroll
            for (int k = 0; k < NQ; ++k)
            {
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T x0 = fv[k % RING][s][0], x1 = fv[k % RING][s][1], x2 = fv[k % RING][s][2];
                    T t0 = x0, t1 = x1, t2 = x2;
                    if constexpr (HASDF)
                    {
                        const T(&dd)[NCOMP] = dv[k % RING][s];
                        t0 = fma_t(dd[6], x2, fma_t(dd[3], x1, dd[0] * x0));
                        t1 = fma_t(dd[7], x2, fma_t(dd[4], x1, dd[1] * x0));
                        t2 = fma_t(dd[8], x2, fma_t(dd[5], x1, dd[2] * x0));
                    }
                    if constexpr (HASW)
                    {
                        const T ww = wv[k % RING][s];
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
                    load_ipd_slice<NPASS, 3, NQ2, NQT, HASDF, HASW>(fv[k % RING], dv[k % RING], wv[k % RING], fc, dc, wc,
                                                                    foff, doff, k + RING);
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
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_iprodderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ df, const T *__restrict__ w, const T *__restrict__ in0, const T *__restrict__ in1,
    T *__restrict__ out, uint64_t nelmt)
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

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"

        // the ring, as in the 3D kernel
        const T *const fc[2] = {in0 + c * (uint64_t)(EC * NQT), in1 + c * (uint64_t)(EC * NQT)};
        const T *dc          = HASDF ? df + c * (uint64_t)(EC * NCOMP * NQT) : nullptr;
        const T *wc          = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int foff[NPASS], doff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            foff[s]     = e * NQT + colp[s];
            doff[s]     = e * (NCOMP * NQT) + colp[s];
        }
        T fv[RING][NPASS][2], dv[RING][NPASS][NCOMP], wv[RING][NPASS];
        (void)dv, (void)wv, (void)dc, (void)wc, (void)doff; // unused without df / w
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_ipd_slice<NPASS, 2, NQ, NQT, HASDF, HASW>(fv[r], dv[r], wv[r], fc, dc, wc, foff, doff, r);

        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
            // ---- the walk over j ----------------------------------------------------------------------
#pragma unroll
            for (int j = 0; j < NQ; ++j)
            {
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T x0 = fv[j % RING][s][0], x1 = fv[j % RING][s][1];
                    T t0 = x0, t1 = x1;
                    if constexpr (HASDF)
                    {
                        const T(&dd)[NCOMP] = dv[j % RING][s];
                        t0 = fma_t(dd[2], x1, dd[0] * x0);
                        t1 = fma_t(dd[3], x1, dd[1] * x0);
                    }
                    if constexpr (HASW)
                    {
                        const T ww = wv[j % RING][s];
                        t0 = ww * t0, t1 = ww * t1;
                    }
                    dreg[s][j] = t1; // g_1
                    if (own[s])
                        imgU[colo[s] + j * NQP] = t0;
                }
                if (j + RING < NQ)
                    load_ipd_slice<NPASS, 2, NQ, NQT, HASDF, HASW>(fv[j % RING], dv[j % RING], wv[j % RING], fc, dc, wc,
                                                                   foff, doff, j + RING);
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
