// physderiv_wave.h -- BwdTrans fused with the physical-space gradient as wave-per-chunk kernels for gfx950.
//
//   u = B x_e,   du_b = D_b u,   out_a[e] = sum_b df[e][a*d + b] du_b       (a = 0 .. d-1, b ascending)
//
// B the tensor-product BwdTrans basis, D_b the collocation derivative matrix of direction b (row-major nq x nq,
// (D_b u)[i] = sum_m deriv_b[i*nq + m] u[m]), df the inverse Jacobian d xi_b / d x_a per point, stored as d*d component
// planes df[e][c][k][j][i], c = a*d + b (not symmetric: 9 planes in 3D, 4 in 2D), each plane laid out like the output of
// BwdTrans.  d output streams out_a[e][k][j][i] in that layout; no point image reaches HBM.  This is the front half of
// the Helmholtz kernels (helmholtz_wave.h: chunk_fetch / chunk_stage, the forward sweeps, the derivative steps and a
// per-point walk over a ring of planes) with a d x d matrix-vector product in the walk and stores in the place of the
// transposed back half.  HelmGeom, image_sweep and the pencil helpers are those of helmholtz_wave.h; the front is the
// same text, csrc/frag/*.inc, in the sequence helmholtz_wave.h lists up to point_values (dreg holds du_2; 2D: du_1).
// This header's own: the df ring and the walk with its stores.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k                                   (u, the point values)
//   2. du_a = D_a u for a = 0, 1 [, 2]
//   3. out_a = sum_b df_ab du_b, b ascending                                   (HASDF == false: out_a = du_a)
//
// 3D.  After the last forward sweep lane (e, j, i) holds the k-pencil u[k] of its point column in registers.  du_2 is a
//   register contraction, u goes to LDS as point image U, lanes (e, k, j) write du_0 into a second image, lanes (e, k, i)
//   overwrite U with du_1.  Lane (e, j, i) then walks k: it reads du_0 and du_1 of the next slice from the images, takes
//   the nine planes of the slice from the ring and stores the three results of its point.
// 2D.  Lane (e, i) holds the j-pencil, du_1 is a register contraction, du_0 one in-place sweep of lanes (e, j) over ONE
//   image; the walk over j takes four planes and stores two results.
//
// df stream.  As the metric stream of helmholtz_wave.h: consecutive lanes read consecutive scalars of every plane,
// non-temporal, through a ring of kHelmRing slices (2 x 9 values per lane and pass in 3D), the first slices requested
// right after the chunk is staged.  The loads are unconditional: lanes without a point column and lanes whose element
// lies beyond the batch read the address of the chunk's last valid column (in bounds, the same lines).  Nothing is read
// outside df.  HASDF = false compiles the loads out: df is never dereferenced and may be null, the kernel returns the
// reference-space derivatives.
//
// Output.  Lane (e, j, i) stores its results of slice k itself: consecutive lanes write consecutive scalars of
// out_a[e][k][.][.], the mirror image of the df loads, and the planes of a column follow one another, so every line is
// completed in L2 by the same wave within one walk.  Plain stores (partial-line non-temporal stores cost 40-90 % in the
// experiments of DESIGN s4.4).  Lanes without a point column and elements beyond the batch store nothing.
#pragma once

#include "helmholtz_wave.h"

namespace sf
{

// one slice n of the d*d planes of this lane's point columns; src offsets are in bounds for every lane
template <int NPASS, int NCOMP, int PLANE, int NQT, typename T>
__device__ __forceinline__ void load_df_slice(T (&dv)[NPASS][NCOMP], const T *__restrict__ dc, const int (&doff)[NPASS],
                                              int n)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
            dv[s][c] = __builtin_nontemporal_load(dc + doff[s] + c * NQT + n * PLANE);
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_physderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ in,
    T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING, NCOMP = 9;
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
        // the df ring: the first slices, requested once the staging registers are consumed
        const T *dc = HASDF ? df + c * (uint64_t)(EC * NCOMP * NQT) : nullptr;
        int doff[NPASS], ooff[NPASS];
        bool put[NPASS]; // this lane stores: it has a point column and the column's element is in the batch
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            doff[s]     = e * (NCOMP * NQT) + colp[s];
            ooff[s]     = e * NQT + colp[s];
            put[s]      = own[s] && ecol[s] < evalid;
        }
        T dv[RING][NPASS][NCOMP];
        (void)dv, (void)dc, (void)doff; // unused without df
        if constexpr (HASDF)
        {
#pragma unroll
            for (int r = 0; r < RING; ++r)
                load_df_slice<NPASS, NCOMP, NQ2, NQT>(dv[r], dc, doff, r);
        }
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
#include "frag/forward1_3d.inc"
        // ---- forward 2 and everything at the points: lane (e,j,i) keeps its k-pencil in registers ---
        {
            T u[NPASS][NQ], dreg[NPASS][NQ];
#include "frag/point_values_3d.inc"
            // ---- the walk over k: out_a = sum_b df_ab du_b, stored by the column's lane -------------
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
                    const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = dreg[s][k];
                    T r0 = x0, r1 = x1, r2 = x2;
                    if constexpr (HASDF)
                    {
                        const T(&dd)[NCOMP] = dv[k % RING][s];
                        r0 = fma_t(dd[2], x2, fma_t(dd[1], x1, dd[0] * x0));
                        r1 = fma_t(dd[5], x2, fma_t(dd[4], x1, dd[3] * x0));
                        r2 = fma_t(dd[8], x2, fma_t(dd[7], x1, dd[6] * x0));
                    }
                    if (put[s])
                    {
                        o0[ooff[s] + k * NQ2] = r0;
                        o1[ooff[s] + k * NQ2] = r1;
                        o2[ooff[s] + k * NQ2] = r2;
                    }
                }
                if constexpr (HASDF)
                {
                    if (k + RING < NQ)
                        load_df_slice<NPASS, NCOMP, NQ2, NQT>(dv[k % RING], dc, doff, k + RING);
                }
                __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a slice
            }
            wave_lds_fence(); // the images are rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_physderiv_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ df, const T *__restrict__ in, T *__restrict__ out0, T *__restrict__ out1, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING, NCOMP = 4;
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
        // the df ring, as in the 3D kernel
        const T *dc = HASDF ? df + c * (uint64_t)(EC * NCOMP * NQT) : nullptr;
        int doff[NPASS], ooff[NPASS];
        bool put[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            doff[s]     = e * (NCOMP * NQT) + colp[s];
            ooff[s]     = e * NQT + colp[s];
            put[s]      = own[s] && ecol[s] < evalid;
        }
        T dv[RING][NPASS][NCOMP];
        (void)dv, (void)dc, (void)doff; // unused without df
        if constexpr (HASDF)
        {
#pragma unroll
            for (int r = 0; r < RING; ++r)
                load_df_slice<NPASS, NCOMP, NQ, NQT>(dv[r], dc, doff, r);
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
                    const T x0 = a0[j % 2][s], x1 = dreg[s][j];
                    T r0 = x0, r1 = x1;
                    if constexpr (HASDF)
                    {
                        const T(&dd)[NCOMP] = dv[j % RING][s];
                        r0 = fma_t(dd[1], x1, dd[0] * x0);
                        r1 = fma_t(dd[3], x1, dd[2] * x0);
                    }
                    if (put[s])
                    {
                        o0[ooff[s] + j * NQ] = r0;
                        o1[ooff[s] + j * NQ] = r1;
                    }
                }
                if constexpr (HASDF)
                {
                    if (j + RING < NQ)
                        load_df_slice<NPASS, NCOMP, NQ, NQT>(dv[j % RING], dc, doff, j + RING);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence(); // the image is rewritten by the next chunk's staging
        }
    }
}

} // namespace sf
