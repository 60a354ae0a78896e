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
// COPY NOTE.  This is a fourth copy of Helmholtz text (after helmholtz_wave.h itself, affine_wave.h and
// physderiv_wave.h): the lane roles, the walk over a ring of planes, and everything after the walk -- the transposed
// derivative steps, the three transposed sweeps and chunk_flush -- are the text of the back half of
// hex_helmholtz_wave_kernel / quad_helmholtz_wave_kernel.  A change to that back half has to be made here too.  The
// existing kernels were not refactored to share it: DESIGN s9 item 7 records why helpers changed their code.
// HelmGeom, image_sweep and the pencil helpers are those of helmholtz_wave.h.
//
// What is new: a kernel with NO front half (there are no modes to read: no chunk_fetch / chunk_stage, no forward
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

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab;          // g_1, then D_1^T g_1
    T *imgD        = slab + G::IMG; // g_0, then D_0^T g_0

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    // the three roles of a lane per pass: column (e,j,i) walking k, pencil (e,k,j) over i, pencil (e,k,i) over j
    bool own[NPASS];
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS], bj[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ2, ab = tc - e * NQ2, a = ab / NQ, b = ab - a * NQ;
        ecol[s] = e;
        colp[s] = ab;                   // (j,i): offset inside a plane of in_a / df / w
        colo[s] = e * ES + a * NQP + b; // (e,j,i): offset of the column's k = 0 point in an image
        bi[s]   = tc * NQP;             // (e,k,j): its i-pencil
        bj[s]   = e * ES + a * PL + b;  // (e,k,i): its j-pencil, stride NQP
    }

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

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
            T u[NPASS][NQ], g2[NPASS][NQ], acc[NPASS][NM];
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
                    g2[s][k] = t2;
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
            wave_lds_fence();
            // D_2^T g_2 in registers, D_0^T g_0 and D_1^T g_1 in place in the images
            T t2[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(g2, t2, d2);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgD, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, false>(imgU, imgU, bj, own, d1);
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int k = 0; k < NQ; ++k)
                    u[s][k] = (imgD[colo[s] + k * PL] + imgU[colo[s] + k * PL]) + t2[s][k];
            // ---- transposed 2: t2[(e,r',i)][j] = sum_k v[k] * B2[r'][k] ------------------------------
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b2);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ2, ji = t - e * NQ2, j = ji / NQ, i = ji - j * NQ;
                    T *dst = slab + (e * NM * NQ + i) * NQP + j;
#pragma unroll
                    for (int r = 0; r < NM; ++r)
                        dst[r * NQ * NQP] = acc[s][r];
                }
            }
            wave_lds_fence();
        }
        // ---- transposed 1: t1[(e,r',q')][i] = sum_j t2[(e,r',i)][j] * B1[q'][j] --------------------
        {
            T u[M::PASST2][NQ], acc[M::PASST2][NM];
            read_pencils<NQ, M::PASST2, M::PT2, NQP>(u, slab, lane);
            contract_dot<NQ, NM, M::PASST2, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < M::PASST2; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= M::PT2 || t < M::PT2)
                {
                    const int er = t / NQ, i = t - er * NQ; // er = e*NM + r'
                    T *dst = slab + er * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
        }
        // ---- transposed 0: out[e][r'][q'][p'] = sum_i t1[(e,r',q')][i] * B0[p'][i] -----------------
        {
            T u[M::PASST1][NQ], acc[M::PASST1][NM];
            read_pencils<NQ, M::PASST1, M::PT1, NQP>(u, slab, lane);
            contract_dot<NQ, NM, M::PASST1, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < M::PASST1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= M::PT1 || t < M::PT1)
                {
                    T *dst = slab + t * NM; // t = (e*NM + r')*NM + q'
#pragma unroll
                    for (int p = 0; p < NM; ++p)
                        dst[p] = acc[s][p];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)M::OUT_DBL, evalid * G::F::NMT, lane);
            wave_lds_fence(); // slab is rewritten by the next chunk's walk
        }
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

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab; // g_0, then D_0^T g_0

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    // the two roles of a lane per pass: column (e,i) walking j, pencil (e,j) over i
    bool own[NPASS];
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ, b = tc - e * NQ;
        ecol[s] = e;
        colp[s] = b;          // i: offset inside a row of in_a / df / w
        colo[s] = e * ES + b; // (e,i): offset of the column's j = 0 point in the image, stride NQP
        bi[s]   = tc * NQP;   // (e,j): its i-pencil
    }

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

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
            T u[NPASS][NQ], g1[NPASS][NQ], acc[NPASS][NM];
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
                    g1[s][j] = t1;
                    if (own[s])
                        imgU[colo[s] + j * NQP] = t0;
                }
                if (j + RING < NQ)
                    load_ipd_slice<NPASS, 2, NQ, NQT, HASDF, HASW>(fv[j % RING], dv[j % RING], wv[j % RING], fc, dc, wc,
                                                                   foff, doff, j + RING);
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence();
            T t1[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(g1, t1, d1);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgU, imgU, bi, own, d0);
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    u[s][j] = imgU[colo[s] + j * NQP] + t1[s][j];
            // ---- transposed 1: t1[(e,q')][i] = sum_j v[j] * B1[q'][j] --------------------------------
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ, i = t - e * NQ;
                    T *dst = slab + e * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
        }
        // ---- transposed 0: out[e][q'][p'] = sum_i t1[(e,q')][i] * B0[p'][i] ------------------------
        {
            T u[M::PASST1][NQ], acc[M::PASST1][NM];
            read_pencils<NQ, M::PASST1, M::PT1, NQP>(u, slab, lane);
            contract_dot<NQ, NM, M::PASST1, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < M::PASST1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= M::PT1 || t < M::PT1)
                {
                    T *dst = slab + t * NM; // t = e*NM + q'
#pragma unroll
                    for (int p = 0; p < NM; ++p)
                        dst[p] = acc[s][p];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)M::OUT_DBL, evalid * G::F::NMT, lane);
            wave_lds_fence();
        }
    }
}

} // namespace sf
