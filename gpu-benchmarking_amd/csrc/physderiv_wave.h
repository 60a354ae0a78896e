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
// transposed back half.  HelmGeom, image_sweep and the pencil helpers are those of helmholtz_wave.h.
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
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NM2 = NM * NM, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING, NCOMP = 9;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab;          // u, then du_1
    T *imgD        = slab + G::IMG; // du_0

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
        colp[s] = ab;                   // (j,i): offset inside a plane of df / out_a
        colo[s] = e * ES + a * NQP + b; // (e,j,i): offset of the column's k = 0 point in an image
        bi[s]   = tc * NQP;             // (e,k,j): its i-pencil
        bj[s]   = e * ES + a * PL + b;  // (e,k,i): its j-pencil, stride NQP
    }

    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

        chunk_stage<IO, AL>(st, slab, lane,
                            IO::VEC2 ? (AL ? align_shift(in + c * IO::IN_DBL) : 0) : line_offset<T>(in + c * IO::IN_DBL));
        wave_lds_fence();
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
        if (n + 1 < it.count)
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, c + it.step, nelmt, lane);

        // ---- forward 0: w1[(e,i,r)][q] = sum_p in[(e,r,q)][p] * B0[p][i] ---------------------------
        {
            T u[F::PASS0][NM], acc[F::PASS0][NQ];
            read_pencils<NM, F::PASS0, F::P0, F::IN_STRIDE>(u, slab, lane);
            contract<NM, NQ, F::PASS0, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < F::PASS0; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= F::P0 || t < F::P0)
                {
                    const int e = t / NM2, rq = t - e * NM2, r = rq / NM, q = rq - r * NM;
                    T *dst = slab + (e * NQ * NM + r) * NMP + q;
#pragma unroll
                    for (int i = 0; i < NQ; ++i)
                        dst[i * NM * NMP] = acc[s][i];
                }
            }
            wave_lds_fence();
        }
        // ---- forward 1: w2[(e,j,i)][r] = sum_q w1[(e,i,r)][q] * B1[q][j] ---------------------------
        {
            T u[F::PASS1][NM], acc[F::PASS1][NQ];
            read_pencils<NM, F::PASS1, F::P1, NMP>(u, slab, lane);
            contract<NM, NQ, F::PASS1, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < F::PASS1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= F::P1 || t < F::P1)
                {
                    const int e = t / (NQ * NM), ir = t - e * (NQ * NM), i = ir / NM, r = ir - i * NM;
                    T *dst = slab + (e * NQ2 + i) * NMP + r;
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        dst[j * NQ * NMP] = acc[s][j];
                }
            }
            wave_lds_fence();
        }
        // ---- forward 2 and everything at the points: lane (e,j,i) keeps its k-pencil in registers ---
        {
            T u[NPASS][NQ], du2[NPASS][NQ];
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b2);
            }
            wave_lds_fence(); // the forward images are dead: the point images take their place
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
                if (own[s])
                {
#pragma unroll
                    for (int k = 0; k < NQ; ++k)
                        imgU[colo[s] + k * PL] = u[s][k];
                }
            wave_lds_fence();
            // du_2[k] = sum_m D2[k][m] u[m] in registers; du_0 into imgD; du_1 over u in imgU
            contract_dot<NQ, NQ, NPASS, BMODE>(u, du2, d2);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, true>(imgU, imgU, bj, own, d1);
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
                    const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = du2[s][k];
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

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab; // u, then du_0

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
        colp[s] = b;          // i: offset inside a row of df / out_a
        colo[s] = e * ES + b; // (e,i): offset of the column's j = 0 point in the image, stride NQP
        bi[s]   = tc * NQP;   // (e,j): its i-pencil
    }

    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

        chunk_stage<IO, AL>(st, slab, lane,
                            IO::VEC2 ? (AL ? align_shift(in + c * IO::IN_DBL) : 0) : line_offset<T>(in + c * IO::IN_DBL));
        wave_lds_fence();
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
        if (n + 1 < it.count)
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, c + it.step, nelmt, lane);

        // ---- forward 0: w1[(e,i)][q] = sum_p in[(e,q)][p] * B0[p][i] -------------------------------
        {
            T u[F::PASS0][NM], acc[F::PASS0][NQ];
            read_pencils<NM, F::PASS0, F::P0, F::IN_STRIDE>(u, slab, lane);
            contract<NM, NQ, F::PASS0, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < F::PASS0; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= F::P0 || t < F::P0)
                {
                    const int e = t / NM, q = t - e * NM;
                    T *dst = slab + e * NQ * NMP + q;
#pragma unroll
                    for (int i = 0; i < NQ; ++i)
                        dst[i * NMP] = acc[s][i];
                }
            }
            wave_lds_fence();
        }
        // ---- forward 1 and everything at the points: lane (e,i) keeps its j-pencil in registers -----
        {
            T u[NPASS][NQ], du1[NPASS][NQ];
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b1);
            }
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
                if (own[s])
                {
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        imgU[colo[s] + j * NQP] = u[s][j];
                }
            wave_lds_fence();
            // du_1[j] = sum_m D1[j][m] u[m] in registers; du_0 over u in the image
            contract_dot<NQ, NQ, NPASS, BMODE>(u, du1, d1);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgU, bi, own, d0);
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
                    const T x0 = a0[j % 2][s], x1 = du1[s][j];
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
