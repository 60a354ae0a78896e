// affine_wave.h -- the fused Helmholtz operator on affine elements as wave-per-chunk kernels for gfx950.
//
//   y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e
//   with  G_ab,e[k][j][i] = ge[e][ab] q2[k] q1[j] q0[i],   w_e[k][j][i] = je[e] q2[k] q1[j] q0[i]
//
// An affine element (parallelepiped, parallelogram) has a constant Jacobian: its metric is d(d+1)/2 constants ge[e][c]
// (c in the order of the planes of g: 3D 00, 01, 02, 11, 12, 22; 2D 00, 01, 11) and its mass weight one constant je[e],
// each times the tensor product of the one-dimensional quadrature weights qw_d, which all elements share.  The kernels
// are those of helmholtz_wave.h -- the same geometry (HelmGeom), front, pencil sweeps, images and back -- with the
// metric stream taken out: per element they move 2 nm^d + d(d+1)/2 + 1 scalars.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k                                   (u, the point values)
//   2. du_a = D_a u for a = 0, 1 [, 2]
//   3. q = qw2[k] (qw1[j] qw0[i])  (2D: qw1[j] qw0[i]);   f_a = q (sum_b ge_ab du_b), b ascending
//   4. v = (((lambda je_e) q) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]         (lambda == 0: the first term is 0)
//   5. transposed sweeps k -> r', j -> q', i -> p'
//
// Per-element constants.  Right after the chunk is staged, where the Helmholtz kernels request the first slices of their
// metric ring, lane (e, j, i) loads the NCOMP constants (and je) of the element of each of its point columns: NCOMP + 1
// values per pass that stay in registers over the walk, instead of the ring's 2 (NCOMP + 1).  The element index is
// clamped to the chunk's last valid element, as the ring's offsets are: nothing is read outside ge or je.  With one
// element per chunk (EC == 1) the index is the constant 0, the address is the same in every lane and the compiler takes
// the loads through the scalar path: the constants then live in SGPRs.
// Weights.  The lane-constant product qw1[j] qw0[i] (2D: qw0[i]) is formed once per wave, before the chunk loop; the
// weight of the walk direction, qw2[k] (2D: qw1[j]), is indexed by the unrolled walk counter, the same in every lane.
// Walk.  The image traffic of the Helmholtz walk and scalar loads only: qw2[k] (2D: qw1[j]) is read in the walk with a
// compile-time index from a const __restrict__ pointer, which hipcc turns into s_loads hoisted out of the chunk loop.
// No vector load, so no vmcnt wait and no scheduling barrier per slice -- by the compiler's choice, not by the source.
// HASJ = false (lambda == 0) compiles the load of je out: je is never dereferenced and may be null.
//
// Twin code.  The front (forward sweeps), the back (transposed sweeps and flush) and the derivative sweeps of the two
// kernels below are copies of hex_helmholtz_wave_kernel / quad_helmholtz_wave_kernel in helmholtz_wave.h; only the
// constant load and the walk body differ.  A fix to one of them belongs in both headers.
#pragma once

#include "helmholtz_wave.h"

namespace sf
{

// ge / je of the elements of this lane's point columns; e is in [0, evalid) for every lane
template <int NPASS, int NCOMP, int EC, bool HASJ, typename T>
__device__ __forceinline__ void load_element_constants(T (&gv)[NPASS][NCOMP], T (&lj)[NPASS], const T *__restrict__ ge,
                                                       const T *__restrict__ je, T lam, uint64_t first,
                                                       const int (&ecol)[NPASS], int evalid)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int e      = EC == 1 ? 0 : (ecol[s] < evalid ? ecol[s] : evalid - 1);
        const uint64_t g = first + (uint64_t)e;
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
            gv[s][c] = ge[g * NCOMP + c];
        if constexpr (HASJ)
            lj[s] = lam * je[g];
        else
            lj[s] = T(0);
    }
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASJ, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_affine_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ ge, const T *__restrict__ je, T lam, const T *__restrict__ in,
    T *__restrict__ out, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NM2 = NM * NM, NQ2 = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab;          // u, then du_1, f_1, D_1^T f_1
    T *imgD        = slab + G::IMG; // du_0, f_0, D_0^T f_0

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    // the three roles of a lane per pass: column (e,j,i) walking k, pencil (e,k,j) over i, pencil (e,k,i) over j
    bool own[NPASS];
    int colo[NPASS], ecol[NPASS], bi[NPASS], bj[NPASS];
    T qji[NPASS]; // qw1[j] qw0[i] of the column
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ2, ab = tc - e * NQ2, a = ab / NQ, b = ab - a * NQ;
        ecol[s] = e;
        colo[s] = e * ES + a * NQP + b; // (e,j,i): offset of the column's k = 0 point in an image
        bi[s]   = tc * NQP;             // (e,k,j): its i-pencil
        bj[s]   = e * ES + a * PL + b;  // (e,k,i): its j-pencil, stride NQP
        qji[s]  = qw1[a] * qw0[b];
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
        // the constants of this chunk's elements, requested once the staging registers are consumed
        T gv[NPASS][G::NCOMP], lj[NPASS];
        load_element_constants<NPASS, G::NCOMP, EC, HASJ>(gv, lj, ge, je, lam, c * (uint64_t)EC, ecol, evalid);
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
            T u[NPASS][NQ], f2[NPASS][NQ], acc[NPASS][NM];
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
            contract_dot<NQ, NQ, NPASS, BMODE>(u, f2, d2);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, true>(imgU, imgU, bj, own, d1);
            // ---- the walk over k: fluxes f_a = q sum_b ge_ab du_b, mass term ((lambda je) q) u ------
            {
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
                    const T qk = qw2[k];
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        const T(&gg)[G::NCOMP] = gv[s];
                        const T q  = qk * qji[s];
                        const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = f2[s][k];
                        const T f0 = q * fma_t(gg[2], x2, fma_t(gg[1], x1, gg[0] * x0));
                        const T f1 = q * fma_t(gg[4], x2, fma_t(gg[3], x1, gg[1] * x0));
                        f2[s][k]   = q * fma_t(gg[5], x2, fma_t(gg[4], x1, gg[2] * x0));
                        u[s][k]    = HASJ ? (lj[s] * q) * u[s][k] : T(0);
                        if (own[s])
                        {
                            imgD[colo[s] + k * PL] = f0;
                            imgU[colo[s] + k * PL] = f1;
                        }
                    }
                }
            }
            wave_lds_fence();
            // D_2^T f_2 in registers, D_0^T f_0 and D_1^T f_1 in place in the images
            T t2[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(f2, t2, d2);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgD, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, false>(imgU, imgU, bj, own, d1);
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int k = 0; k < NQ; ++k)
                    u[s][k] = ((u[s][k] + imgD[colo[s] + k * PL]) + imgU[colo[s] + k * PL]) + t2[s][k];
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
            wave_lds_fence(); // slab is rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASJ, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_affine_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ qw0, const T *__restrict__ qw1, const T *__restrict__ ge, const T *__restrict__ je, T lam,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP;
    constexpr int NPASS = G::NPASS, NP = G::NP;
    constexpr int ES = NQ * NQP; // element stride of the point image
    static_assert(KMAP > 0, "short-lived waves only");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
    T *imgU        = slab; // u, then du_0, f_0, D_0^T f_0

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    // the two roles of a lane per pass: column (e,i) walking j, pencil (e,j) over i
    bool own[NPASS];
    int colo[NPASS], ecol[NPASS], bi[NPASS];
    T qi[NPASS]; // qw0[i] of the column
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ, b = tc - e * NQ;
        ecol[s] = e;
        colo[s] = e * ES + b; // (e,i): offset of the column's j = 0 point in the image, stride NQP
        bi[s]   = tc * NQP;   // (e,j): its i-pencil
        qi[s]   = qw0[b];
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
        T gv[NPASS][G::NCOMP], lj[NPASS];
        load_element_constants<NPASS, G::NCOMP, EC, HASJ>(gv, lj, ge, je, lam, c * (uint64_t)EC, ecol, evalid);
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
            T u[NPASS][NQ], f1[NPASS][NQ], acc[NPASS][NM];
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
            contract_dot<NQ, NQ, NPASS, BMODE>(u, f1, d1);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgU, bi, own, d0);
            // ---- the walk over j ----------------------------------------------------------------------
            {
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
                    const T qj = qw1[j];
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        const T(&gg)[G::NCOMP] = gv[s];
                        const T q  = qj * qi[s];
                        const T x0 = a0[j % 2][s], x1 = f1[s][j];
                        const T f0 = q * fma_t(gg[1], x1, gg[0] * x0);
                        f1[s][j]   = q * fma_t(gg[2], x1, gg[1] * x0);
                        u[s][j]    = HASJ ? (lj[s] * q) * u[s][j] : T(0);
                        if (own[s])
                            imgU[colo[s] + j * NQP] = f0;
                    }
                }
            }
            wave_lds_fence();
            T t1[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(f1, t1, d1);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgU, imgU, bi, own, d0);
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    u[s][j] = (u[s][j] + imgU[colo[s] + j * NQP]) + t1[s][j];
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
