// helmholtz_wave.h -- the fused Helmholtz operator as wave-per-chunk kernels for gfx950.
//
//   y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e
//
// B the tensor-product BwdTrans basis, D_a the collocation derivative matrix of direction a at the quadrature points
// (row-major nq x nq, (D_a u)[i] = sum_m deriv_a[i*nq + m] u[m]), G the symmetric metric tensor per point, stored as
// component planes g[e][c][k][j][i] (3D: c = 00, 01, 02, 11, 12, 22; 2D: c = 00, 01, 11), w the mass weight per point.
// BwdTrans, three (two) derivatives, the metric contraction, the transposed derivatives and IProductWRTBase in ONE
// kernel: the quadrature-space images never exist in HBM.  The front (chunk_fetch / chunk_stage, the forward sweeps) and
// the back (the transposed sweeps, chunk_flush) are those of the mass kernel (mass_wave.h); the middle is new.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k                                   (u, the point values)
//   2. du_a = D_a u for a = 0, 1 [, 2]
//   3. f_a = sum_b G_ab du_b, b ascending
//   4. v = ((lambda w) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]                 (lambda == 0: the first term is 0)
//   5. transposed sweeps k -> r', j -> q', i -> p'
//
// 3D.  After the last forward sweep lane (e, j, i) holds the k-pencil u[k] of its point column in registers.
//   du_2 is a register contraction (contract_dot with the rows of deriv2).  u is written to LDS as a point image U
//   (index ((e nq + k) nq + j) S + i, S = nq | 1 odd): lanes (e, k, j) own its i-pencils and write du_0 into a second
//   image, lanes (e, k, i) own its j-pencils and overwrite them with du_1 -- u itself stays in the registers of the
//   column owners.  Lane (e, j, i) then walks k: it takes the six metric planes and w of its point, du_0 and du_1 from
//   the images, writes f_0 and f_1 back over them, keeps f_2 and (lambda w) u in registers.  D_2^T f_2 is a register
//   contraction (contract(): the summed index is the row of deriv2); D_0^T and D_1^T are two more in-place pencil sweeps
//   over the flux images; the column owner adds the three terms in the order of step 4.  Two point images per chunk, which
//   reuse the space of the (dead) input and forward intermediates.
// 2D.  One direction fewer: lane (e, i) holds the j-pencil, du_1 / D_1^T f_1 are register contractions, du_0 / D_0^T f_0
//   in-place sweeps of lanes (e, j) over ONE point image.
//
// Metric stream.  Lane (e, j, i) reads g[e][c][k][j][i] and w[e][k][j][i]: consecutive lanes read consecutive scalars of
// every plane, every line is fetched from HBM once, non-temporal.  The loads run through a ring of kRing slices: the
// slices 0 .. kRing-1 are requested right after the chunk is staged (in flight under the forward sweeps), slice k + kRing
// when slice k has been consumed -- 7 kRing values per lane instead of 7 nq.  The loads are unconditional, so that the
// walk is straight-line code and every wait is counted (the ISA of 3D nq 8 fp64 waits with s_waitcnt vmcnt(14) .. (19)
// inside the walk, i.e. only for the oldest slice; behind conditional loads hipcc falls back to vmcnt(0), see the note
// in mass_wave.h -- the conditional form was not built here).  Lanes without a point column and lanes whose element
// lies beyond the batch read the address of the chunk's last valid column instead (in bounds, the same lines), and what
// they compute never leaves the slab.  Nothing is read outside g or w.  HASW = false (lambda == 0) compiles the w loads
// out: w is never dereferenced and may be null.
#pragma once

#include "mass_wave.h"

namespace sf
{

constexpr int kHelmRing = 2; // metric slices in flight per lane

template <int NQ, int EC, int DIM, typename T = double> struct HelmGeom
{
    using M      = MassGeom<NQ, EC, DIM, T>; // front and back half
    using F      = typename M::F;
    using Scalar = T;
    static constexpr int VW    = VecOf<T>::W;
    static constexpr int NM    = NQ - 1;
    static constexpr int NQP   = NQ | 1;                              // pencil stride of a point image (odd)
    static constexpr int NP    = (DIM == 3) ? EC * NQ * NQ : EC * NQ; // point columns = pencils of any direction
    static constexpr int NPASS = cdiv(NP, kWave);
    static constexpr int IMG   = NP * NQP;                            // one point image, scalars
    static constexpr int NIMG  = (DIM == 3) ? 2 : 1;
    static constexpr int NCOMP = (DIM == 3) ? 6 : 3;
    static constexpr int RING  = NQ < kHelmRing ? NQ : kHelmRing;
    static constexpr int SLAB  = (CMax<M::SLAB, NIMG * IMG>::value + VW - 1) / VW * VW;
    static_assert(NP == ((DIM == 3) ? F::P2 : F::P1) && NPASS == ((DIM == 3) ? F::PASS2 : F::PASS1),
                  "the point columns are the pencils of the last forward sweep");
    static_assert(sizeof(T) * SLAB <= 16 * 1024, "slab per wave");
};

template <int NQ, int EC, int DIM, int WPB, typename T = double> constexpr size_t helmholtz_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * HelmGeom<NQ, EC, DIM, T>::SLAB;
}

// one slice n of the metric planes (and of w) of this lane's point columns; src offsets are in bounds for every lane
template <int NPASS, int NCOMP, int PLANE, int NQT, bool HASW, typename T>
__device__ __forceinline__ void load_metric_slice(T (&gv)[NPASS][NCOMP], T (&wv)[NPASS], const T *__restrict__ gc,
                                                  const T *__restrict__ wc, const int (&goff)[NPASS],
                                                  const int (&woff)[NPASS], int n)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c)
            gv[s][c] = __builtin_nontemporal_load(gc + goff[s] + c * NQT + n * PLANE);
        if constexpr (HASW)
            wv[s] = __builtin_nontemporal_load(wc + woff[s] + n * PLANE);
        else
            wv[s] = T(0);
    }
}

// pencils of a point image owned by this lane: p[s][m] = img[base[s] + m*ST]
template <int NQ, int NPASS, int ST, typename T>
__device__ __forceinline__ void read_image_pencils(T (&p)[NPASS][NQ], const T *img, const int (&base)[NPASS])
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
#pragma unroll
        for (int m = 0; m < NQ; ++m)
            p[s][m] = img[base[s] + m * ST];
}
template <int NQ, int NPASS, int ST, typename T>
__device__ __forceinline__ void write_image_pencils(const T (&p)[NPASS][NQ], T *img, const int (&base)[NPASS],
                                                    const bool (&own)[NPASS])
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
        if (own[s])
        {
#pragma unroll
            for (int m = 0; m < NQ; ++m)
                img[base[s] + m * ST] = p[s][m];
        }
}

// In-place pencil sweep over a point image: every owned pencil p becomes D p (DOT: q[i] = sum_m D[i][m] p[m]) or D^T p
// (q[i'] = sum_i D[i][i'] p[i]).  src == dst is safe: a lane reads its whole pencil before it writes it.
template <int NQ, int NPASS, int ST, int BMODE, bool DOT, typename T>
__device__ __forceinline__ void image_sweep(const T *src, T *dst, const int (&base)[NPASS], const bool (&own)[NPASS],
                                            const T *__restrict__ d)
{
    T p[NPASS][NQ], q[NPASS][NQ];
    read_image_pencils<NQ, NPASS, ST>(p, src, base);
    if constexpr (DOT)
        contract_dot<NQ, NQ, NPASS, BMODE>(p, q, d);
    else
        contract<NQ, NQ, NPASS, BMODE>(p, q, d);
    wave_lds_fence();
    write_image_pencils<NQ, NPASS, ST>(q, dst, base, own);
    wave_lds_fence();
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_helmholtz_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ g, const T *__restrict__ w, T lam,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NM2 = NM * NM, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING;
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
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS], bj[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ2, ab = tc - e * NQ2, a = ab / NQ, b = ab - a * NQ;
        ecol[s] = e;
        colp[s] = ab;                    // (j,i): offset inside a plane of g / w
        colo[s] = e * ES + a * NQP + b;  // (e,j,i): offset of the column's k = 0 point in an image
        bi[s]   = tc * NQP;              // (e,k,j): its i-pencil
        bj[s]   = e * ES + a * PL + b;   // (e,k,i): its j-pencil, stride NQP
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
        // the metric ring: the first slices, requested once the staging registers are consumed
        const T *gc = g + c * (uint64_t)(EC * G::NCOMP * NQT);
        const T *wc = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int goff[NPASS], woff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            goff[s]     = e * (G::NCOMP * NQT) + colp[s];
            woff[s]     = e * NQT + colp[s];
        }
        T gv[RING][NPASS][G::NCOMP], wv[RING][NPASS];
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_metric_slice<NPASS, G::NCOMP, NQ2, NQT, HASW>(gv[r], wv[r], gc, wc, goff, woff, r);
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
            // ---- the walk over k: fluxes f_a = sum_b G_ab du_b, mass term (lambda w) u --------------
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
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        const T(&gg)[G::NCOMP] = gv[k % RING][s];
                        const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = f2[s][k];
                        const T f0 = fma_t(gg[2], x2, fma_t(gg[1], x1, gg[0] * x0));
                        const T f1 = fma_t(gg[4], x2, fma_t(gg[3], x1, gg[1] * x0));
                        f2[s][k]   = fma_t(gg[5], x2, fma_t(gg[4], x1, gg[2] * x0));
                        u[s][k]    = HASW ? (lam * wv[k % RING][s]) * u[s][k] : T(0);
                        if (own[s])
                        {
                            imgD[colo[s] + k * PL] = f0;
                            imgU[colo[s] + k * PL] = f1;
                        }
                    }
                    if (k + RING < NQ)
                        load_metric_slice<NPASS, G::NCOMP, NQ2, NQT, HASW>(gv[k % RING], wv[k % RING], gc, wc, goff, woff,
                                                                          k + RING);
                    __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a slice
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
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_helmholtz_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ g, const T *__restrict__ w, T lam, const T *__restrict__ in, T *__restrict__ out,
    uint64_t nelmt)
{
    using G          = HelmGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING;
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
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ, b = tc - e * NQ;
        ecol[s] = e;
        colp[s] = b;          // i: offset inside a row of g / w
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
        const T *gc = g + c * (uint64_t)(EC * G::NCOMP * NQT);
        const T *wc = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int goff[NPASS], woff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            goff[s]     = e * (G::NCOMP * NQT) + colp[s];
            woff[s]     = e * NQT + colp[s];
        }
        T gv[RING][NPASS][G::NCOMP], wv[RING][NPASS];
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_metric_slice<NPASS, G::NCOMP, NQ, NQT, HASW>(gv[r], wv[r], gc, wc, goff, woff, r);
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
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        const T(&gg)[G::NCOMP] = gv[j % RING][s];
                        const T x0 = a0[j % 2][s], x1 = f1[s][j];
                        const T f0 = fma_t(gg[1], x1, gg[0] * x0);
                        f1[s][j]   = fma_t(gg[2], x1, gg[1] * x0);
                        u[s][j]    = HASW ? (lam * wv[j % RING][s]) * u[s][j] : T(0);
                        if (own[s])
                            imgU[colo[s] + j * NQP] = f0;
                    }
                    if (j + RING < NQ)
                        load_metric_slice<NPASS, G::NCOMP, NQ, NQT, HASW>(gv[j % RING], wv[j % RING], gc, wc, goff, woff,
                                                                         j + RING);
                    __builtin_amdgcn_sched_barrier(0);
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
