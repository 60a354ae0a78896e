// helmholtz_wave.h -- the fused Helmholtz operator as wave-per-chunk kernels for gfx950.
//
//   y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e
//
// B the tensor-product BwdTrans basis, D_a the collocation derivative matrix of direction a at the quadrature points
// (row-major nq x nq, (D_a u)[i] = sum_m deriv_a[i*nq + m] u[m]), G the symmetric metric tensor per point, stored as
// component planes g[e][c][k][j][i] (3D: c = 00, 01, 02, 11, 12, 22; 2D: c = 00, 01, 11), w the mass weight per point.
// BwdTrans, three (two) derivatives, the metric contraction, the transposed derivatives and IProductWRTBase in ONE
// kernel: the quadrature-space images never exist in HBM.  The front (chunk_fetch / chunk_stage, the forward sweeps) and
// the back (the transposed sweeps, chunk_flush) are those of the mass kernel, the same text: csrc/frag/*.inc, included
// in place (mass_wave.h says how the fragments work and which names they expect).  A kernel below is, in order:
//   wave_slab, [imgU, imgD], wave_chunks, lane_roles, chunk_fetch_first | per chunk: chunk_head, chunk_stage, [the
//   first slices of the metric ring], chunk_fetch_next, forward0, forward1 (3D), point_values (steps 1 end and 2),
//   [the walk: steps 3 and the mass term], deriv_transposed (D_a^T), [the sum of step 4], transposed_last,
//   transposed1 (3D), transposed0.
// The bracketed parts are this header's own; affine_wave.h, physderiv_wave.h and iprodderiv_wave.h put other middles
// between the same fragments.  dreg is the register pencil of the last direction: du_2 before the walk, f_2 after it.
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
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab;          // u, then du_1, f_1, D_1^T f_1
    T *imgD = slab + G::IMG; // du_0, f_0, D_0^T f_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_3d.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
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
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
#include "frag/forward1_3d.inc"
        // ---- forward 2 and everything at the points: lane (e,j,i) keeps its k-pencil in registers ---
        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
#include "frag/point_values_3d.inc"
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
                        const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = dreg[s][k];
                        const T f0 = fma_t(gg[2], x2, fma_t(gg[1], x1, gg[0] * x0));
                        const T f1 = fma_t(gg[4], x2, fma_t(gg[3], x1, gg[1] * x0));
                        dreg[s][k] = fma_t(gg[5], x2, fma_t(gg[4], x1, gg[2] * x0)); // f_2
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
#include "frag/deriv_transposed_3d.inc"
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int k = 0; k < NQ; ++k)
                    u[s][k] = ((u[s][k] + imgD[colo[s] + k * PL]) + imgU[colo[s] + k * PL]) + t2[s][k];
#include "frag/transposed_last_3d.inc"
        }
#include "frag/transposed1_3d.inc"
#include "frag/transposed0.inc"
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

#include "frag/wave_slab.inc"
    T *imgU = slab; // u, then du_0, f_0, D_0^T f_0
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_2d.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // the metric ring, as in the 3D kernel
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
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
        // ---- forward 1 and everything at the points: lane (e,i) keeps its j-pencil in registers -----
        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
#include "frag/point_values_2d.inc"
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
                        const T x0 = a0[j % 2][s], x1 = dreg[s][j];
                        const T f0 = fma_t(gg[1], x1, gg[0] * x0);
                        dreg[s][j] = fma_t(gg[2], x1, gg[1] * x0); // f_1
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
#include "frag/deriv_transposed_2d.inc"
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    u[s][j] = (u[s][j] + imgU[colo[s] + j * NQP]) + t1[s][j];
#include "frag/transposed_last_2d.inc"
        }
#include "frag/transposed0.inc"
    }
}

} // namespace sf
