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
// Shared text.  The front (forward sweeps), the derivative steps and the back (transposed sweeps and flush) are the
// fragments of csrc/frag/*.inc, in the sequence that helmholtz_wave.h lists; this header's own are the constant load,
// the walk body and the sum.  One spot is written out: the lane roles, which also form the weight product of the
// column (frag/lane_roles_*.inc followed by a loop for the weights changed the assembly of most instantiations).
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
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
    T *imgU = slab;          // u, then du_1, f_1, D_1^T f_1
    T *imgD = slab + G::IMG; // du_0, f_0, D_0^T f_0
#include "frag/wave_chunks.inc"
    // The lane roles of frag/lane_roles_3d.inc, written out: the weight product of the column is formed in the same loop
    // (formed after the shared text, the weight loads move and the assembly of most instantiations changes), no colp.
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
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // the constants of this chunk's elements, requested once the staging registers are consumed
        T gv[NPASS][G::NCOMP], lj[NPASS];
        load_element_constants<NPASS, G::NCOMP, EC, HASJ>(gv, lj, ge, je, lam, c * (uint64_t)EC, ecol, evalid);
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
#include "frag/forward1_3d.inc"
        // ---- forward 2 and everything at the points: lane (e,j,i) keeps its k-pencil in registers ---
        {
            T u[NPASS][NQ], dreg[NPASS][NQ], acc[NPASS][NM];
#include "frag/point_values_3d.inc"
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
                        const T x0 = a0[k % 2][s], x1 = a1[k % 2][s], x2 = dreg[s][k];
                        const T f0 = q * fma_t(gg[2], x2, fma_t(gg[1], x1, gg[0] * x0));
                        const T f1 = q * fma_t(gg[4], x2, fma_t(gg[3], x1, gg[1] * x0));
                        dreg[s][k] = q * fma_t(gg[5], x2, fma_t(gg[4], x1, gg[2] * x0)); // f_2
                        u[s][k]    = HASJ ? (lj[s] * q) * u[s][k] : T(0);
                        if (own[s])
                        {
                            imgD[colo[s] + k * PL] = f0;
                            imgU[colo[s] + k * PL] = f1;
                        }
                    }
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

#include "frag/wave_slab.inc"
    T *imgU = slab; // u, then du_0, f_0, D_0^T f_0
#include "frag/wave_chunks.inc"
    // the lane roles of frag/lane_roles_2d.inc, written out for the same reason as in the 3D kernel
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
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        T gv[NPASS][G::NCOMP], lj[NPASS];
        load_element_constants<NPASS, G::NCOMP, EC, HASJ>(gv, lj, ge, je, lam, c * (uint64_t)EC, ecol, evalid);
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
                    const T qj = qw1[j];
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
                    {
                        const T(&gg)[G::NCOMP] = gv[s];
                        const T q  = qj * qi[s];
                        const T x0 = a0[j % 2][s], x1 = dreg[s][j];
                        const T f0 = q * fma_t(gg[1], x1, gg[0] * x0);
                        dreg[s][j] = q * fma_t(gg[2], x1, gg[1] * x0); // f_1
                        u[s][j]    = HASJ ? (lj[s] * q) * u[s][j] : T(0);
                        if (own[s])
                            imgU[colo[s] + j * NQP] = f0;
                    }
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
