// iproduct_wave.h -- IProductWRTBase, the transpose of BwdTrans, as wave-per-chunk kernels for gfx950.
//
//   3D: out[e][r][q][p] = sum_k sum_j sum_i in[e][k][j][i] * B0[p][i] * B1[q][j] * B2[r][k]
//   2D: out[e][q][p]    = sum_j sum_i       in[e][j][i]    * B0[p][i] * B1[q][j]
//
// Same bases (row-major nm x nq), extents and element-major layouts as the BwdTrans kernels of bwdtrans_wave.h, with the
// roles of `in` (nq^d points per element) and `out` (nm^d modes per element) swapped.  Everything but the contraction is
// the BwdTrans machinery: one wavefront owns a chunk of EC elements, the chunk is fetched one chunk ahead into staging
// registers (chunk_fetch) and staged into the wave's LDS slab with odd pencil strides (chunk_stage), each sweep is "lane
// owns a pencil", and the chunk's output image leaves through the slab as one flat 16-byte-per-lane stream (OUT_LDS,
// chunk_flush) -- the only sensible output path, since nm^d is odd at every even order (343 at nq = 8).
//
// Sweep order i -> p (B0), then j -> q (B1), then k -> r (B2); each sum is taken in ascending index.  A sweep contracts a
// pencil of nq values into nm values with the DOT-PRODUCT form acc[p] = sum_i u[i] * B[p][i]: the caller's basis array is
// read as it is, row by row (row p = B[p][0 .. nq), contiguous), through the two-deep SGPR ring of contract() -- no
// transposed copy, no workspace, so every launch is capture-safe.
//
// Both kernels are the front fragments of the fused operators (frag/wave_slab.inc .. frag/chunk_fetch_next.inc) and the
// sweeps of frag/sweep.inc with contract_dot.  The last sweep of the quad kernel stays written out: as frag/sweep.inc
// with G::Sw1 it changed the code of 24 of the 51 kernels of iproduct.hip, all of them quad_iprod_wave_kernel.
#pragma once

#include "bwdtrans_wave.h"

namespace sf
{

// The geometry of BwdTrans (bwdtrans_wave.h) with the lengths swapped: every direction contracts nq values to nm.  The
// chunk I/O (chunk_fetch, chunk_stage, chunk_flush) reads it as it is.
template <int NQ, int EC, int DIM, typename T = double>
using IprodGeom = SweepGeom<DIM, EC, T, NQ, NQ - 1, NQ, NQ - 1, DIM == 3 ? NQ : 1, DIM == 3 ? NQ - 1 : 1>;

// ------------------------------------------------------------------------------------------------
// Dot-product contraction, columns [I0, I0+NB) of every basis row: acc[s][p] (+)= sum_i u[s][i] * B[p*NIN + i], ascending
// i (I0 == 0 starts the sums).  The rows go through a two-deep SGPR ring in the order of contract(): (1) touch row p (the
// wait for its scalar loads lands here), (2) request row p+1, (3) the FMAs of row p, (4) an order fence on row p's
// results, so that neither the next row's loads nor its FMAs move across.  BASIS_SMEM streams whole rows (NB = NIN);
// BASIS_SMEM_COLS{,16} take the rows in blocks of 8 / 16 columns, then the next block.
// ------------------------------------------------------------------------------------------------
template <int NIN, int NOUT, int NPASS, int I0, int KB, typename T>
__device__ __forceinline__ void contract_dot_cols(const T (&u)[NPASS][NIN], T (&acc)[NPASS][NOUT],
                                                  const T *__restrict__ bas, int &zero)
{
    constexpr int NB = (NIN - I0) < KB ? (NIN - I0) : KB;
    T b[2][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
        b[0][i] = bas[zero + I0 + i];
#pragma unroll
    for (int p = 0; p < NOUT; ++p)
    {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            asm volatile("" : "+s"(zero) : "s"(b[p % 2][i]));
        if (p + 1 < NOUT)
        {
#pragma unroll
            for (int i = 0; i < NB; ++i)
                b[(p + 1) % 2][i] = bas[zero + (p + 1) * NIN + I0 + i];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            T a = (I0 == 0) ? u[s][0] * b[p % 2][0] : fma_t(u[s][I0], b[p % 2][0], acc[s][p]);
#pragma unroll
            for (int i = 1; i < NB; ++i)
                a = fma_t(u[s][I0 + i], b[p % 2][i], a);
            acc[s][p] = a;
        }
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
            asm volatile("" : "+s"(zero) : "v"(acc[s][p]));
    }
    if constexpr (I0 + NB < NIN)
        contract_dot_cols<NIN, NOUT, NPASS, I0 + NB, KB, T>(u, acc, bas, zero);
}

template <int NIN, int NOUT, int NPASS, int BMODE, typename T>
__device__ __forceinline__ void contract_dot(const T (&u)[NPASS][NIN], T (&acc)[NPASS][NOUT], const T *__restrict__ bas)
{
    static_assert(BMODE == BASIS_SMEM || BMODE == BASIS_SMEM_COLS || BMODE == BASIS_SMEM_COLS16,
                  "the transposed kernels take the basis as scalar operands");
    // opaque zero offset: the pointer stays a provably global kernel argument (s_load), the loads stay in the loop
    int zero = 0;
    asm volatile("s_mov_b32 %0, 0" : "=s"(zero));
    constexpr int KB = BMODE == BASIS_SMEM ? NIN : (BMODE == BASIS_SMEM_COLS ? 8 : 16);
    contract_dot_cols<NIN, NOUT, NPASS, 0, KB, T>(u, acc, bas, zero);
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_iprod_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G  = IprodGeom<NQ, EC, 3, T>;
    using IO = G;
    static_assert(OUTM == OUT_LDS, "the output (nm^3 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
#include "frag/chunk_fetch_next.inc"
        // ---- direction 0: w1[(e,p,k)][j] = sum_i in[(e,k,j)][i] * B0[p][i] ------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT contract_dot
#define SWEEP_BASIS b0
#include "frag/sweep.inc"
        // ---- direction 1: w2[(e,q,p)][k] = sum_j w1[(e,p,k)][j] * B1[q][j] ------------------------
#define SWEEP G::Sw1
#define SWEEP_CONTRACT contract_dot
#define SWEEP_BASIS b1
#include "frag/sweep.inc"
        // ---- direction 2: out[e][r][(q,p)] = sum_k w2[(e,q,p)][k] * B2[r][k] ----------------------
#define SWEEP G::Sw2
#define SWEEP_CONTRACT contract_dot
#define SWEEP_BASIS b2
#include "frag/sweep.inc"
        chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
        wave_lds_fence(); // slab is rewritten by the next chunk's staging
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_iprod_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G          = IprodGeom<NQ, EC, 2, T>;
    using IO         = G;
    constexpr int NM = NQ - 1;
    static_assert(OUTM == OUT_LDS, "the output (nm^2 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
#include "frag/chunk_fetch_next.inc"
        // ---- direction 0: w[(e,p)][j] = sum_i in[(e,j)][i] * B0[p][i] -----------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT contract_dot
#define SWEEP_BASIS b0
#include "frag/sweep.inc"
        // ---- direction 1: out[e][q][p] = sum_j w[(e,p)][j] * B1[q][j] -----------------------------
        {
            T u[G::PASS1][NQ], acc[G::PASS1][NM];
            read_pencils<NQ, G::PASS1, G::P1, G::S1>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS1, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P1 || t < G::P1)
                {
                    const int e = t / NM, p = t - e * NM;
                    T *dst = slab + e * G::OUT_ELEM + p;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NM] = acc[s][q];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
            wave_lds_fence();
        }
    }
}

} // namespace sf
