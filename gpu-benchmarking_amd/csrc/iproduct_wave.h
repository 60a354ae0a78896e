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
// transposed copy, no workspace, so every launch is capture-safe.  contract_dot lives next to contract in
// bwdtrans_wave.h: the tensor kernels of bwdtrans_aniso.h use both.
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
