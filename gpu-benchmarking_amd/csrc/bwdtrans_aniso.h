// bwdtrans_aniso.h -- the flagship wave-per-chunk kernel of bwdtrans_wave.h for ANISOTROPIC compile-time extents,
// (nq0, nq1, nq2) and (nq0, nq1): same structure -- one wavefront per chunk of EC elements, flat 16-byte non-temporal
// loads / stores, lane owns a pencil, the images rewritten in place in one LDS slab, basis rows as SGPR operands, XCD
// runs -- with every extent taken per direction (BwdGeom).  Each kernel is its prologue (one chunk per wave), the sweeps
// of frag/sweep.inc and the flush.  The reference kernels take the extents at run time
// (benchmark05/benchmark05.cc:291-297, benchmark04/benchmark04.cc:353-360).  3D: the shapes instantiated ahead of time
// are the table in bwdtrans_rt.hip, every other anisotropic shape runs the run-time-extent kernel of bwdtrans_rt.h.
// 2D: no shape is compiled ahead of time.  The library instantiates the shapes a caller asks for at run time (rtc.hip).
#pragma once

#include "bwdtrans_wave.h"

namespace sf
{

template <int NQ0, int NQ1, int NQ2, int EC, int WPB, int BMODE, int MINW, int XG = 64, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_wave3_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G = BwdGeom<3, EC, T, NQ0, NQ1, NQ2>;
    static_assert(BMODE != BASIS_LDS, "basis rows are scalar operands");

#include "frag/wave_slab.inc"
#include "frag/wave_one_chunk.inc"
    // ---- direction 0: w1[(e,i,r)][q] = sum_p in[(e,r,q)][p] * B0[p][i] --------------------------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b0
#include "frag/sweep.inc"
    // ---- direction 1: w2[(e,j,i)][r] = sum_q w1[(e,i,r)][q] * B1[q][j] --------------------------------------------
#define SWEEP G::Sw1
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b1
#include "frag/sweep.inc"
    // ---- direction 2: out[e][k][(j,i)] = sum_r w2[(e,j,i)][r] * B2[r][k] ------------------------------------------
#define SWEEP G::Sw2
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b2
#include "frag/sweep.inc"
    chunk_flush<G, true, false>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
}

template <int NQ0, int NQ1, int EC, int WPB, int BMODE, int MINW, int XG = 64, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_wave2_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G = BwdGeom<2, EC, T, NQ0, NQ1>;
    static_assert(BMODE != BASIS_LDS, "basis rows are scalar operands");

#include "frag/wave_slab.inc"
#include "frag/wave_one_chunk.inc"
    // ---- direction 0: w1[(e,i)][q] = sum_p in[(e,q)][p] * B0[p][i] --------------------------------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b0
#include "frag/sweep.inc"
    // ---- direction 1: out[e][j][i] = sum_q w1[(e,i)][q] * B1[q][j] --------------------------------------------------
#define SWEEP G::Sw1
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b1
#include "frag/sweep.inc"
    chunk_flush<G, true, false>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
}

} // namespace sf
