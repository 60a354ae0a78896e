// bwdtrans_aniso.h -- the flagship wave-per-chunk kernel of bwdtrans_wave.h for ANISOTROPIC compile-time extents,
// (nq0, nq1, nq2) and (nq0, nq1): same structure -- one wavefront per chunk of EC elements, flat 16-byte non-temporal
// loads / stores, lane owns a pencil, the images rewritten in place in one LDS slab, basis rows as SGPR operands, XCD
// runs -- with every extent taken per direction (BwdGeom).  Each kernel is its prologue (one chunk per wave), the sweeps
// of frag/sweep.inc and the flush.  The reference kernels take the extents at run time
// (benchmark05/benchmark05.cc:291-297, benchmark04/benchmark04.cc:353-360).  3D: the shapes instantiated ahead of time
// are the table in bwdtrans_rt.hip, every other anisotropic shape runs the run-time-extent kernel of bwdtrans_rt.h.
// 2D: no shape is compiled ahead of time.  The library instantiates the shapes a caller asks for at run time (rtc.hip).
//
// hex_tensor_wave_kernel / quad_tensor_wave_kernel (sf_tensor_*) are the same kernels with the input and the output
// length of every direction named separately (SweepGeom) and the matrix of a direction read row-major I x O (TR = 0,
// contract) or row-major O x I (TR = 1, contract_dot).  Their table is tensor_launch.h, every other shape is instantiated
// at run time (rtc.hip).
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

// ---- sf_tensor_*: independent input / output extents ----------------------------------------------------------------
// The contraction of a sweep by the layout of its matrix: TR = 0 row-major NIN x NOUT, TR = 1 row-major NOUT x NIN.  Both
// sum in ascending summed index, the first term a multiplication, the rest FMAs.
template <int TR> struct TensorContract
{
    template <int NIN, int NOUT, int NPASS, int BMODE, typename T>
    static __device__ __forceinline__ void run(const T (&u)[NPASS][NIN], T (&acc)[NPASS][NOUT], const T *__restrict__ bas)
    {
        if constexpr (TR == 0)
            contract<NIN, NOUT, NPASS, BMODE>(u, acc, bas);
        else
            contract_dot<NIN, NOUT, NPASS, BMODE>(u, acc, bas);
    }
};

template <int I0, int O0, int I1, int O1, int I2, int O2, int TR, int EC, int WPB, int BMODE, int MINW, int XG = 64,
          typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_tensor_wave_kernel(
    const T *__restrict__ m0, const T *__restrict__ m1, const T *__restrict__ m2,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G = SweepGeom<3, EC, T, I0, O0, I1, O1, I2, O2>;
    static_assert(BMODE != BASIS_LDS, "matrix rows are scalar operands");
    static_assert(TR == 0 || TR == 1, "trans is 0 or 1");

#include "frag/wave_slab.inc"
#include "frag/wave_one_chunk.inc"
    // ---- direction 0: w1[(e,i,r)][q] = sum_p in[(e,r,q)][p] * M0(p,i) -----------------------------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT TensorContract<TR>::template run
#define SWEEP_BASIS m0
#include "frag/sweep.inc"
    // ---- direction 1: w2[(e,j,i)][r] = sum_q w1[(e,i,r)][q] * M1(q,j) -----------------------------------------------
#define SWEEP G::Sw1
#define SWEEP_CONTRACT TensorContract<TR>::template run
#define SWEEP_BASIS m1
#include "frag/sweep.inc"
    // ---- direction 2: out[e][k][(j,i)] = sum_r w2[(e,j,i)][r] * M2(r,k) ---------------------------------------------
#define SWEEP G::Sw2
#define SWEEP_CONTRACT TensorContract<TR>::template run
#define SWEEP_BASIS m2
#include "frag/sweep.inc"
    chunk_flush<G, true, false>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
}

template <int I0, int O0, int I1, int O1, int TR, int EC, int WPB, int BMODE, int MINW, int XG = 64, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_tensor_wave_kernel(
    const T *__restrict__ m0, const T *__restrict__ m1, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G = SweepGeom<2, EC, T, I0, O0, I1, O1>;
    static_assert(BMODE != BASIS_LDS, "matrix rows are scalar operands");
    static_assert(TR == 0 || TR == 1, "trans is 0 or 1");

#include "frag/wave_slab.inc"
#include "frag/wave_one_chunk.inc"
    // ---- direction 0: w1[(e,i)][q] = sum_p in[(e,q)][p] * M0(p,i) ---------------------------------------------------
#define SWEEP G::Sw0
#define SWEEP_CONTRACT TensorContract<TR>::template run
#define SWEEP_BASIS m0
#include "frag/sweep.inc"
    // ---- direction 1: out[e][j][i] = sum_q w1[(e,i)][q] * M1(q,j) ---------------------------------------------------
#define SWEEP G::Sw1
#define SWEEP_CONTRACT TensorContract<TR>::template run
#define SWEEP_BASIS m1
#include "frag/sweep.inc"
    chunk_flush<G, true, false>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::OUT_ELEM, lane);
}

} // namespace sf
