// bwdtrans_wave2.h -- the 2D twin of bwdtrans_wave3.h: the wave-per-chunk kernel of bwdtrans_wave.h for ANISOTROPIC
// compile-time extents (nq0, nq1).  One wavefront per chunk of EC elements, flat 16-byte non-temporal loads / stores,
// lane owns a pencil, both images rewritten in place in one LDS slab, basis rows as SGPR operands, XCD runs.  The
// reference takes both extents at run time (benchmark04/benchmark04.cc:353-360); no shape of this template is
// compiled ahead of time: the library instantiates the ones a caller asks for at run time (rtc.hip).
#pragma once

#include "bwdtrans_wave.h"

namespace sf
{

// geometry with the member names chunk_fetch / chunk_stage / read_pencils / chunk_flush expect (NM = nm0)
template <int NQ0, int NQ1, int EC, typename T = double> struct WaveGeom2
{
    using Scalar = T;
    using Vec    = typename VecOf<T>::type;
    static constexpr int VW  = VecOf<T>::W;
    static constexpr int NM0 = NQ0 - 1, NM1 = NQ1 - 1;
    static constexpr int NM  = NM0;
    static constexpr int NMT = NM0 * NM1, NQT = NQ0 * NQ1;
    static constexpr int IN_STRIDE = NM0 | 1; // pencils (e,q) of nm0 values
    static constexpr int S1 = NM1 | 1;        // pencils (e,i) of nm1 values
    static constexpr int IN_DBL    = EC * NMT;
    static constexpr bool VEC2     = (IN_DBL % VW) == 0;
    static constexpr int P0 = EC * NM1, P1 = EC * NQ0;
    static constexpr int PASS0 = cdiv(P0, kWave), PASS1 = cdiv(P1, kWave);
    static constexpr int SLAB0    = CMax<P0 * IN_STRIDE, P1 * S1>::value;
    static constexpr int OUT_DBL  = EC * NQT;
    static constexpr int SLAB_OUT = (CMax<SLAB0, OUT_DBL>::value + VW - 1) / VW * VW;
    static constexpr int NLD      = VEC2 ? cdiv(IN_DBL / VW, kWave) : cdiv(IN_DBL, kWave);
};

template <int NQ0, int NQ1, int EC, int WPB, typename T = double> constexpr size_t wave2_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * WaveGeom2<NQ0, NQ1, EC, T>::SLAB_OUT;
}

template <int NQ0, int NQ1, int EC, int WPB, int BMODE, int MINW, int XG = 64, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_wave2_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G = WaveGeom2<NQ0, NQ1, EC, T>;
    constexpr int NM0 = G::NM0, NM1 = G::NM1, S1 = G::S1;
    static_assert(BMODE != BASIS_LDS, "basis rows are scalar operands");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw2[];
    T *lds = reinterpret_cast<T *>(lds_raw2);
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab = lds + wib * G::SLAB_OUT;

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const uint64_t c      = logical_block<XG>() * WPB + wib; // one chunk per short-lived wave
    if (c >= nchunk)
        return;
    const uint64_t left = nelmt - c * EC;
    const int evalid    = left >= EC ? EC : (int)left;

    typename G::Vec st[G::NLD];
    chunk_fetch<G, EC, true, false>(st, in, c, nelmt, lane);
    chunk_stage<G, false>(st, slab, lane, G::VEC2 ? 0 : line_offset<T>(in + c * G::IN_DBL));
    wave_lds_fence();

    // ---- direction 0: w1[(e,i)][q] = sum_p in[(e,q)][p] * B0[p][i] --------------------------------------------------
    {
        T u[G::PASS0][NM0], acc[G::PASS0][NQ0];
        read_pencils<NM0, G::PASS0, G::P0, G::IN_STRIDE>(u, slab, lane);
        contract<NM0, NQ0, G::PASS0, BMODE>(u, acc, b0);
        wave_lds_fence();
#pragma unroll
        for (int s = 0; s < G::PASS0; ++s)
        {
            const int t = s * kWave + lane;
            if ((s + 1) * kWave <= G::P0 || t < G::P0)
            {
                const int e = t / NM1, q = t - e * NM1;
                T *dst = slab + e * NQ0 * S1 + q;
#pragma unroll
                for (int i = 0; i < NQ0; ++i)
                    dst[i * S1] = acc[s][i];
            }
        }
        wave_lds_fence();
    }
    // ---- direction 1: out[e][j][i] = sum_q w1[(e,i)][q] * B1[q][j] --------------------------------------------------
    {
        T u[G::PASS1][NM1], acc[G::PASS1][NQ1];
        read_pencils<NM1, G::PASS1, G::P1, S1>(u, slab, lane);
        contract<NM1, NQ1, G::PASS1, BMODE>(u, acc, b1);
        wave_lds_fence();
#pragma unroll
        for (int s = 0; s < G::PASS1; ++s)
        {
            const int t = s * kWave + lane;
            if ((s + 1) * kWave <= G::P1 || t < G::P1)
            {
                const int e = t / NQ0, i = t - e * NQ0;
                T *dst = slab + e * G::NQT + i;
#pragma unroll
                for (int j = 0; j < NQ1; ++j)
                    dst[j * NQ0] = acc[s][j];
            }
        }
        wave_lds_fence();
        chunk_flush<G, true, false>(slab, out + c * (uint64_t)(EC * G::NQT), evalid * G::NQT, lane);
    }
}

} // namespace sf
