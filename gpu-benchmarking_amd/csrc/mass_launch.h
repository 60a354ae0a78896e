// mass_launch.h -- launchers and the per-order configuration of the fused mass kernels (mass_wave.h), shared by the fp64
// (mass.hip) and fp32 (mass_f32.hip) translation units.
//
// The configuration of an order starts from its BwdTrans row of wave_table.h (HexCfg / QuadCfg / *CfgF32), with the
// output through the line-aligned LDS stream (OUT_LDS, MEMF bit 3) as in iproduct.hip.  The fused kernel keeps more
// registers live than either half (the weights, and two accumulator sets at the hand-over), so MassHexCfg / MassQuadCfg
// override the rows whose MINW would make it spill; the rows of wave_table.h themselves are not touched.
#pragma once

#include "mass_wave.h"
#include "sf_dispatch.h"
#include "wave_launch.h"
#include "wave_table.h"

#include <type_traits>

namespace sf
{

template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_mass(const ArgsT<DIM, T> &a, const T *w, hipStream_t s)
{
    static OccCache cache = {};
    constexpr size_t lds = mass_lds_bytes<NQ, EC, DIM, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(KMAP > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<WPB, EC, KMAP>(hex_mass_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>,
                                             cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, w, a.in, a.out, a.nelmt);
    else
        return launch_chunked<WPB, EC, KMAP>(quad_mass_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>,
                                             cache, lds, 0, s, a.nelmt, a.b0, a.b1, w, a.in, a.out, a.nelmt);
}

// the BwdTrans row of the order unless overridden below
template <int NQ, typename T> struct MassHexCfg : std::conditional<sizeof(T) == 8, HexCfg<NQ>, HexCfgF32<NQ>>::type
{
};
template <int NQ, typename T> struct MassQuadCfg : std::conditional<sizeof(T) == 8, QuadCfg<NQ>, QuadCfgF32<NQ>>::type
{
};

template <int DIM, int NQ, typename T> static int go_mass(const ArgsT<DIM, T> &a, const T *w, hipStream_t s)
{
    using C = typename std::conditional<DIM == 3, MassHexCfg<NQ, T>, MassQuadCfg<NQ, T>>::type;
    return launch_mass<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, w, s);
}

#define SF_MASS_HEX_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11)
#define SF_MASS_QUAD_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

// SF_ENOTBUILT when the order has no instantiation (mass_wave_built()); instantiated for double in mass.hip and for float
// in mass_f32.hip
template <int DIM, typename T> int launch_mass_wave(unsigned nq, const ArgsT<DIM, T> &a, const T *w, hipStream_t s)
{
#define SF_CASE(N) case N: return go_mass<DIM, N, T>(a, w, s);
    if constexpr (DIM == 3)
        switch (nq)
        {
            SF_MASS_HEX_CASES(SF_CASE)
        }
    else
        switch (nq)
        {
            SF_MASS_QUAD_CASES(SF_CASE)
        }
#undef SF_CASE
    return SF_ENOTBUILT;
}

} // namespace sf
