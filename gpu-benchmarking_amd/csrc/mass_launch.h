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

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_hex_mass(const HexArgsT<T> &a, const T *w, hipStream_t s)
{
    static OccCache cache = {};
    auto kern            = hex_mass_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>;
    constexpr size_t lds = mass_lds_bytes<NQ, EC, 3, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    if (a.nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (a.nelmt + EC - 1) / EC;
    const uint64_t per    = (uint64_t)WPB * KMAP;
    const uint64_t grid   = (nchunk + per - 1) / per;
    (void)resident_blocks(kern, kWave * WPB, lds, cache); // raises the kernel's LDS limit once per device
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * WPB, lds, s>>>(a.b0, a.b1, a.b2, w, a.in, a.out, a.nelmt);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_quad_mass(const QuadArgsT<T> &a, const T *w, hipStream_t s)
{
    static OccCache cache = {};
    auto kern            = quad_mass_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>;
    constexpr size_t lds = mass_lds_bytes<NQ, EC, 2, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    if (a.nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (a.nelmt + EC - 1) / EC;
    const uint64_t per    = (uint64_t)WPB * KMAP;
    const uint64_t grid   = (nchunk + per - 1) / per;
    (void)resident_blocks(kern, kWave * WPB, lds, cache);
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * WPB, lds, s>>>(a.b0, a.b1, w, a.in, a.out, a.nelmt);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

// the BwdTrans row of the order unless overridden below
template <int NQ, typename T> struct MassHexCfg : std::conditional<sizeof(T) == 8, HexCfg<NQ>, HexCfgF32<NQ>>::type
{
};
template <int NQ, typename T> struct MassQuadCfg : std::conditional<sizeof(T) == 8, QuadCfg<NQ>, QuadCfgF32<NQ>>::type
{
};

template <int NQ, typename T> static int go_hex_mass(const HexArgsT<T> &a, const T *w, hipStream_t s)
{
    using C = MassHexCfg<NQ, T>;
    return launch_hex_mass<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, w, s);
}
template <int NQ, typename T> static int go_quad_mass(const QuadArgsT<T> &a, const T *w, hipStream_t s)
{
    using C = MassQuadCfg<NQ, T>;
    return launch_quad_mass<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, w, s);
}

#define SF_MASS_HEX_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11)
#define SF_MASS_QUAD_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

} // namespace sf
