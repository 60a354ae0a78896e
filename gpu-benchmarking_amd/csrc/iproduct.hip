// iproduct.hip -- compile-time instantiations of the IProductWRTBase wave kernels (iproduct_wave.h) + nq dispatch.
// The configuration of every order is the BwdTrans row of wave_table.h (HexCfg / QuadCfg / *CfgF32): the transpose moves
// the same bytes and issues the same FMAs.  Two things differ from the BwdTrans rows and hold for every order: the output
// always leaves through the LDS stream (OUT_LDS), line-aligned (MEMF bit 3), and the chunks are never split into pieces.
#include "iproduct_wave.h"
#include "sf_dispatch.h"
#include "wave_launch.h"
#include "wave_table.h"

namespace sf
{

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_hex_iprod(const HexArgsT<T> &a, hipStream_t s)
{
    static OccCache cache = {};
    auto kern            = hex_iprod_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>;
    constexpr size_t lds = iprod_lds_bytes<NQ, EC, 3, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    if (a.nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (a.nelmt + EC - 1) / EC;
    const uint64_t per    = (uint64_t)WPB * KMAP;
    const uint64_t grid   = (nchunk + per - 1) / per;
    (void)resident_blocks(kern, kWave * WPB, lds, cache); // raises the kernel's LDS limit once per device
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * WPB, lds, s>>>(a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_quad_iprod(const QuadArgsT<T> &a, hipStream_t s)
{
    static OccCache cache = {};
    auto kern            = quad_iprod_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>;
    constexpr size_t lds = iprod_lds_bytes<NQ, EC, 2, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    if (a.nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (a.nelmt + EC - 1) / EC;
    const uint64_t per    = (uint64_t)WPB * KMAP;
    const uint64_t grid   = (nchunk + per - 1) / per;
    (void)resident_blocks(kern, kWave * WPB, lds, cache);
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * WPB, lds, s>>>(a.b0, a.b1, a.in, a.out, a.nelmt);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

// the BwdTrans row of the order, output through the line-aligned LDS stream
template <class C, int NQ, typename T> static int go_hex(const HexArgsT<T> &a, hipStream_t s)
{
    return launch_hex_iprod<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, s);
}
template <class C, int NQ, typename T> static int go_quad(const QuadArgsT<T> &a, hipStream_t s)
{
    return launch_quad_iprod<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, s);
}

#define SF_HEX_CASES(F)                                                                                                \
    F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11)
#define SF_QUAD_CASES(F)                                                                                               \
    F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

// SF_ENOTBUILT when the order has no instantiation (3D isotropic nq 2..11, 2D isotropic nq 2..16)
int launch_hex_iprod_wave_nq(unsigned nq, const HexArgs &a, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex<HexCfg<N>, N, double>(a, s);
        SF_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_hex_iprod_wave_f32_nq(unsigned nq, const HexArgsT<float> &a, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex<HexCfgF32<N>, N, float>(a, s);
        SF_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_iprod_wave_nq(unsigned nq, const QuadArgs &a, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad<QuadCfg<N>, N, double>(a, s);
        SF_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_iprod_wave_f32_nq(unsigned nq, const QuadArgsT<float> &a, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad<QuadCfgF32<N>, N, float>(a, s);
        SF_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

#undef SF_HEX_CASES
#undef SF_QUAD_CASES

bool iprod_wave_built(int dim, unsigned nq)
{
    return nq >= 2 && nq <= (dim == 3 ? 11u : 16u);
}

} // namespace sf
