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

template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, typename T>
static int launch_iprod(const ArgsT<DIM, T> &a, hipStream_t s)
{
    static OccCache cache = {};
    constexpr size_t lds = slab_lds_bytes<IprodGeom<NQ, EC, DIM, T>, WPB>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(KMAP > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<WPB, EC, KMAP>(hex_iprod_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>,
                                             cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
    else
        return launch_chunked<WPB, EC, KMAP>(quad_iprod_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUT_LDS, MEMF, T>,
                                             cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.in, a.out, a.nelmt);
}

// the BwdTrans row of the order, output through the line-aligned LDS stream
template <int DIM, int NQ, typename T> static int go_iprod(const ArgsT<DIM, T> &a, hipStream_t s)
{
    using C = typename std::conditional<
        DIM == 3, typename std::conditional<sizeof(T) == 8, HexCfg<NQ>, HexCfgF32<NQ>>::type,
        typename std::conditional<sizeof(T) == 8, QuadCfg<NQ>, QuadCfgF32<NQ>>::type>::type;
    return launch_iprod<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, (C::MF | 8), T>(a, s);
}

#define SF_HEX_CASES(F)                                                                                                \
    F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11)
#define SF_QUAD_CASES(F)                                                                                               \
    F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

// SF_ENOTBUILT when the order has no instantiation (3D isotropic nq 2..11, 2D isotropic nq 2..16)
template <int DIM, typename T> int launch_iprod_wave(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s)
{
#define SF_CASE(N) case N: return go_iprod<DIM, N, T>(a, s);
    if constexpr (DIM == 3)
        switch (nq)
        {
            SF_HEX_CASES(SF_CASE)
        }
    else
        switch (nq)
        {
            SF_QUAD_CASES(SF_CASE)
        }
#undef SF_CASE
    return SF_ENOTBUILT;
}
template int launch_iprod_wave<3, double>(unsigned, const HexArgs &, hipStream_t);
template int launch_iprod_wave<3, float>(unsigned, const HexArgsT<float> &, hipStream_t);
template int launch_iprod_wave<2, double>(unsigned, const QuadArgs &, hipStream_t);
template int launch_iprod_wave<2, float>(unsigned, const QuadArgsT<float> &, hipStream_t);

#undef SF_HEX_CASES
#undef SF_QUAD_CASES

bool iprod_wave_built(int dim, unsigned nq)
{
    return nq >= 2 && nq <= (dim == 3 ? 11u : 16u);
}

} // namespace sf
