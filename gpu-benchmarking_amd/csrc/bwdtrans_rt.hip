// bwdtrans_rt.hip -- launcher of the run-time-extent wave kernel (bwdtrans_rt.h): what SF_VARIANT_AUTO runs for
// anisotropic 3D extents up to 16 per direction (the reference takes nq0, nq1, nq2 at run time,
// benchmark05/benchmark05.cc:291-297, 1425-1429).
#include "bwdtrans_rt.h"
#include "bwdtrans_aniso.h"
#include "chunked_launch.h"
#include "rtc_config.h"
#include "sf_dispatch.h"

namespace sf
{

static unsigned magic_of(unsigned d)
{
    return d <= 1 ? 0u : (unsigned)((0x100000000ull + d - 1) / d);
}

template <int NB> static int go_rt(const RtShape &sh, int wpb, size_t lds, const HexArgs &a, hipStream_t s)
{
    auto kern = hex_wave_rt_kernel<NB>;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const uint64_t nchunk = (a.nelmt + sh.ec - 1) / sh.ec;
    const uint64_t grid   = (nchunk + wpb - 1) / wpb;
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * wpb, lds, s>>>(sh, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}

// ---- compile-time triples (bwdtrans_aniso.h) -----------------------------------------------------------------------
// EC: chunks of about one nq = 8 element (512 points) -- the footprint the isotropic rows converged on
template <int NQ0, int NQ1, int NQ2> struct Cfg3
{
    static constexpr int NQT = NQ0 * NQ1 * NQ2;
    static constexpr int EC  = 512 / NQT < 1 ? 1 : (512 / NQT > 8 ? 8 : 512 / NQT);
    static constexpr int MX  = NQ0 > NQ1 ? (NQ0 > NQ2 ? NQ0 : NQ2) : (NQ1 > NQ2 ? NQ1 : NQ2);
    static constexpr int BM  = MX <= 10 ? BASIS_SMEM : BASIS_SMEM_COLS;
};

template <int NQ0, int NQ1, int NQ2> static int go3(const HexArgs &a, hipStream_t s)
{
    using C = Cfg3<NQ0, NQ1, NQ2>;
    static OccCache cache = {};
    constexpr size_t lds  = slab_lds_bytes<BwdGeom<3, C::EC, double, NQ0, NQ1, NQ2>, 4>();
    static_assert(lds <= 64 * 1024, "LDS slab");
    // one chunk per short-lived wave (KMAP = 1), four waves per workgroup
    return launch_chunked<4, C::EC, 1>(hex_wave3_kernel<NQ0, NQ1, NQ2, C::EC, 4, C::BM, 2>, cache, lds, 0, s, a.nelmt, a.b0,
                                       a.b1, a.b2, a.in, a.out, a.nelmt);
}

// The instantiated shapes: every ordering of the extents {8,8,4}, {4,8,6}, {10,6,8} (the shapes the round-2 review
// names) and of the neighbouring-order mixes a p-adaptive mesh produces around the benchmark's orders.
#define SF_TRIPLES(X)                                                                                                        \
    X(8, 8, 4) X(8, 4, 8) X(4, 8, 8) X(4, 8, 6) X(4, 6, 8) X(8, 4, 6) X(8, 6, 4) X(6, 4, 8) X(6, 8, 4) X(10, 6, 8)           \
    X(10, 8, 6) X(6, 10, 8) X(6, 8, 10) X(8, 10, 6) X(8, 6, 10) X(8, 8, 6) X(8, 6, 8) X(6, 8, 8) X(6, 6, 8) X(6, 8, 6)       \
    X(8, 6, 6) X(8, 8, 10) X(8, 10, 8) X(10, 8, 8) X(10, 10, 8) X(10, 8, 10) X(8, 10, 10) X(6, 6, 4) X(6, 4, 6) X(4, 6, 6)   \
    X(4, 4, 6) X(4, 6, 4) X(6, 4, 4)

// the run-time specialisation's host-side configuration (rtc_config.h) restates Cfg3 and the slab of BwdGeom: pinned
// here to the template's own values for every compile-time triple
template <int A, int B, int C> constexpr bool rtc_matches_cfg3()
{
    constexpr RtcCfg r = rtc_cfg(3, A, B, C, 8);
    using C3           = Cfg3<A, B, C>;
    using G            = BwdGeom<3, C3::EC, double, A, B, C>;
    return r.ec == C3::EC && r.bmode == C3::BM && r.wpb == 4 && r.minw == 2 && r.xg == 64 && r.slab == G::SLAB &&
           r.lds == slab_lds_bytes<G, 4>();
}
#define SF_PIN3(A, B, C) static_assert(rtc_matches_cfg3<A, B, C>(), "rtc_config.h disagrees with Cfg3 / BwdGeom");
SF_TRIPLES(SF_PIN3)
#undef SF_PIN3

// SF_ENOTBUILT: the shape is not in the table (the caller then takes the run-time-extent kernel)
int launch_hex_wave3(unsigned nq0, unsigned nq1, unsigned nq2, const HexArgs &a, hipStream_t s)
{
    const unsigned key = (nq0 << 16) | (nq1 << 8) | nq2;
    switch (key)
    {
#define SF_CASE3(A, B, C)                                                                                                    \
    case ((A << 16) | (B << 8) | C): return go3<A, B, C>(a, s);
        SF_TRIPLES(SF_CASE3)
#undef SF_CASE3
    default: return SF_ENOTBUILT;
    }
}

// SF_ENOTBUILT: an extent above 16, or one element's images beyond what a wave's share of the LDS holds
int launch_hex_rt(unsigned nq0, unsigned nq1, unsigned nq2, const HexArgs &a, hipStream_t s)
{
    const unsigned mx = nq0 > nq1 ? (nq0 > nq2 ? nq0 : nq2) : (nq1 > nq2 ? nq1 : nq2);
    if (mx > 16 || nq0 < 2 || nq1 < 2 || nq2 < 2)
        return SF_ENOTBUILT;
    if (a.nelmt == 0)
        return SF_OK;
    const int nb = (int)((mx + 1) / 2 * 2);
    RtShape sh;
    sh.nq0 = (int)nq0, sh.nq1 = (int)nq1, sh.nq2 = (int)nq2;
    sh.nm0 = sh.nq0 - 1, sh.nm1 = sh.nq1 - 1, sh.nm2 = sh.nq2 - 1;
    sh.s0 = sh.nm0 | 1, sh.s1 = sh.nm1 | 1, sh.s2 = sh.nm2 | 1;
    sh.nmt = sh.nm0 * sh.nm1 * sh.nm2, sh.nqt = sh.nq0 * sh.nq1 * sh.nq2;
    // elements per chunk: enough pencils to fill the 64 lanes in the last (widest) sweep, at most 16 KiB of images per wave
    const auto images = [&](int ec, int *off_b) {
        const int in_img = sh.nm2 * sh.nm1 * sh.s0, w2 = sh.nq1 * sh.nq0 * sh.s2;
        const int w1 = sh.nq0 * sh.nm2 * sh.s1;
        const int za = (ec * (in_img > w2 ? in_img : w2) + 1) & ~1, zb = (ec * (w1 > sh.nqt ? w1 : sh.nqt) + 1) & ~1;
        *off_b = za;
        return za + zb;
    };
    // chunks that fill the 64 lanes in the widest sweep (nq0 nq1 pencils per element); larger chunks measured slower
    // (their LDS images cost more occupancy than the shared basis rows give back)
    int ec = 64 / (sh.nq0 * sh.nq1);
    ec = ec < 1 ? 1 : (ec > 16 ? 16 : ec);
    int off_b = 0;
    while (ec > 1 && images(ec, &off_b) > 2048)
        --ec;
    sh.ec    = ec;
    sh.slab  = images(ec, &off_b);
    sh.off_b = off_b;
    if (sh.ec * sh.nqt >= 65536 || sh.ec * sh.nq0 * sh.nq1 * sh.s2 >= 65536)
        return SF_ENOTBUILT; // the index arithmetic divides by multiplication, exact below 2^16
    sh.m_nm0 = magic_of(sh.nm0), sh.m_nm1 = magic_of(sh.nm1), sh.m_nm12 = magic_of(sh.nm1 * sh.nm2);
    sh.m_nm2 = magic_of(sh.nm2), sh.m_nq0nm2 = magic_of(sh.nq0 * sh.nm2), sh.m_nq01 = magic_of(sh.nq0 * sh.nq1);
    const size_t basis = 0;
    int wpb            = 4;
    while (wpb > 1 && basis + sizeof(double) * (size_t)wpb * sh.slab > 64 * 1024)
        wpb >>= 1;
    const size_t lds = basis + sizeof(double) * (size_t)wpb * sh.slab;
    if (lds > 160 * 1024)
        return SF_ENOTBUILT;
    switch (nb)
    {
    case 2: return go_rt<2>(sh, wpb, lds, a, s);
    case 4: return go_rt<4>(sh, wpb, lds, a, s);
    case 6: return go_rt<6>(sh, wpb, lds, a, s);
    case 8: return go_rt<8>(sh, wpb, lds, a, s);
    case 10: return go_rt<10>(sh, wpb, lds, a, s);
    case 12: return go_rt<12>(sh, wpb, lds, a, s);
    case 14: return go_rt<14>(sh, wpb, lds, a, s);
    case 16: return go_rt<16>(sh, wpb, lds, a, s);
    default: return SF_ENOTBUILT;
    }
}

} // namespace sf
