// helmholtz_launch.h -- launchers and the per-order configuration of the fused Helmholtz kernels (helmholtz_wave.h),
// shared by the fp64 (helmholtz.hip) and fp32 (helmholtz_f32.hip) translation units.
//
// The configuration of an order starts from its BwdTrans row of wave_table.h (HexCfg / QuadCfg / *CfgF32) with the output
// through the line-aligned LDS stream (OUT_LDS, MEMF bit 3), as the mass kernels do.  Two overrides, both because the
// kernel keeps more alive than either half (the point values, one flux, the metric ring and a pencil sweep's operands
// per point column; two point images per chunk in 3D):
//   * at most 128 point columns per chunk (two passes of the wave): 3D EC <= 128 / nq^2 -- the rows of nq 2, and in fp32
//     nq 3, 6 and 7, shrink; fp64 nq 6 takes one element -- and 2D EC <= 128 / nq from nq 9 (fp32 nq 13 shrinks);
//   * at most two waves per SIMD are asked of the register allocator (MINW <= 2): with the rows' MINW = 4 the fp64
//     3D nq 7 / 8 and several fp32 kernels spill one to eighteen registers.
// The table: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with and without the mass term (HASW).
// 3D nq 9..11 are NOT in the table (their point images and registers have not been fitted): AUTO sends them to the
// any-extent kernel of helmholtz_generic.hip, SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "helmholtz_wave.h"
#include "sf_dispatch.h"
#include "wave_launch.h"
#include "wave_table.h"

#include <type_traits>

namespace sf
{

// One launcher for the kernels of helmholtz_wave.h and of affine_wave.h (affine_launch.h).  The struct of the extra
// arguments, X = HelmArgsT<T> / AffineArgsT<T>, picks the family: HelmFamily<X> names its kernels, hands them their
// arguments and says whether the mass term is on.
template <class X> struct HelmFamily;
template <typename T> struct HelmFamily<HelmArgsT<T>>
{
    static bool has_mass(const HelmArgsT<T> &x) { return x.w != nullptr; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(hex_helmholtz_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.g, x.w,
                                                 x.lam, a.in, a.out, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(quad_helmholtz_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, x.d0, x.d1, x.g, x.w, x.lam, a.in,
                                                 a.out, a.nelmt);
    }
};

// the occupancy cache is one per kernel instantiation: X is among the template arguments
template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASM, typename T, class X>
static int launch_helm_k(const ArgsT<DIM, T> &a, const X &x, hipStream_t s)
{
    static OccCache cache = {};
    constexpr size_t lds = helmholtz_lds_bytes<NQ, EC, DIM, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(KMAP > 0, "short-lived waves: the grid covers the batch");
    return HelmFamily<X>::template launch<DIM, NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASM>(cache, lds, a, x, s);
}

constexpr int helm_hex_ec(int nq, int row_ec, int scalar_bytes)
{
    if (nq == 6 && scalar_bytes == 8)
        return 1; // two elements are 72 columns: two passes at the lane use of one (36 of 64), twice the registers
    const int cap = 128 / (nq * nq) > 0 ? 128 / (nq * nq) : 1;
    return row_ec < cap ? row_ec : cap;
}
constexpr int helm_quad_ec(int nq, int row_ec)
{
    const int cap = nq >= 9 ? 128 / nq : row_ec; // fp32 nq 13 (16 elements, four passes of 13-long pencils) spills
    return row_ec < cap ? row_ec : cap;
}

template <int NQ, typename T> struct HelmHexCfg
{
    using R = typename std::conditional<sizeof(T) == 8, HexCfg<NQ>, HexCfgF32<NQ>>::type;
    static constexpr int EC = helm_hex_ec(NQ, R::EC, (int)sizeof(T)), WPB = R::WPB, BM = R::BM;
    static constexpr int MW = R::MW > 2 ? 2 : R::MW;
    static constexpr int KM = R::KM, MF = R::MF | 8;
};
template <int NQ, typename T> struct HelmQuadCfg
{
    using R = typename std::conditional<sizeof(T) == 8, QuadCfg<NQ>, QuadCfgF32<NQ>>::type;
    static constexpr int EC = helm_quad_ec(NQ, R::EC), WPB = R::WPB, BM = R::BM, MW = R::MW > 2 ? 2 : R::MW;
    static constexpr int KM = R::KM, MF = R::MF | 8;
};

template <int DIM, int NQ, typename T, class X> static int go_helm(const ArgsT<DIM, T> &a, const X &x, hipStream_t s)
{
    using C = typename std::conditional<DIM == 3, HelmHexCfg<NQ, T>, HelmQuadCfg<NQ, T>>::type;
    return HelmFamily<X>::has_mass(x)
               ? launch_helm_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, true, T>(a, x, s)
               : launch_helm_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, false, T>(a, x, s);
}

#define SF_HELM_HEX_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8)
#define SF_HELM_QUAD_CASES(F) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11) F(12) F(13) F(14) F(15) F(16)

// The order switch of every family on this table, written once: f(std::integral_constant<int, NQ>()) for the order's
// case, SF_ENOTBUILT for an order without one.
template <int DIM, class Fn> static int with_helm_order(unsigned nq, Fn &&f)
{
#define SF_CASE(N) case N: return f(std::integral_constant<int, N>());
    if constexpr (DIM == 3)
        switch (nq)
        {
            SF_HELM_HEX_CASES(SF_CASE)
        }
    else
        switch (nq)
        {
            SF_HELM_QUAD_CASES(SF_CASE)
        }
#undef SF_CASE
    return SF_ENOTBUILT;
}

// whether the order has a case: what the *_wave_built() predicates of the families on this table answer
static inline bool helm_order_built(int dim, unsigned nq)
{
    const auto has_case = [](auto) { return (int)SF_OK; };
    return (dim == 3 ? with_helm_order<3>(nq, has_case) : with_helm_order<2>(nq, has_case)) == SF_OK;
}

// SF_ENOTBUILT when the order has no instantiation (helmholtz_wave_built() / affine_wave_built())
template <int DIM, typename T, class X>
static int launch_helm_wave(unsigned nq, const ArgsT<DIM, T> &a, const X &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_helm<DIM, decltype(n)::value, T>(a, x, s); });
}

// instantiated for double in helmholtz.hip and for float in helmholtz_f32.hip
template <int DIM, typename T>
int launch_helmholtz_wave(unsigned nq, const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s)
{
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}

} // namespace sf
