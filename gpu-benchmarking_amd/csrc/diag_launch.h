// diag_launch.h -- launchers and the per-order configuration of the Helmholtz-diagonal kernels (diag_wave.h), shared by the
// fp64 (diag.hip) and fp32 (diag_f32.hip) translation units.
//
// The configuration of an order is its Helmholtz row (helmholtz_launch.h: HelmHexCfg / HelmQuadCfg -- the BwdTrans row of
// wave_table.h with at most 128 point columns per chunk, MINW <= 2 and the output through the line-aligned LDS stream),
// unchanged: the kernel streams the same planes with the same lane -> point mapping and leaves through the same back.
// What it keeps alive is less than the Helmholtz kernel's (one image of the first contraction, the three images keyed by
// the direction-0 table, the ring of plane pencils), so every row of that table fits without scratch or spills.
// The table: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with and without the mass term (HASW).
// 3D nq 9..11 are NOT in the table, as for the operator itself: AUTO sends them to the any-extent kernel of
// diag_generic.hip, SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "diag_wave.h"
#include "helmholtz_launch.h"

namespace sf
{

// the occupancy cache is one per kernel instantiation
template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T>
static int launch_diag_k(const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s)
{
    static OccCache cache = {};
    constexpr size_t lds = diag_lds_bytes<NQ, EC, DIM, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(KMAP > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<WPB, EC, KMAP>(hex_diag_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>, cache, lds,
                                             0, s, a.nelmt, a.b0, a.b1, a.b2, x.g, x.w, x.lam, a.out, a.nelmt);
    else
        return launch_chunked<WPB, EC, KMAP>(quad_diag_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>, cache, lds,
                                             0, s, a.nelmt, a.b0, a.b1, x.g, x.w, x.lam, a.out, a.nelmt);
}

template <int DIM, int NQ, typename T> static int go_diag(const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s)
{
    using C = typename std::conditional<DIM == 3, HelmHexCfg<NQ, T>, HelmQuadCfg<NQ, T>>::type;
    return x.w != nullptr ? launch_diag_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, true, T>(a, x, s)
                          : launch_diag_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, false, T>(a, x, s);
}

// instantiated for double in diag.hip and for float in diag_f32.hip; SF_ENOTBUILT when the order has no instantiation
// (diag_wave_built())
template <int DIM, typename T>
int launch_diag_wave(unsigned nq, const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_diag<DIM, decltype(n)::value, T>(a, x, s); });
}

} // namespace sf
