// geom_launch.h -- the geometric-factor kernels (geom_wave.h) behind the chunked launch and the order cases of
// helmholtz_launch.h, shared by the fp64 (geom.hip) and fp32 (geom_f32.hip) translation units.
//
// The table is that of the Helmholtz kernels: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float.  The
// configuration of an order starts from its Helmholtz row (HelmHexCfg / HelmQuadCfg: EC, basis delivery, MINW, memory
// flags).  Its own: the LDS need -- the Helmholtz slab plus four (2D: one) kept point images per wave, GeomGeom -- and with
// it the waves per workgroup: the row's WPB, halved until the workgroup's slabs fit kGeomLdsBudget, so that two
// workgroups of every order share a CU's 160 KiB.  No row has been measured yet.
// Output masks.  Four instantiations per order and scalar type: all four outputs, df only, w only, g and w.  Any other
// request runs the smallest of these that contains it (in practice: all four) and the kernel's null checks keep the
// planes that were not asked for unwritten.
#pragma once

#include "geom_args.h"
#include "geom_wave.h"
#include "helmholtz_launch.h"

namespace sf
{

constexpr size_t kGeomLdsBudget = 80 * 1024;

constexpr int geom_wpb(int row_wpb, size_t slab_bytes)
{
    int wpb = row_wpb;
    while (wpb > 1 && (size_t)wpb * slab_bytes > kGeomLdsBudget)
        wpb /= 2;
    return wpb;
}

template <int DIM, int NQ, typename T> struct GeomCfg
{
    using R = typename std::conditional<DIM == 3, HelmHexCfg<NQ, T>, HelmQuadCfg<NQ, T>>::type;
    // fp64 2D nq 15 / 16: twelve pointer arguments beside the 64 SGPRs of the row's 16-column basis ring spill two to six
    // SGPRs; the 8-column ring (the same sums in the same order) does not
    static constexpr int BM = (DIM == 2 && sizeof(T) == 8 && NQ >= 15) ? (int)BASIS_SMEM_COLS : R::BM;
    static constexpr int EC = R::EC, MW = R::MW, KM = R::KM, MF = R::MF;
    static constexpr int WPB = geom_wpb(R::WPB, sizeof(T) * (size_t)GeomGeom<NQ, EC, DIM, T>::SLAB);
};

// the occupancy cache is one per kernel instantiation
template <int DIM, int NQ, int MASK, typename T>
static int launch_geom_k(const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    using C = GeomCfg<DIM, NQ, T>;
    static OccCache cache = {};
    constexpr size_t lds = geom_lds_bytes<NQ, C::EC, DIM, C::WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(C::KM > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<C::WPB, C::EC, C::KM>(
            hex_geom_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, MASK, T>, cache, lds, 0, s, a.nelmt, a.b0,
            a.b1, a.b2, x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.x0, x.x1, x.x2, x.df, x.w, x.g, x.detj, a.nelmt);
    else
        return launch_chunked<C::WPB, C::EC, C::KM>(
            quad_geom_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, MASK, T>, cache, lds, 0, s, a.nelmt, a.b0,
            a.b1, x.d0, x.d1, x.qw0, x.qw1, x.x0, x.x1, x.df, x.w, x.g, x.detj, a.nelmt);
}

// the built instantiation that a request runs: the smallest superset of its outputs
template <int DIM, int NQ, typename T> static int go_geom(const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    const int want = (x.df ? kGeomDf : 0) | (x.w ? kGeomW : 0) | (x.g ? kGeomG : 0) | (x.detj ? kGeomDet : 0);
    if (want == kGeomDf)
        return launch_geom_k<DIM, NQ, kGeomDf, T>(a, x, s);
    if (want == kGeomW)
        return launch_geom_k<DIM, NQ, kGeomW, T>(a, x, s);
    if ((want & ~(kGeomG | kGeomW)) == 0)
        return launch_geom_k<DIM, NQ, kGeomG | kGeomW, T>(a, x, s);
    return launch_geom_k<DIM, NQ, kGeomAll, T>(a, x, s);
}

// SF_ENOTBUILT when the order has no instantiation (geom_wave_built()); instantiated for double in geom.hip and for
// float in geom_f32.hip
template <int DIM, typename T>
int launch_geom_wave(unsigned nq, const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_geom<DIM, decltype(n)::value, T>(a, x, s); });
}

} // namespace sf
