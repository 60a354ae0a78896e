// advect_launch.h -- the advection kernels (advect_wave.h) behind the chunked launch and the order cases of
// helmholtz_launch.h, shared by the fp64 (advect.hip) and fp32 (advect_f32.hip) translation units.
//
// The table is that of the Helmholtz kernels: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with one
// field and with d: 88 instantiations.  The configuration of an order is its row of geom_launch.h (GeomCfg: the
// Helmholtz row, the 8-column basis ring at fp64 2D nq 15 / 16 where the pointer arguments would spill SGPRs), with the
// waves per workgroup refitted to the slab of the instantiation: that of GeomGeom with d fields, of HelmGeom with one.
// No row has been measured yet.
#pragma once

#include "advect_args.h"
#include "advect_wave.h"
#include "geom_launch.h"

namespace sf
{

template <int DIM, int NQ, int NF, typename T> struct AdvectCfg : GeomCfg<DIM, NQ, T>
{
    using C = GeomCfg<DIM, NQ, T>;
    // fp32 3D nq 8 with three fields: the row's two elements (two passes: three pencils and the ring twice) spill two
    // VGPRs; one element is one full pass of the wave
    static constexpr int EC  = (DIM == 3 && NQ == 8 && NF == 3 && sizeof(T) == 4) ? 1 : C::EC;
    static constexpr int WPB = geom_wpb(C::R::WPB, sizeof(T) * (size_t)AdvectGeom<NQ, EC, DIM, NF, T>::SLAB);
};

// the occupancy cache is one per kernel instantiation
template <int DIM, int NQ, int NF, typename T>
static int launch_advect_k(const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s)
{
    using C = AdvectCfg<DIM, NQ, NF, T>;
    static OccCache cache = {};
    constexpr size_t lds = advect_lds_bytes<NQ, C::EC, DIM, NF, C::WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(C::KM > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<C::WPB, C::EC, C::KM>(
            hex_advect_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, NF, T>, cache, lds, 0, s, a.nelmt, a.b0,
            a.b1, a.b2, x.d0, x.d1, x.d2, x.df, x.w, x.c0, x.c1, x.c2, x.in0, x.in1, x.in2, x.out0, x.out1, x.out2,
            a.nelmt);
    else
        return launch_chunked<C::WPB, C::EC, C::KM>(
            quad_advect_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, NF, T>, cache, lds, 0, s, a.nelmt, a.b0,
            a.b1, x.d0, x.d1, x.df, x.w, x.c0, x.c1, x.in0, x.in1, x.out0, x.out1, a.nelmt);
}

template <int DIM, int NQ, typename T> static int go_advect(const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s)
{
    return x.nf == 1 ? launch_advect_k<DIM, NQ, 1, T>(a, x, s) : launch_advect_k<DIM, NQ, DIM, T>(a, x, s);
}

// SF_ENOTBUILT when the order has no instantiation (advect_wave_built()); instantiated for double in advect.hip and for
// float in advect_f32.hip
template <int DIM, typename T>
int launch_advect_wave(unsigned nq, const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_advect<DIM, decltype(n)::value, T>(a, x, s); });
}

} // namespace sf
