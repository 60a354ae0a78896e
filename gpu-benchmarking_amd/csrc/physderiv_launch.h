// physderiv_launch.h -- the fused BwdTrans + gradient kernels (physderiv_wave.h) as a family of the launcher of
// helmholtz_launch.h, shared by the fp64 (physderiv.hip) and fp32 (physderiv_f32.hip) translation units.
//
// The table and the configuration of an order are those of the Helmholtz kernels (HelmHexCfg / HelmQuadCfg of
// helmholtz_launch.h): 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with and without df (HASDF;
// the launcher's "mass term" switch).  The kernels keep the geometry of the Helmholtz front half and a ring of 2 x 9
// (2D: 2 x 4) planes where Helmholtz holds 2 x 7 (2 x 4); no row has been changed, because no measurement stands behind
// a change yet.  3D nq 9..11 are NOT in the table: AUTO sends them to the any-extent kernel of physderiv_generic.hip,
// SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "helmholtz_launch.h"
#include "physderiv_wave.h"

namespace sf
{

// the gradient family of the launcher of helmholtz_launch.h
template <typename T> struct HelmFamily<PhysDerivArgsT<T>>
{
    static bool has_mass(const PhysDerivArgsT<T> &x) { return x.df != nullptr; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x,
                      hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(hex_physderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASDF, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.df, a.in,
                                                 x.out0, x.out1, x.out2, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(quad_physderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASDF, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, x.d0, x.d1, x.df, a.in, x.out0,
                                                 x.out1, a.nelmt);
    }
};

// SF_ENOTBUILT when the order has no instantiation (physderiv_wave_built()); instantiated for double in physderiv.hip and
// for float in physderiv_f32.hip
template <int DIM, typename T>
int launch_physderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x, hipStream_t s)
{
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}

} // namespace sf
