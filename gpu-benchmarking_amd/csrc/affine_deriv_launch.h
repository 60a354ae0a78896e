// affine_deriv_launch.h -- the affine-element gradient and weak-divergence kernels (affine_deriv_wave.h) as two families
// of the launcher of helmholtz_launch.h, shared by the fp64 (affine_deriv.hip) and fp32 (affine_deriv_f32.hip)
// translation units.
//
// The table and the configuration of an order are those of the Helmholtz kernels (HelmHexCfg / HelmQuadCfg of
// helmholtz_launch.h): 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float.  The launcher carries one boolean:
// the weak divergence takes it as HASW (je != null); the gradient has no switch (dfe is required) and names the same
// kernel for both values.  22 orders x {double, float} x (1 + 2) = 132 instantiations.  The kernels keep the geometry of
// their deformed counterparts and hold d*d (+ 1) constants per pass where those hold a ring of 2 d*d (+ 2) values; no
// row has been changed, because no measurement stands behind a change yet.  3D nq 9..11 are NOT in the table: AUTO sends
// them to the any-extent kernels of affine_deriv_generic.hip, SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "affine_deriv_wave.h"
#include "helmholtz_launch.h"

namespace sf
{

// the affine gradient family of the launcher of helmholtz_launch.h
template <typename T> struct HelmFamily<AffinePhysDerivArgsT<T>>
{
    static bool has_mass(const AffinePhysDerivArgsT<T> &) { return true; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const AffinePhysDerivArgsT<T> &x,
                      hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(hex_affine_physderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.dfe, a.in,
                                                 x.out0, x.out1, x.out2, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(quad_affine_physderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, x.d0, x.d1, x.dfe, a.in, x.out0,
                                                 x.out1, a.nelmt);
    }
};

// the affine weak-divergence family
template <typename T> struct HelmFamily<AffineIprodDerivArgsT<T>>
{
    static bool has_mass(const AffineIprodDerivArgsT<T> &x) { return x.je != nullptr; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const AffineIprodDerivArgsT<T> &x,
                      hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(
                hex_affine_iprodderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>, cache, lds, 0, s, a.nelmt,
                a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.dfe, x.je, x.in0, x.in1, x.in2, a.out, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(
                quad_affine_iprodderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASW, T>, cache, lds, 0, s, a.nelmt,
                a.b0, a.b1, x.d0, x.d1, x.qw0, x.qw1, x.dfe, x.je, x.in0, x.in1, a.out, a.nelmt);
    }
};

// SF_ENOTBUILT when the order has no instantiation (affine_deriv_wave_built()); instantiated for double in
// affine_deriv.hip and for float in affine_deriv_f32.hip
template <int DIM, typename T>
int launch_affine_physderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffinePhysDerivArgsT<T> &x, hipStream_t s)
{
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}
template <int DIM, typename T>
int launch_affine_iprodderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineIprodDerivArgsT<T> &x, hipStream_t s)
{
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}

} // namespace sf
