// iprodderiv_launch.h -- the IProductWRTDerivBase kernels (iprodderiv_wave.h) as two families of the launcher of
// helmholtz_launch.h, shared by the fp64 (iprodderiv.hip) and fp32 (iprodderiv_f32.hip) translation units.
//
// The table and the configuration of an order are those of the Helmholtz kernels (HelmHexCfg / HelmQuadCfg of
// helmholtz_launch.h): 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float.  The launcher carries one boolean,
// which is HASDF here (the launcher's "mass term" switch); HASW is chosen by the argument struct: IprodDerivArgsT<T>
// names the kernels without the weight, IprodDerivWArgsT<T> those with it.  22 orders x {double, float} x HASDF x HASW
// = 176 instantiations; no row's EC has been overridden (every instantiation builds without scratch or spills at the
// Helmholtz row's EC: tests/test_iprodderiv_cpu.py::test_wave_instantiations_use_no_scratch).  3D nq 9..11 are NOT in
// the table: AUTO sends them to the any-extent kernel of iprodderiv_generic.hip, SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "helmholtz_launch.h"
#include "iprodderiv_wave.h"

namespace sf
{

template <bool HASW, class X, typename T> struct IprodDerivFamily
{
    static bool has_mass(const X &x) { return x.df != nullptr; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASDF>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const X &x, hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(
                hex_iprodderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASDF, HASW, T>, cache, lds, 0, s, a.nelmt,
                a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.df, x.w, x.in0, x.in1, x.in2, a.out, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(
                quad_iprodderiv_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASDF, HASW, T>, cache, lds, 0, s, a.nelmt,
                a.b0, a.b1, x.d0, x.d1, x.df, x.w, x.in0, x.in1, a.out, a.nelmt);
    }
};
// the two families of the launcher of helmholtz_launch.h: without and with the weight
template <typename T> struct HelmFamily<IprodDerivArgsT<T>> : IprodDerivFamily<false, IprodDerivArgsT<T>, T>
{
};
template <typename T> struct HelmFamily<IprodDerivWArgsT<T>> : IprodDerivFamily<true, IprodDerivWArgsT<T>, T>
{
};

// SF_ENOTBUILT when the order has no instantiation (iprodderiv_wave_built()); instantiated for double in iprodderiv.hip
// and for float in iprodderiv_f32.hip
template <int DIM, typename T>
int launch_iprodderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const IprodDerivArgsT<T> &x, hipStream_t s)
{
    if (x.w != nullptr)
        return launch_helm_wave<DIM, T>(nq, a, IprodDerivWArgsT<T>{x}, s);
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}

} // namespace sf
