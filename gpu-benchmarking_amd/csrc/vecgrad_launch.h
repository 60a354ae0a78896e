// vecgrad_launch.h -- the vector-gradient kernels (vecgrad_wave.h) behind the chunked launch and the order cases of
// helmholtz_launch.h, shared by the fp64 (vecgrad.hip) and fp32 (vecgrad_f32.hip) translation units.
//
// The table is that of the Helmholtz kernels: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float: 44
// instantiations.  The configuration of an order is its row of advect_launch.h with d fields (AdvectCfg: the row of
// GeomCfg, one element per chunk at fp32 3D nq 8, the waves per workgroup fitted to the slab of GeomGeom): the slab, the
// d register pencils and the front are those of that kernel, the ring is lighter (d*d values per slice where it holds
// d*d + d + 1).  No row is tuned; the measurements are in DESIGN s4.22.
// Output masks.  One instantiation per order and scalar type, all outputs (kVecAll): the kernel's null checks keep the
// planes that were not asked for unwritten.  A narrower instantiation (divergence and curl without the d*d stores of
// grad) holds the same pencils, ring and slab, which set the registers and the LDS of a row
// (profiles/r21/vecgrad_kernel_resources.log): it would not buy occupancy and is not built.
#pragma once

#include "advect_launch.h"
#include "vecgrad_args.h"
#include "vecgrad_wave.h"

namespace sf
{

template <int DIM, int NQ, typename T> struct VecgradCfg : AdvectCfg<DIM, NQ, DIM, T>
{
};

// the occupancy cache is one per kernel instantiation
template <int DIM, int NQ, int MASK, typename T>
static int launch_vecgrad_k(const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s)
{
    using C = VecgradCfg<DIM, NQ, T>;
    static OccCache cache = {};
    constexpr size_t lds = geom_lds_bytes<NQ, C::EC, DIM, C::WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(C::KM > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<C::WPB, C::EC, C::KM>(
            hex_vecgrad_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, MASK, T>, cache, lds, 0, s, a.nelmt,
            a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.df, x.in0, x.in1, x.in2, x.grad, x.div, x.curl0, x.curl1, x.curl2,
            a.nelmt);
    else
        return launch_chunked<C::WPB, C::EC, C::KM>(
            quad_vecgrad_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, MASK, T>, cache, lds, 0, s, a.nelmt,
            a.b0, a.b1, x.d0, x.d1, x.df, x.in0, x.in1, x.grad, x.div, x.curl0, a.nelmt);
}

// the built instantiation that a request runs: the smallest superset of its outputs (one is built: all of them)
template <int DIM, int NQ, typename T>
static int go_vecgrad(const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s)
{
    return launch_vecgrad_k<DIM, NQ, kVecAll, T>(a, x, s);
}

// SF_ENOTBUILT when the order has no instantiation (vecgrad_wave_built()); instantiated for double in vecgrad.hip and
// for float in vecgrad_f32.hip
template <int DIM, typename T>
int launch_vecgrad_wave(unsigned nq, const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_vecgrad<DIM, decltype(n)::value, T>(a, x, s); });
}

} // namespace sf
