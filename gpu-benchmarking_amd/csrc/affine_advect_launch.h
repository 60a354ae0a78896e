// affine_advect_launch.h -- the affine advection kernels (affine_advect_wave.h) behind the chunked launch and the order
// cases of helmholtz_launch.h, shared by the fp64 (affine_advect.hip) and fp32 (affine_advect_f32.hip) translation units.
//
// The table is that of the Helmholtz kernels: 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with one
// field and with d, each with and without the weight: 176 instantiations.  The configuration of an order is its row of
// advect_launch.h (AdvectCfg); the LDS slab is that of the deformed kernel.  No row has been measured yet.
#pragma once

#include "advect_launch.h"
#include "affine_advect_args.h"
#include "affine_advect_wave.h"

namespace sf
{

// AdvectCfg as it stands, the one-element chunk of fp32 3D nq 8 with three fields included: with the row's two elements
// the affine kernel no longer spills (202 VGPRs, 2 waves per workgroup, occupancy 2) but one element per chunk is one
// full pass at 103 VGPRs, 4 waves per workgroup and occupancy 4, and which of the two is faster has not been measured.
template <int DIM, int NQ, int NF, typename T> struct AffineAdvectCfg : AdvectCfg<DIM, NQ, NF, T>
{
};

// the occupancy cache is one per kernel instantiation
template <int DIM, int NQ, int NF, bool HASW, typename T>
static int launch_affine_advect_k(const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x, hipStream_t s)
{
    using C = AffineAdvectCfg<DIM, NQ, NF, T>;
    static OccCache cache = {};
    constexpr size_t lds = advect_lds_bytes<NQ, C::EC, DIM, NF, C::WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(C::KM > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<C::WPB, C::EC, C::KM>(
            hex_affine_advect_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, NF, HASW, T>, cache, lds, 0, s,
            a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2, x.dfe, x.je, x.c0, x.c1, x.c2, x.in0, x.in1,
            x.in2, x.out0, x.out1, x.out2, a.nelmt);
    else
        return launch_chunked<C::WPB, C::EC, C::KM>(
            quad_affine_advect_wave_kernel<NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, NF, HASW, T>, cache, lds, 0, s,
            a.nelmt, a.b0, a.b1, x.d0, x.d1, x.qw0, x.qw1, x.dfe, x.je, x.c0, x.c1, x.in0, x.in1, x.out0, x.out1, a.nelmt);
}

template <int DIM, int NQ, typename T>
static int go_affine_advect(const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x, hipStream_t s)
{
    if (x.je)
        return x.nf == 1 ? launch_affine_advect_k<DIM, NQ, 1, true, T>(a, x, s)
                         : launch_affine_advect_k<DIM, NQ, DIM, true, T>(a, x, s);
    return x.nf == 1 ? launch_affine_advect_k<DIM, NQ, 1, false, T>(a, x, s)
                     : launch_affine_advect_k<DIM, NQ, DIM, false, T>(a, x, s);
}

// SF_ENOTBUILT when the order has no instantiation (affine_advect_wave_built()); instantiated for double in
// affine_advect.hip and for float in affine_advect_f32.hip
template <int DIM, typename T>
int launch_affine_advect_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x, hipStream_t s)
{
    return with_helm_order<DIM>(nq, [&](auto n) { return go_affine_advect<DIM, decltype(n)::value, T>(a, x, s); });
}

} // namespace sf
