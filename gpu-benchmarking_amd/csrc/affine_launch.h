// affine_launch.h -- launchers of the affine Helmholtz kernels (affine_wave.h), shared by the fp64 (affine.hip) and fp32
// (affine_f32.hip) translation units.
//
// The table and the configuration of an order are those of the Helmholtz kernels (HelmHexCfg / HelmQuadCfg of
// helmholtz_launch.h): 3D isotropic nq 2..8, 2D isotropic nq 2..16, double and float, each with and without the mass
// term (HASJ).  The kernels keep the same geometry and fewer registers alive (the constants of an element instead of
// the metric ring); no row has been changed, because no measurement stands behind a change yet.  3D nq 9..11 are NOT in
// the table: AUTO sends them to the any-extent kernel of affine_generic.hip, SF_VARIANT_WAVE answers SF_ENOTBUILT.
#pragma once

#include "affine_wave.h"
#include "helmholtz_launch.h"

namespace sf
{

template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASJ, typename T>
static int launch_affine_k(const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
    static OccCache cache = {};
    constexpr size_t lds = helmholtz_lds_bytes<NQ, EC, DIM, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(KMAP > 0, "short-lived waves: the grid covers the batch");
    if constexpr (DIM == 3)
        return launch_chunked<WPB, EC, KMAP>(hex_affine_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASJ, T>, cache,
                                             lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.qw0, x.qw1, x.qw2,
                                             x.ge, x.je, x.lam, a.in, a.out, a.nelmt);
    else
        return launch_chunked<WPB, EC, KMAP>(quad_affine_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASJ, T>, cache,
                                             lds, 0, s, a.nelmt, a.b0, a.b1, x.d0, x.d1, x.qw0, x.qw1, x.ge, x.je, x.lam,
                                             a.in, a.out, a.nelmt);
}

template <int DIM, int NQ, typename T>
static int go_affine(const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
    using C = typename std::conditional<DIM == 3, HelmHexCfg<NQ, T>, HelmQuadCfg<NQ, T>>::type;
    return x.je ? launch_affine_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, true, T>(a, x, s)
                : launch_affine_k<DIM, NQ, C::EC, C::WPB, C::BM, C::MW, C::KM, C::MF, false, T>(a, x, s);
}

// SF_ENOTBUILT when the order has no instantiation (affine_wave_built()); instantiated for double in affine.hip and for
// float in affine_f32.hip
template <int DIM, typename T>
int launch_affine_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
#define SF_CASE(N) case N: return go_affine<DIM, N, T>(a, x, s);
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

} // namespace sf
