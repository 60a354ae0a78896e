// affine_launch.h -- the affine Helmholtz kernels (affine_wave.h) as a family of the launcher of helmholtz_launch.h,
// shared by the fp64 (affine.hip) and fp32 (affine_f32.hip) translation units.
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

// the affine family of the launcher of helmholtz_launch.h
template <typename T> struct HelmFamily<AffineArgsT<T>>
{
    static bool has_mass(const AffineArgsT<T> &x) { return x.je != nullptr; }
    template <int DIM, int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASJ>
    static int launch(std::atomic<int> *cache, size_t lds, const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
    {
        if constexpr (DIM == 3)
            return launch_chunked<WPB, EC, KMAP>(hex_affine_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASJ, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.b2, x.d0, x.d1, x.d2, x.qw0, x.qw1,
                                                 x.qw2, x.ge, x.je, x.lam, a.in, a.out, a.nelmt);
        else
            return launch_chunked<WPB, EC, KMAP>(quad_affine_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, MEMF, HASJ, T>,
                                                 cache, lds, 0, s, a.nelmt, a.b0, a.b1, x.d0, x.d1, x.qw0, x.qw1, x.ge, x.je,
                                                 x.lam, a.in, a.out, a.nelmt);
    }
};

// SF_ENOTBUILT when the order has no instantiation (affine_wave_built()); instantiated for double in affine.hip and for
// float in affine_f32.hip
template <int DIM, typename T>
int launch_affine_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
    return launch_helm_wave<DIM, T>(nq, a, x, s);
}

} // namespace sf
