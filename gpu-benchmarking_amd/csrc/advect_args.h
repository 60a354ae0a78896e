// advect_args.h -- the entry points of the advection family (sf_advect_*) between the C ABI (capi.hip) and the
// translation units that define them; the part of sf_dispatch.h that belongs to this family, kept in a header of its own
// so that no other translation unit sees a changed header (as geom_args.h).
// advect.hip / advect_f32.hip: the wave kernels of advect_wave.h, the Helmholtz table (3D nq 2..8, 2D nq 2..16);
// advect_generic.hip: any extents up to 12 per direction in 3D and 32 in 2D.
#pragma once

#include "sf_dispatch.h"

namespace sf
{

// What the family takes beyond the bases (b0 .. b2 and nelmt of the BwdTrans arguments; `in` and `out` are not used): the
// derivative matrices, the d*d planes of the inverse Jacobian, the weight plane, the d planes of the advecting velocity,
// and nf = 1 or d fields of modes in and out (in_a / out_a with a >= nf are not looked at).
template <typename T> struct AdvectArgsT
{
    const T *d0, *d1, *d2, *df, *w;
    const T *c0, *c1, *c2;
    const T *in0, *in1, *in2;
    T *out0, *out1, *out2;
    int nf;
};
template <int DIM, typename T>
int launch_advect_wave(unsigned nq, const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_advect_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AdvectArgsT<T> &x, hipStream_t s);
bool advect_wave_built(int dim, unsigned nq);
bool advect_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);

// The LDS classes of the any-extent advection kernels (advect_generic.hip, affine_advect_generic.hip) in scalars: two
// point images.  3D 12^3: 3456; 2D 32^2: 2048, the small class.
constexpr int kAdvSmallCap = 2048, kAdvLargeCap = 2 * 12 * 12 * 12;
// LDS the extents need: two point images
inline unsigned advect_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return 2 * nq0 * nq1 * (dim == 3 ? nq2 : 1);
}

} // namespace sf
