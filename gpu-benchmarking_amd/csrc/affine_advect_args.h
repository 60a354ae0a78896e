// affine_advect_args.h -- the entry points of the affine advection family (sf_aff_advect_*) between the C ABI (capi.hip)
// and the translation units that define them; the part of sf_dispatch.h that belongs to this family, kept in a header of
// its own so that no other translation unit sees a changed header (as advect_args.h).
// affine_advect.hip / affine_advect_f32.hip: the wave kernels of affine_advect_wave.h, the Helmholtz table (3D nq 2..8,
// 2D nq 2..16); affine_advect_generic.hip: any extents up to 12 per direction in 3D and 32 in 2D.
#pragma once

#include "sf_dispatch.h"

namespace sf
{

// What the family takes beyond the bases (b0 .. b2 and nelmt of the BwdTrans arguments; `in` and `out` are not used): the
// derivative matrices, the one-dimensional quadrature weights and je[e] (all null when je is: no weight), the d*d
// constants of the inverse Jacobian per element, the d planes of the advecting velocity, and nf = 1 or d fields of modes
// in and out (in_a / out_a with a >= nf are not looked at).
template <typename T> struct AffineAdvectArgsT
{
    const T *d0, *d1, *d2;
    const T *qw0, *qw1, *qw2;
    const T *dfe, *je;
    const T *c0, *c1, *c2;
    const T *in0, *in1, *in2;
    T *out0, *out1, *out2;
    int nf;
};
template <int DIM, typename T>
int launch_affine_advect_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_affine_advect_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineAdvectArgsT<T> &x,
                                 hipStream_t s);
bool affine_advect_wave_built(int dim, unsigned nq);
bool affine_advect_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);

} // namespace sf
