// geom_args.h -- the entry points of the geometric-factor family (sf_geom_* / sf_geom_affine_*) between the C ABI
// (capi.hip) and the translation units that define them; the part of sf_dispatch.h that belongs to this family, kept in
// a header of its own so that no other translation unit sees a changed header.
// geom.hip / geom_f32.hip: the wave kernels of geom_wave.h, the Helmholtz table (3D nq 2..8, 2D nq 2..16);
// geom_generic.hip: any extents up to 12 per direction in 3D and 32 in 2D, and the affine kernel.
#pragma once

#include "sf_dispatch.h"

namespace sf
{

// What the family takes beyond the bases (b0 .. b2 and nelmt of the BwdTrans arguments; `in` and `out` are not used): the
// derivative matrices, the one-dimensional quadrature weights (read only when w or g is written), the d coordinate
// streams of modes and the four outputs, each null when it is not asked for.
template <typename T> struct GeomArgsT
{
    const T *d0, *d1, *d2, *qw0, *qw1, *qw2;
    const T *x0, *x1, *x2;
    T *df, *w, *g, *detj;
};
template <int DIM, typename T>
int launch_geom_wave(unsigned nq, const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_geom_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s);
// the same formulas at the point (0, 0, 0) of every element: df -> dfe[e][c], w -> je[e] = |det|, g -> ge[e][c]; qw_d
// and detj are not used
template <int DIM, typename T>
int launch_geom_affine(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const GeomArgsT<T> &x, hipStream_t s);
bool geom_wave_built(int dim, unsigned nq);
bool geom_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);

} // namespace sf
