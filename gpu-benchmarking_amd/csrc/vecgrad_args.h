// vecgrad_args.h -- the entry points of the vector-gradient family (sf_vecgrad_*) between the C ABI (capi.hip) and the
// translation units that define them; the part of sf_dispatch.h that belongs to this family, kept in a header of its own
// so that no other translation unit sees a changed header (as advect_args.h).
// vecgrad.hip / vecgrad_f32.hip: the wave kernels of vecgrad_wave.h, the Helmholtz table (3D nq 2..8, 2D nq 2..16);
// vecgrad_generic.hip: any extents up to 12 per direction in 3D and 32 in 2D.
#pragma once

#include "sf_dispatch.h"

namespace sf
{

// What the family takes beyond the bases (b0 .. b2 and nelmt of the BwdTrans arguments; `in` and `out` are not used): the
// derivative matrices, the d*d planes of the inverse Jacobian, the d fields of modes, and the outputs -- the d*d planes
// of the gradient, the divergence and the d(d-1)/2 planes of the curl (2D: curl0 only).  An output that is null is not
// written.
template <typename T> struct VecgradArgsT
{
    const T *d0, *d1, *d2, *df;
    const T *in0, *in1, *in2;
    T *grad, *div, *curl0, *curl1, *curl2;
};
template <int DIM, typename T>
int launch_vecgrad_wave(unsigned nq, const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_vecgrad_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const VecgradArgsT<T> &x, hipStream_t s);
bool vecgrad_wave_built(int dim, unsigned nq);
bool vecgrad_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);

} // namespace sf
