// affine.hip -- fp64 instantiations of the affine Helmholtz kernels (affine_wave.h) + nq dispatch; configuration in
// affine_launch.h.  The fp32 instantiations are in affine_f32.hip (the two halves build in parallel).
#include "affine_launch.h"

namespace sf
{

template int launch_affine_wave<3, double>(unsigned, const HexArgs &, const AffineArgsT<double> &, hipStream_t);
template int launch_affine_wave<2, double>(unsigned, const QuadArgs &, const AffineArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool affine_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
