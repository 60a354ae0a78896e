// affine_deriv.hip -- fp64 instantiations of the affine-element gradient and weak-divergence kernels
// (affine_deriv_wave.h) + nq dispatch; configuration in affine_deriv_launch.h.  The fp32 instantiations are in
// affine_deriv_f32.hip (the two halves build in parallel).
#include "affine_deriv_launch.h"

namespace sf
{

template int launch_affine_physderiv_wave<3, double>(unsigned, const HexArgs &, const AffinePhysDerivArgsT<double> &,
                                                     hipStream_t);
template int launch_affine_physderiv_wave<2, double>(unsigned, const QuadArgs &, const AffinePhysDerivArgsT<double> &,
                                                     hipStream_t);
template int launch_affine_iprodderiv_wave<3, double>(unsigned, const HexArgs &, const AffineIprodDerivArgsT<double> &,
                                                      hipStream_t);
template int launch_affine_iprodderiv_wave<2, double>(unsigned, const QuadArgs &, const AffineIprodDerivArgsT<double> &,
                                                      hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool affine_deriv_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
