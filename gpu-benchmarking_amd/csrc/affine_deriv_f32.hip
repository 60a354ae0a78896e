// affine_deriv_f32.hip -- fp32 instantiations of the affine-element gradient and weak-divergence kernels
// (affine_deriv_wave.h) + nq dispatch; configuration in affine_deriv_launch.h.  Same table of orders as affine_deriv.hip
// (affine_deriv_wave_built()).
#include "affine_deriv_launch.h"

namespace sf
{

template int launch_affine_physderiv_wave<3, float>(unsigned, const HexArgsT<float> &, const AffinePhysDerivArgsT<float> &,
                                                    hipStream_t);
template int launch_affine_physderiv_wave<2, float>(unsigned, const QuadArgsT<float> &, const AffinePhysDerivArgsT<float> &,
                                                    hipStream_t);
template int launch_affine_iprodderiv_wave<3, float>(unsigned, const HexArgsT<float> &,
                                                     const AffineIprodDerivArgsT<float> &, hipStream_t);
template int launch_affine_iprodderiv_wave<2, float>(unsigned, const QuadArgsT<float> &,
                                                     const AffineIprodDerivArgsT<float> &, hipStream_t);

} // namespace sf
