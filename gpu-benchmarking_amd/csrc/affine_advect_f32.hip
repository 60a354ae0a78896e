// affine_advect_f32.hip -- fp32 instantiations of the affine advection kernels (affine_advect_wave.h) + nq dispatch;
// configuration in affine_advect_launch.h.  Same table of orders as affine_advect.hip (affine_advect_wave_built()).
#include "affine_advect_launch.h"

namespace sf
{

template int launch_affine_advect_wave<3, float>(unsigned, const HexArgsT<float> &, const AffineAdvectArgsT<float> &,
                                                 hipStream_t);
template int launch_affine_advect_wave<2, float>(unsigned, const QuadArgsT<float> &, const AffineAdvectArgsT<float> &,
                                                 hipStream_t);

} // namespace sf
