// affine_f32.hip -- fp32 instantiations of the affine Helmholtz kernels (affine_wave.h) + nq dispatch; configuration in
// affine_launch.h.  Same table of orders as affine.hip (affine_wave_built()).
#include "affine_launch.h"

namespace sf
{

template int launch_affine_wave<3, float>(unsigned, const HexArgsT<float> &, const AffineArgsT<float> &, hipStream_t);
template int launch_affine_wave<2, float>(unsigned, const QuadArgsT<float> &, const AffineArgsT<float> &, hipStream_t);

} // namespace sf
