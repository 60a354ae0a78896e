// helmholtz_f32.hip -- fp32 instantiations of the fused Helmholtz kernels (helmholtz_wave.h) + nq dispatch; configuration
// in helmholtz_launch.h.  Same table of orders as helmholtz.hip (helmholtz_wave_built()).
#include "helmholtz_launch.h"

namespace sf
{

template int launch_helmholtz_wave<3, float>(unsigned, const HexArgsT<float> &, const HelmArgsT<float> &, hipStream_t);
template int launch_helmholtz_wave<2, float>(unsigned, const QuadArgsT<float> &, const HelmArgsT<float> &, hipStream_t);

} // namespace sf
