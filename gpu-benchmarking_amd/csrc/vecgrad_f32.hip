// vecgrad_f32.hip -- fp32 instantiations of the vector-gradient kernels (vecgrad_wave.h) + nq dispatch; configuration in
// vecgrad_launch.h.  Same table of orders as vecgrad.hip (vecgrad_wave_built()).
#include "vecgrad_launch.h"

namespace sf
{

template int launch_vecgrad_wave<3, float>(unsigned, const HexArgsT<float> &, const VecgradArgsT<float> &, hipStream_t);
template int launch_vecgrad_wave<2, float>(unsigned, const QuadArgsT<float> &, const VecgradArgsT<float> &, hipStream_t);

} // namespace sf
