// advect_f32.hip -- fp32 instantiations of the advection kernels (advect_wave.h) + nq dispatch; configuration in
// advect_launch.h.  Same table of orders as advect.hip (advect_wave_built()).
#include "advect_launch.h"

namespace sf
{

template int launch_advect_wave<3, float>(unsigned, const HexArgsT<float> &, const AdvectArgsT<float> &, hipStream_t);
template int launch_advect_wave<2, float>(unsigned, const QuadArgsT<float> &, const AdvectArgsT<float> &, hipStream_t);

} // namespace sf
