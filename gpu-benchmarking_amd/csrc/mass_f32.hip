// mass_f32.hip -- fp32 instantiations of the fused mass kernels (mass_wave.h) + nq dispatch; configuration in
// mass_launch.h.  Same table of orders as mass.hip (mass_wave_built()).
#include "mass_launch.h"

namespace sf
{

template int launch_mass_wave<3, float>(unsigned, const HexArgsT<float> &, const float *, hipStream_t);
template int launch_mass_wave<2, float>(unsigned, const QuadArgsT<float> &, const float *, hipStream_t);

} // namespace sf
