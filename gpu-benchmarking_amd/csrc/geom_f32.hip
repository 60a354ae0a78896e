// geom_f32.hip -- fp32 instantiations of the geometric-factor kernels (geom_wave.h) + nq dispatch; configuration in
// geom_launch.h.  Same table of orders as geom.hip (geom_wave_built()).
#include "geom_launch.h"

namespace sf
{

template int launch_geom_wave<3, float>(unsigned, const HexArgsT<float> &, const GeomArgsT<float> &, hipStream_t);
template int launch_geom_wave<2, float>(unsigned, const QuadArgsT<float> &, const GeomArgsT<float> &, hipStream_t);

} // namespace sf
