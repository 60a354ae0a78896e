// physderiv_f32.hip -- fp32 instantiations of the fused BwdTrans + gradient kernels (physderiv_wave.h) + nq dispatch;
// configuration in physderiv_launch.h.  Same table of orders as physderiv.hip (physderiv_wave_built()).
#include "physderiv_launch.h"

namespace sf
{

template int launch_physderiv_wave<3, float>(unsigned, const HexArgsT<float> &, const PhysDerivArgsT<float> &,
                                             hipStream_t);
template int launch_physderiv_wave<2, float>(unsigned, const QuadArgsT<float> &, const PhysDerivArgsT<float> &,
                                             hipStream_t);

} // namespace sf
