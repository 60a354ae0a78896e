// iprodderiv_f32.hip -- fp32 instantiations of the IProductWRTDerivBase kernels (iprodderiv_wave.h) + nq dispatch;
// configuration in iprodderiv_launch.h.  Same table of orders as iprodderiv.hip (iprodderiv_wave_built()).
#include "iprodderiv_launch.h"

namespace sf
{

template int launch_iprodderiv_wave<3, float>(unsigned, const HexArgsT<float> &, const IprodDerivArgsT<float> &,
                                              hipStream_t);
template int launch_iprodderiv_wave<2, float>(unsigned, const QuadArgsT<float> &, const IprodDerivArgsT<float> &,
                                              hipStream_t);

} // namespace sf
