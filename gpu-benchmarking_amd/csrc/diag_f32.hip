// diag_f32.hip -- fp32 instantiations of the Helmholtz-diagonal kernels (diag_wave.h) + nq dispatch; configuration in
// diag_launch.h.  Same table of orders as diag.hip (diag_wave_built()).
#include "diag_launch.h"

namespace sf
{

template int launch_diag_wave<3, float>(unsigned, const HexArgsT<float> &, const DiagArgsT<float> &, hipStream_t);
template int launch_diag_wave<2, float>(unsigned, const QuadArgsT<float> &, const DiagArgsT<float> &, hipStream_t);

} // namespace sf
