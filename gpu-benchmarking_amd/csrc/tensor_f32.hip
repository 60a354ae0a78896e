// tensor_f32.hip -- the sf_tensor_* wave kernels of the table (tensor_launch.h), 3D, float.
#include "tensor_launch.h"

namespace sf
{
template int launch_tensor_wave<3, float>(const unsigned (&)[3], const unsigned (&)[3], int, const HexArgsT<float> &,
                                          hipStream_t);
} // namespace sf
