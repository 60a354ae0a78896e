// tensor_quad.hip -- the sf_tensor_* wave kernels of the table (tensor_launch.h), 2D, double.
#include "tensor_launch.h"

namespace sf
{
template int launch_tensor_wave<2, double>(const unsigned (&)[3], const unsigned (&)[3], int, const QuadArgs &, hipStream_t);
} // namespace sf
