// tensor.hip -- the sf_tensor_* wave kernels of the table (tensor_launch.h), 3D, double; and which shapes the table holds.
#include "tensor_launch.h"

namespace sf
{

template int launch_tensor_wave<3, double>(const unsigned (&)[3], const unsigned (&)[3], int, const HexArgs &, hipStream_t);

bool tensor_wave_built(int dim, const unsigned (&ni)[3], const unsigned (&no)[3])
{
    for (int d = 1; d < dim; ++d)
        if (ni[d] != ni[0] || no[d] != no[0])
            return false;
    if (ni[0] > 63 || no[0] > 63)
        return false;
#define SF_CASE(I, O) case I * 64 + O: return true;
    if (dim == 3)
        switch (ni[0] * 64 + no[0])
        {
            SF_TENSOR_HEX_PAIRS(SF_CASE)
        }
    else
        switch (ni[0] * 64 + no[0])
        {
            SF_TENSOR_QUAD_PAIRS(SF_CASE)
        }
#undef SF_CASE
    return false;
}

} // namespace sf
