// vecgrad.hip -- fp64 instantiations of the vector-gradient kernels (vecgrad_wave.h) + nq dispatch; configuration in
// vecgrad_launch.h.  The fp32 instantiations are in vecgrad_f32.hip (the two halves build in parallel).
#include "vecgrad_launch.h"

namespace sf
{

template int launch_vecgrad_wave<3, double>(unsigned, const HexArgs &, const VecgradArgsT<double> &, hipStream_t);
template int launch_vecgrad_wave<2, double>(unsigned, const QuadArgs &, const VecgradArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool vecgrad_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
