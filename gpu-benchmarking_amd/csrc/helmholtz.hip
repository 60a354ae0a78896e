// helmholtz.hip -- fp64 instantiations of the fused Helmholtz kernels (helmholtz_wave.h) + nq dispatch; configuration in
// helmholtz_launch.h.  The fp32 instantiations are in helmholtz_f32.hip (the two halves build in parallel).
#include "helmholtz_launch.h"

namespace sf
{

template int launch_helmholtz_wave<3, double>(unsigned, const HexArgs &, const HelmArgsT<double> &, hipStream_t);
template int launch_helmholtz_wave<2, double>(unsigned, const QuadArgs &, const HelmArgsT<double> &, hipStream_t);

// 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool helmholtz_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
