// advect.hip -- fp64 instantiations of the advection kernels (advect_wave.h) + nq dispatch; configuration in
// advect_launch.h.  The fp32 instantiations are in advect_f32.hip (the two halves build in parallel).
#include "advect_launch.h"

namespace sf
{

template int launch_advect_wave<3, double>(unsigned, const HexArgs &, const AdvectArgsT<double> &, hipStream_t);
template int launch_advect_wave<2, double>(unsigned, const QuadArgs &, const AdvectArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool advect_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
