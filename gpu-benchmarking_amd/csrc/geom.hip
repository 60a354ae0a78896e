// geom.hip -- fp64 instantiations of the geometric-factor kernels (geom_wave.h) + nq dispatch; configuration in
// geom_launch.h.  The fp32 instantiations are in geom_f32.hip (the two halves build in parallel).
#include "geom_launch.h"

namespace sf
{

template int launch_geom_wave<3, double>(unsigned, const HexArgs &, const GeomArgsT<double> &, hipStream_t);
template int launch_geom_wave<2, double>(unsigned, const QuadArgs &, const GeomArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool geom_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
