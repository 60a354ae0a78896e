// mass.hip -- fp64 instantiations of the fused mass kernels (mass_wave.h) + nq dispatch; configuration in mass_launch.h.
// The fp32 instantiations are in mass_f32.hip (a translation unit of their own: the two halves build in parallel).
#include "mass_launch.h"

namespace sf
{

template int launch_mass_wave<3, double>(unsigned, const HexArgs &, const double *, hipStream_t);
template int launch_mass_wave<2, double>(unsigned, const QuadArgs &, const double *, hipStream_t);

// 3D isotropic nq 2..11, 2D isotropic nq 2..16
bool mass_wave_built(int dim, unsigned nq)
{
    return nq >= 2 && nq <= (dim == 3 ? 11u : 16u);
}

} // namespace sf
