// diag.hip -- fp64 instantiations of the Helmholtz-diagonal kernels (diag_wave.h) + nq dispatch; configuration in
// diag_launch.h.  The fp32 instantiations are in diag_f32.hip (the two halves build in parallel).
#include "diag_launch.h"

namespace sf
{

template int launch_diag_wave<3, double>(unsigned, const HexArgs &, const DiagArgsT<double> &, hipStream_t);
template int launch_diag_wave<2, double>(unsigned, const QuadArgs &, const DiagArgsT<double> &, hipStream_t);

// 3D isotropic nq 2..8, 2D isotropic nq 2..16: the Helmholtz table
bool diag_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
