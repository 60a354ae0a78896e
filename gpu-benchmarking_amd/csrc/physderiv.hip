// physderiv.hip -- fp64 instantiations of the fused BwdTrans + gradient kernels (physderiv_wave.h) + nq dispatch;
// configuration in physderiv_launch.h.  The fp32 instantiations are in physderiv_f32.hip (the two halves build in
// parallel).
#include "physderiv_launch.h"

namespace sf
{

template int launch_physderiv_wave<3, double>(unsigned, const HexArgs &, const PhysDerivArgsT<double> &, hipStream_t);
template int launch_physderiv_wave<2, double>(unsigned, const QuadArgs &, const PhysDerivArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool physderiv_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
