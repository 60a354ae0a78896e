// iprodderiv.hip -- fp64 instantiations of the IProductWRTDerivBase kernels (iprodderiv_wave.h) + nq dispatch;
// configuration in iprodderiv_launch.h.  The fp32 instantiations are in iprodderiv_f32.hip (the two halves build in
// parallel).
#include "iprodderiv_launch.h"

namespace sf
{

template int launch_iprodderiv_wave<3, double>(unsigned, const HexArgs &, const IprodDerivArgsT<double> &, hipStream_t);
template int launch_iprodderiv_wave<2, double>(unsigned, const QuadArgs &, const IprodDerivArgsT<double> &, hipStream_t);

// the Helmholtz table: 3D isotropic nq 2..8, 2D isotropic nq 2..16
bool iprodderiv_wave_built(int dim, unsigned nq)
{
    return helm_order_built(dim, nq);
}

} // namespace sf
