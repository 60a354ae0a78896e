// helmholtz.hip -- fp64 instantiations of the fused Helmholtz kernels (helmholtz_wave.h) + nq dispatch; configuration in
// helmholtz_launch.h.  The fp32 instantiations are in helmholtz_f32.hip (the two halves build in parallel).
#include "helmholtz_launch.h"

namespace sf
{

// SF_ENOTBUILT when the order has no instantiation (3D isotropic nq 2..8, 2D isotropic nq 2..16)
int launch_hex_helmholtz_wave_nq(unsigned nq, const HexArgs &a, const HelmArgsT<double> &x, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex_helmholtz<N, double>(a, x, s);
        SF_HELM_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_helmholtz_wave_nq(unsigned nq, const QuadArgs &a, const HelmArgsT<double> &x, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad_helmholtz<N, double>(a, x, s);
        SF_HELM_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

bool helmholtz_wave_built(int dim, unsigned nq)
{
    return nq >= 2 && nq <= (dim == 3 ? 8u : 16u);
}

} // namespace sf
