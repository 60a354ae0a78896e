// helmholtz_f32.hip -- fp32 instantiations of the fused Helmholtz kernels (helmholtz_wave.h) + nq dispatch; configuration
// in helmholtz_launch.h.  Same table of orders as helmholtz.hip (helmholtz_wave_built()).
#include "helmholtz_launch.h"

namespace sf
{

int launch_hex_helmholtz_wave_f32_nq(unsigned nq, const HexArgsT<float> &a, const HelmArgsT<float> &x, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex_helmholtz<N, float>(a, x, s);
        SF_HELM_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_helmholtz_wave_f32_nq(unsigned nq, const QuadArgsT<float> &a, const HelmArgsT<float> &x, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad_helmholtz<N, float>(a, x, s);
        SF_HELM_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

} // namespace sf
