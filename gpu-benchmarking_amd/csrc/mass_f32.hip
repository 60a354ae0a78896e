// mass_f32.hip -- fp32 instantiations of the fused mass kernels (mass_wave.h) + nq dispatch; configuration in
// mass_launch.h.  Same table of orders as mass.hip (mass_wave_built()).
#include "mass_launch.h"

namespace sf
{

int launch_hex_mass_wave_f32_nq(unsigned nq, const HexArgsT<float> &a, const float *w, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex_mass<N, float>(a, w, s);
        SF_MASS_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_mass_wave_f32_nq(unsigned nq, const QuadArgsT<float> &a, const float *w, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad_mass<N, float>(a, w, s);
        SF_MASS_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

} // namespace sf
