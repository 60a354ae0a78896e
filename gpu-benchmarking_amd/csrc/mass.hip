// mass.hip -- fp64 instantiations of the fused mass kernels (mass_wave.h) + nq dispatch; configuration in mass_launch.h.
// The fp32 instantiations are in mass_f32.hip (a translation unit of their own: the two halves build in parallel).
#include "mass_launch.h"

namespace sf
{

// SF_ENOTBUILT when the order has no instantiation (3D isotropic nq 2..11, 2D isotropic nq 2..16)
int launch_hex_mass_wave_nq(unsigned nq, const HexArgs &a, const double *w, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_hex_mass<N, double>(a, w, s);
        SF_MASS_HEX_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

int launch_quad_mass_wave_nq(unsigned nq, const QuadArgs &a, const double *w, hipStream_t s)
{
    switch (nq)
    {
#define SF_CASE(N) case N: return go_quad_mass<N, double>(a, w, s);
        SF_MASS_QUAD_CASES(SF_CASE)
#undef SF_CASE
    default: return SF_ENOTBUILT;
    }
}

bool mass_wave_built(int dim, unsigned nq)
{
    return nq >= 2 && nq <= (dim == 3 ? 11u : 16u);
}

} // namespace sf
