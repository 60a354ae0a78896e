// tensor_launch.h -- the ahead-of-time table of the sf_tensor_* wave kernels (hex_tensor_wave_kernel /
// quad_tensor_wave_kernel of bwdtrans_aniso.h) and its dispatch, for the scalar type and the dimension of the including
// unit: tensor.hip <3, double>, tensor_quad.hip <2, double>, tensor_f32.hip <3, float>, tensor_quad_f32.hip <2, float>.
//
// The table holds isotropic pairs ni -> no, every direction the same, both values of `trans`:
//   3D   n -> n for n 2..8;   n -> ceil(3n/2) and back for n 2..6   (2>3 3>5 4>6 5>8 6>9)
//   2D   n -> n for n 2..16;  n -> ceil(3n/2) and back for n 2..10  (... 7>11 8>12 9>14 10>15)
// Every row is tensor_cfg (rtc_config.h) as it stands, a first choice and not a tuned one; a pair that spilled under it
// would get a smaller EC here or leave the table (none does: no kernel of the table has scratch or spills, see
// tools/kernel_resources.py).  Every other shape is served by a run-time specialisation (rtc.hip) or the any-extent kernel
// (tensor_generic.hip).
#pragma once

#include "bwdtrans_aniso.h"
#include "chunked_launch.h"
#include "rtc_config.h"
#include "sf_dispatch.h"

namespace sf
{

static_assert(kRtcBasisSmem == BASIS_SMEM && kRtcBasisCols == BASIS_SMEM_COLS, "basis modes");

template <int DIM, int I, int O, int TR, typename T> static int go_tensor(const ArgsT<DIM, T> &a, hipStream_t s)
{
    static constexpr int ni[3] = {I, I, DIM == 3 ? I : 1}, no[3] = {O, O, DIM == 3 ? O : 1};
    constexpr RtcCfg c  = tensor_cfg(DIM, ni, no, (int)sizeof(T));
    using G             = SweepGeom<DIM, c.ec, T, I, O, I, O, DIM == 3 ? I : 1, DIM == 3 ? O : 1>;
    static_assert(c.ok && c.slab == G::SLAB && c.lds == slab_lds_bytes<G, c.wpb>(), "tensor_cfg against SweepGeom");
    static OccCache cache = {};
    if constexpr (DIM == 3)
        return launch_chunked<c.wpb, c.ec, 1>(
            hex_tensor_wave_kernel<I, O, I, O, I, O, TR, c.ec, c.wpb, c.bmode, c.minw, c.xg, T>, cache, c.lds, 0, s,
            a.nelmt, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
    else
        return launch_chunked<c.wpb, c.ec, 1>(quad_tensor_wave_kernel<I, O, I, O, TR, c.ec, c.wpb, c.bmode, c.minw, c.xg, T>,
                                              cache, c.lds, 0, s, a.nelmt, a.b0, a.b1, a.in, a.out, a.nelmt);
}

#define SF_TENSOR_HEX_PAIRS(F)                                                                                         \
    F(2, 2) F(3, 3) F(4, 4) F(5, 5) F(6, 6) F(7, 7) F(8, 8)                                                            \
    F(2, 3) F(3, 5) F(4, 6) F(5, 8) F(6, 9) F(3, 2) F(5, 3) F(6, 4) F(8, 5) F(9, 6)
#define SF_TENSOR_QUAD_PAIRS(F)                                                                                        \
    F(2, 2) F(3, 3) F(4, 4) F(5, 5) F(6, 6) F(7, 7) F(8, 8) F(9, 9) F(10, 10) F(11, 11) F(12, 12) F(13, 13) F(14, 14)  \
    F(15, 15) F(16, 16)                                                                                                \
    F(2, 3) F(3, 5) F(4, 6) F(5, 8) F(6, 9) F(7, 11) F(8, 12) F(9, 14) F(10, 15)                                       \
    F(3, 2) F(5, 3) F(6, 4) F(8, 5) F(9, 6) F(11, 7) F(12, 8) F(14, 9) F(15, 10)

// the isotropic pair of a shape, or false
template <int DIM> static bool tensor_iso_pair(const unsigned (&ni)[3], const unsigned (&no)[3], unsigned *i, unsigned *o)
{
    for (int d = 1; d < DIM; ++d)
        if (ni[d] != ni[0] || no[d] != no[0])
            return false;
    *i = ni[0], *o = no[0];
    return true;
}

// SF_ENOTBUILT off the table
template <int DIM, typename T>
int launch_tensor_wave(const unsigned (&ni)[3], const unsigned (&no)[3], int trans, const ArgsT<DIM, T> &a, hipStream_t s)
{
    unsigned i = 0, o = 0;
    if (!tensor_iso_pair<DIM>(ni, no, &i, &o) || i > 63 || o > 63)
        return SF_ENOTBUILT;
#define SF_CASE(I, O)                                                                                                  \
    case I * 64 + O: return trans ? go_tensor<DIM, I, O, 1, T>(a, s) : go_tensor<DIM, I, O, 0, T>(a, s);
    if constexpr (DIM == 3)
        switch (i * 64 + o)
        {
            SF_TENSOR_HEX_PAIRS(SF_CASE)
        }
    else
        switch (i * 64 + o)
        {
            SF_TENSOR_QUAD_PAIRS(SF_CASE)
        }
#undef SF_CASE
    return SF_ENOTBUILT;
}

} // namespace sf
