// rtc_config.h -- launch configuration of the run-time specialised wave kernels (rtc.hip): which template arguments
// a shape gets and how much dynamic LDS its launch needs.  Plain C++ (no HIP): the host restates, with run-time
// constexpr functions, what Cfg3 (bwdtrans_rt.hip) and BwdGeom (bwdtrans_wave.h) compute at compile time.  bwdtrans_rt.hip and rtc.hip pin the two against each other with static_asserts, so the
// host and the device cannot disagree on the slab size.
#pragma once

#include <cstddef>

namespace sf
{

constexpr int rtc_cdiv(int a, int b)
{
    return (a + b - 1) / b;
}
constexpr int rtc_max(int a, int b)
{
    return a > b ? a : b;
}
constexpr int rtc_clamp(int v, int lo, int hi)
{
    return v < lo ? lo : (v > hi ? hi : v);
}

constexpr int kRtcMaxLds   = 64 * 1024; // dynamic LDS per workgroup a specialisation may use
constexpr int kRtcMaxExt3  = 16;        // extents per direction: 3D 2..16, 2D 2..24
constexpr int kRtcMaxExt2  = 24;
constexpr int kRtcBasisSmem = 1, kRtcBasisCols = 2; // BASIS_SMEM / BASIS_SMEM_COLS of bwdtrans_wave.h

struct RtcCfg
{
    int ec, wpb, bmode, minw, xg;
    int slab;   // scalars per wave (BwdGeom::SLAB)
    size_t lds; // dynamic LDS bytes of one workgroup
    bool ok;    // false: the slab of one wave exceeds kRtcMaxLds
};

// BwdGeom<3, EC, T, NQ0, NQ1, NQ2>::SLAB, vw = scalars per 16-byte lane
constexpr int rtc_slab3(int nq0, int nq1, int nq2, int ec, int vw)
{
    const int nm0 = nq0 - 1, nm1 = nq1 - 1, nm2 = nq2 - 1;
    const int p0 = ec * nm2 * nm1, p1 = ec * nq0 * nm2, p2 = ec * nq1 * nq0;
    const int slab0 = rtc_max(rtc_max(p0 * (nm0 | 1), p1 * (nm1 | 1)), p2 * (nm2 | 1));
    return (rtc_max(slab0, ec * nq0 * nq1 * nq2) + vw - 1) / vw * vw;
}

// BwdGeom<2, EC, T, NQ0, NQ1>::SLAB
constexpr int rtc_slab2(int nq0, int nq1, int ec, int vw)
{
    const int nm0 = nq0 - 1, nm1 = nq1 - 1;
    const int slab0 = rtc_max(ec * nm1 * (nm0 | 1), ec * nq0 * (nm1 | 1));
    return (rtc_max(slab0, ec * nq0 * nq1) + vw - 1) / vw * vw;
}

// Cfg3<NQ0, NQ1, NQ2>::EC: chunks of about one nq = 8 element (512 points)
constexpr int rtc_ec3(int nq0, int nq1, int nq2)
{
    return rtc_clamp(512 / (nq0 * nq1 * nq2), 1, 8);
}

// 2D: about 256 points per chunk (the isotropic 2D rows, wave_table.h), and enough pencils to occupy 48 of the 64
// lanes in the wider sweep
constexpr int rtc_ec2(int nq0, int nq1)
{
    return rtc_clamp(rtc_max(256 / (nq0 * nq1), rtc_cdiv(48, rtc_max(nq1 - 1, nq0))), 1, 16);
}

// dim 3 ignores nothing, dim 2 ignores nq2; sbytes 8 (fp64) or 4 (fp32: twice the elements, the same bytes).
// Four waves per workgroup as Cfg3, halved while the workgroup's slabs exceed kRtcMaxLds.
constexpr RtcCfg rtc_cfg(int dim, int nq0, int nq1, int nq2, int sbytes)
{
    RtcCfg c{};
    const int vw = 16 / sbytes;
    const int mx = dim == 3 ? rtc_max(rtc_max(nq0, nq1), nq2) : rtc_max(nq0, nq1);
    c.ec    = (dim == 3 ? rtc_ec3(nq0, nq1, nq2) : rtc_ec2(nq0, nq1)) * (sbytes == 4 ? 2 : 1);
    // basis rows as scalar operands: whole rows up to nq = 10 (Cfg3), column blocks above for fp64; fp32 rows take half
    // the SGPRs and stay whole (its column-blocked form needs scratch under some compilers, e.g. ROCm 7.0's)
    c.bmode = (mx <= 10 || sbytes == 4) ? kRtcBasisSmem : kRtcBasisCols;
    c.minw  = 2;
    c.xg    = 64;
    c.slab  = dim == 3 ? rtc_slab3(nq0, nq1, nq2, c.ec, vw) : rtc_slab2(nq0, nq1, c.ec, vw);
    c.wpb   = 4;
    while (c.wpb > 1 && (size_t)sbytes * c.wpb * c.slab > (size_t)kRtcMaxLds)
        c.wpb >>= 1;
    c.lds = (size_t)sbytes * c.wpb * c.slab;
    c.ok  = c.lds <= (size_t)kRtcMaxLds;
    return c;
}

// ---- sf_tensor_*: the wave kernels with independent input / output extents (hex_tensor_wave_kernel,
// quad_tensor_wave_kernel of bwdtrans_aniso.h).  One function serves the ahead-of-time table (tensor_launch.h) and the
// run-time specialisation (rtc.hip).  A first choice, not a tuned one: the rules of rtc_cfg with "points" read as "the
// larger of the two images", so that ni = nq - 1, no = nq reproduces rtc_cfg (pinned below).
constexpr int kTensorMaxExt3 = 16, kTensorMaxExt2 = 24; // extents per direction a specialisation takes, from 1

// SweepGeom<DIM, EC, T, I0, O0, I1, O1, I2, O2>::SLAB (2D: ni[2] = no[2] = 1), vw = scalars per 16-byte lane
constexpr int tensor_slab(int dim, const int (&ni)[3], const int (&no)[3], int ec, int vw)
{
    const int i2 = dim == 3 ? ni[2] : 1, o2 = dim == 3 ? no[2] : 1;
    const int p0 = ec * i2 * ni[1], p1 = ec * no[0] * i2, p2 = ec * no[1] * no[0];
    const int w2 = dim == 3 ? p2 * (i2 | 1) : 0;
    const int slab0 = rtc_max(rtc_max(p0 * (ni[0] | 1), p1 * (ni[1] | 1)), w2);
    return (rtc_max(slab0, ec * no[0] * no[1] * o2) + vw - 1) / vw * vw;
}

// elements per chunk for fp64: about 512 (3D) / 256 (2D) scalars of the larger image, in 2D at least 48 pencils in the
// wider sweep
constexpr int tensor_ec(int dim, const int (&ni)[3], const int (&no)[3])
{
    if (dim == 3)
        return rtc_clamp(512 / rtc_max(ni[0] * ni[1] * ni[2], no[0] * no[1] * no[2]), 1, 8);
    return rtc_clamp(rtc_max(256 / rtc_max(ni[0] * ni[1], no[0] * no[1]), rtc_cdiv(48, rtc_max(ni[1], no[0]))), 1, 16);
}

// 2D ignores ni[2] / no[2]; sbytes 8 (fp64) or 4 (fp32: twice the elements, the same bytes)
constexpr RtcCfg tensor_cfg(int dim, const int (&ni)[3], const int (&no)[3], int sbytes)
{
    RtcCfg c{};
    int mx = 1;
    for (int d = 0; d < dim; ++d)
        mx = rtc_max(mx, rtc_max(ni[d], no[d]));
    c.ec    = tensor_ec(dim, ni, no) * (sbytes == 4 ? 2 : 1);
    c.bmode = (mx <= 10 || sbytes == 4) ? kRtcBasisSmem : kRtcBasisCols;
    c.minw  = 2;
    c.xg    = 64;
    c.slab  = tensor_slab(dim, ni, no, c.ec, 16 / sbytes);
    c.wpb   = 4;
    while (c.wpb > 1 && (size_t)sbytes * c.wpb * c.slab > (size_t)kRtcMaxLds)
        c.wpb >>= 1;
    c.lds = (size_t)sbytes * c.wpb * c.slab;
    c.ok  = c.lds <= (size_t)kRtcMaxLds;
    return c;
}

// ni = nq - 1, no = nq is rtc_cfg
constexpr bool tensor_cfg_is_rtc_cfg(int dim, int nq0, int nq1, int nq2, int sbytes)
{
    const int ni[3] = {nq0 - 1, nq1 - 1, dim == 3 ? nq2 - 1 : 1}, no[3] = {nq0, nq1, dim == 3 ? nq2 : 1};
    const RtcCfg a = tensor_cfg(dim, ni, no, sbytes), b = rtc_cfg(dim, nq0, nq1, nq2, sbytes);
    return a.ec == b.ec && a.wpb == b.wpb && a.bmode == b.bmode && a.minw == b.minw && a.xg == b.xg && a.slab == b.slab &&
           a.lds == b.lds && a.ok == b.ok;
}
constexpr bool tensor_cfg_is_rtc_cfg_everywhere()
{
    for (int s = 4; s <= 8; s += 4)
    {
        for (int a = 2; a <= kRtcMaxExt3; ++a)
            for (int b = 2; b <= kRtcMaxExt3; ++b)
                for (int c = 2; c <= kRtcMaxExt3; ++c)
                    if (!tensor_cfg_is_rtc_cfg(3, a, b, c, s))
                        return false;
        for (int a = 2; a <= kRtcMaxExt2; ++a)
            for (int b = 2; b <= kRtcMaxExt2; ++b)
                if (!tensor_cfg_is_rtc_cfg(2, a, b, 0, s))
                    return false;
    }
    return true;
}
static_assert(tensor_cfg_is_rtc_cfg_everywhere(), "tensor_cfg with ni = nq - 1, no = nq is rtc_cfg");

} // namespace sf
