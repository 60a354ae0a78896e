// rtc_compile.h -- compile half of the run-time specialisation (rtc_compile.cc): hiprtc, loaded with dlopen on first
// use, turns the embedded kernel headers into a code object for one shape.  No HIP runtime call: bin/sf_rtc_check uses
// it on a machine without a GPU, the library's load / launch half (rtc.hip) on top of it.
#pragma once

#include "rtc_config.h"

#include <cstdint>
#include <string>
#include <vector>

namespace sf
{

// kind 0: BwdTrans (hex_wave3_kernel / quad_wave2_kernel), nq<d> points from nq<d> - 1 modes; the fields below sbytes are 0.
// kind 1: the tensor-product apply (hex_tensor_wave_kernel / quad_tensor_wave_kernel): nq<d> are the output extents,
// ni<d> the input extents (dim 2: nq2 = ni2 = 0), trans 0 or 1.
struct RtcKey
{
    int dim, nq0, nq1, nq2, sbytes; // dim 2: nq2 = 0
    int kind = 0, ni0 = 0, ni1 = 0, ni2 = 0, trans = 0;
    bool operator<(const RtcKey &o) const
    {
        if (kind != o.kind)
            return kind < o.kind;
        if (ni0 != o.ni0)
            return ni0 < o.ni0;
        if (ni1 != o.ni1)
            return ni1 < o.ni1;
        if (ni2 != o.ni2)
            return ni2 < o.ni2;
        if (trans != o.trans)
            return trans < o.trans;
        if (dim != o.dim)
            return dim < o.dim;
        if (nq0 != o.nq0)
            return nq0 < o.nq0;
        if (nq1 != o.nq1)
            return nq1 < o.nq1;
        if (nq2 != o.nq2)
            return nq2 < o.nq2;
        return sbytes < o.sbytes;
    }
};

// SF_EINVAL unless dim is 2 or 3, every extent 2..16 (3D) / 2..24 (2D) and sbytes 4 or 8; *k normalised (dim 2: nq2 = 0)
int rtc_key(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, RtcKey *k);
// the same for a tensor shape: every extent 1..16 (3D) / 1..24 (2D), trans 0 or 1
int rtc_tensor_key(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes, RtcKey *k);
RtcCfg rtc_cfg_of(const RtcKey &k);
// the instantiation's name expression, e.g. sf::hex_wave3_kernel<6, 6, 12, 1, 4, 1, 2, 64, double>
std::string rtc_name_expression(const RtcKey &k);
// compile options for `arch` (a gcnArchName): what the Makefile gives hipcc, plus the resource-usage remarks
std::vector<std::string> rtc_options(const std::string &arch);
// "fp64 3D 6x6x12"; a tensor shape "fp64 3D 4>7x4>7x4>7", with ":t" behind it for trans = 1
std::string rtc_describe(const RtcKey &k);

struct RtcCode
{
    std::vector<char> code;   // code object (empty on failure)
    std::string lowered_name; // symbol of the instantiation in `code`
    std::string log;          // hiprtc's log (resource-usage remarks included)
    double seconds = 0;       // wall time of the compile
    long scratch   = 0;       // scratch bytes per lane the compiler reports (ScratchSize remark)
};

// SF_OK, or SF_ECOMPILE (hiprtc missing, arch refused, compile failed; out->log says which)
int rtc_compile(const RtcKey &k, const std::string &arch, RtcCode *out);
// FNV-1a 64 over the embedded headers, in order: name, NUL, text, NUL
uint64_t rtc_source_hash();

} // namespace sf
