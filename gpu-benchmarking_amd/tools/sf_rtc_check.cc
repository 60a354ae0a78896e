// sf_rtc_check -- compile shapes through the library's run-time specialisation code (csrc/rtc_compile.cc: the same
// embedded headers, options and launch configuration), with no device call, and print each one's resources.
//
//   bin/sf_rtc_check [--arch gfx950] SHAPE...     SHAPE = 6x6x12 (3D) | 4x9 (2D), suffix :f32 for fp32
// A tensor shape (sf_specialise_tensor) names input > output per direction: 4>7x4>7x4>7 | 9>6x9>6, suffixes :t for
// trans = 1 and :f32, in either order.
//
// Line 1: "source-hash <16 hex digits>" (FNV-1a 64 of the embedded headers).  Then per shape:
//   fp64 3D 6x6x12  vgpr 54 agpr 0 sgpr 70 scratch 0 spill v0/s0 occ 8 lds 49152 wpb 4 ec 1  compile 0.52 s  ok
// with "SPILLS" in place of "ok" when the kernel needs scratch (the library refuses such a specialisation), and
// "FAILED" when it does not compile; a tensor shape whose slab exceeds the limit of one workgroup prints "REFUSED" and the
// reason, without compiling.  Exit status: the number of shapes that failed to compile.
#include "../csrc/rtc_compile.h"
#include "../../include/sumfact.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <regex>
#include <sstream>
#include <string>

using namespace sf;

// 4>7x4>7x4>7[:t][:f32]
static bool parse_tensor_shape(std::string str, RtcKey *k)
{
    unsigned ni[3] = {1, 1, 1}, no[3] = {1, 1, 1};
    int n = 0, sb = 8, trans = 0;
    for (size_t colon; (colon = str.rfind(':')) != std::string::npos; str = str.substr(0, colon))
    {
        const std::string t = str.substr(colon + 1);
        if (t == "f32")
            sb = 4;
        else if (t == "t")
            trans = 1;
        else if (t != "f64")
            return false;
    }
    std::stringstream ss(str);
    std::string tok;
    while (std::getline(ss, tok, 'x'))
    {
        const size_t gt = tok.find('>');
        if (n == 3 || gt == std::string::npos || gt == 0 || gt + 1 == tok.size())
            return false;
        ni[n] = (unsigned)std::strtoul(tok.substr(0, gt).c_str(), nullptr, 10);
        no[n] = (unsigned)std::strtoul(tok.substr(gt + 1).c_str(), nullptr, 10);
        ++n;
    }
    return (n == 2 || n == 3) && rtc_tensor_key(n, ni, no, trans, sb, k) == SF_OK;
}

static bool parse_shape(const char *s, RtcKey *k)
{
    unsigned e[3] = {0, 0, 0};
    int n = 0, sb = 8;
    std::string str(s);
    if (str.find('>') != std::string::npos)
        return parse_tensor_shape(str, k);
    const size_t colon = str.find(':');
    if (colon != std::string::npos)
    {
        const std::string t = str.substr(colon + 1);
        if (t == "f32")
            sb = 4;
        else if (t != "f64")
            return false;
        str = str.substr(0, colon);
    }
    std::stringstream ss(str);
    std::string tok;
    while (std::getline(ss, tok, 'x'))
    {
        if (n == 3 || tok.empty())
            return false;
        e[n++] = (unsigned)std::strtoul(tok.c_str(), nullptr, 10);
    }
    return (n == 2 || n == 3) && rtc_key(n, e[0], e[1], e[2], sb, k) == SF_OK;
}

// "remark: <where>: VGPRs: 54 [-Rpass-analysis=kernel-resource-usage]" -> {"VGPRs": 54, ...}
static std::map<std::string, long> resources(const std::string &log)
{
    std::map<std::string, long> r;
    static const std::regex re(R"(remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass)");
    std::stringstream ss(log);
    std::string ln;
    std::smatch m;
    while (std::getline(ss, ln))
        if (std::regex_search(ln, m, re))
            r[m[1].str()] = std::stol(m[2].str());
    return r;
}

int main(int argc, char **argv)
{
    std::string arch = "gfx950";
    int first        = 1;
    if (argc > 2 && !std::strcmp(argv[1], "--arch"))
        arch = argv[2], first = 3;
    if (first >= argc)
    {
        std::fprintf(stderr, "usage: %s [--arch gfx950] SHAPE...  (6x6x12, 4x9, 3x5x4:f32)\n", argv[0]);
        return 255;
    }
    std::printf("source-hash %016llx\n", (unsigned long long)rtc_source_hash());
    int failed = 0;
    for (int i = first; i < argc; ++i)
    {
        RtcKey k;
        if (!parse_shape(argv[i], &k))
        {
            std::printf("%-18s invalid shape\n", argv[i]);
            ++failed;
            continue;
        }
        const RtcCfg c = rtc_cfg_of(k);
        if (k.kind == 1 && !c.ok)
        {
            std::printf("%-18s REFUSED  one wave's LDS slab (%zu bytes) exceeds %d\n", rtc_describe(k).c_str(), c.lds,
                        kRtcMaxLds);
            ++failed;
            continue;
        }
        RtcCode code;
        const int rc = rtc_compile(k, arch, &code);
        if (rc != SF_OK)
        {
            std::printf("%-18s FAILED  compile %.2f s\n%s\n", rtc_describe(k).c_str(), code.seconds, code.log.c_str());
            ++failed;
            continue;
        }
        auto r  = resources(code.log);
        auto at = [&](const char *key) { return r.count(key) ? r[key] : -1L; };
        const bool spills = at("ScratchSize") != 0 || at("VGPRs Spill") > 0 || at("SGPRs Spill") > 0;
        std::printf("%-18s vgpr %3ld agpr %3ld sgpr %3ld scratch %3ld spill v%ld/s%ld occ %ld lds %6zu wpb %d ec %2d  "
                    "compile %.2f s  %s\n",
                    rtc_describe(k).c_str(), at("VGPRs"), at("AGPRs"), at("TotalSGPRs"), at("ScratchSize"),
                    at("VGPRs Spill"), at("SGPRs Spill"), at("Occupancy"), c.lds, c.wpb, c.ec, code.seconds,
                    spills ? "SPILLS" : "ok");
        std::fflush(stdout);
    }
    return failed;
}
