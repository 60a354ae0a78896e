// rtc_compile.cc -- compile half of the run-time specialisation (see rtc_compile.h).  Host C++ only.
#include "rtc_compile.h"

#include "../../include/sumfact.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <mutex>

namespace sf
{
namespace
{
#include "rtc_sources.inc" // kRtcHeaderNames / kRtcHeaderTexts / kRtcNumHeaders (tools/embed_rtc_sources.py)

// hiprtc supplies the device-side types itself; these stand in for the host headers the kernel headers include
const char *const kStandInNames[] = {"hip/hip_runtime.h", "cstddef", "cstdint", "stddef.h", "stdint.h"};
const char kStdTypes[] = "#pragma once\n"
                         "typedef __hip_internal::uint8_t uint8_t;\n"
                         "typedef __hip_internal::uint16_t uint16_t;\n"
                         "typedef __hip_internal::uint32_t uint32_t;\n"
                         "typedef __hip_internal::uint64_t uint64_t;\n"
                         "typedef __hip_internal::int8_t int8_t;\n"
                         "typedef __hip_internal::int16_t int16_t;\n"
                         "typedef __hip_internal::int32_t int32_t;\n"
                         "typedef __hip_internal::int64_t int64_t;\n"
                         "typedef __hip_internal::uint64_t uintptr_t;\n";
const char *const kStandInTexts[] = {"#pragma once\n", kStdTypes, kStdTypes, kStdTypes, kStdTypes};
constexpr int kNumStandIns        = 5;

// the hiprtc entry points used here (hiprtcResult is an int-sized enum, hiprtcProgram a pointer)
struct Hiprtc
{
    typedef int (*Create)(void **, const char *, const char *, int, const char *const *, const char *const *);
    typedef int (*Destroy)(void **);
    typedef int (*AddName)(void *, const char *);
    typedef int (*Compile)(void *, int, const char *const *);
    typedef int (*Lowered)(void *, const char *, const char **);
    typedef int (*Size)(void *, size_t *);
    typedef int (*Get)(void *, char *);
    typedef const char *(*ErrStr)(int);
    Create create;
    Destroy destroy;
    AddName add_name;
    Compile compile;
    Lowered lowered;
    Size log_size, code_size;
    Get log, code;
    ErrStr err;
};

// dlopen'ed once, on the first compile; nullptr when the library or a symbol is missing (never linked: libsumfact.so
// has no DT_NEEDED on it)
const Hiprtc *hiprtc(std::string *why)
{
    static Hiprtc h;
    static const Hiprtc *ok = nullptr;
    static std::string err;
    static std::once_flag once;
    std::call_once(once, [] {
        void *lib = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
        if (!lib)
            lib = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib)
        {
            const char *e = dlerror();
            err = std::string("hiprtc not found: ") + (e ? e : "dlopen failed");
            return;
        }
        bool all = true;
        auto sym = [&](const char *n) {
            void *p = dlsym(lib, n);
            if (!p)
            {
                all = false;
                err = std::string("hiprtc lacks ") + n;
            }
            return p;
        };
        h.create    = (Hiprtc::Create)sym("hiprtcCreateProgram");
        h.destroy   = (Hiprtc::Destroy)sym("hiprtcDestroyProgram");
        h.add_name  = (Hiprtc::AddName)sym("hiprtcAddNameExpression");
        h.compile   = (Hiprtc::Compile)sym("hiprtcCompileProgram");
        h.lowered   = (Hiprtc::Lowered)sym("hiprtcGetLoweredName");
        h.log_size  = (Hiprtc::Size)sym("hiprtcGetProgramLogSize");
        h.log       = (Hiprtc::Get)sym("hiprtcGetProgramLog");
        h.code_size = (Hiprtc::Size)sym("hiprtcGetCodeSize");
        h.code      = (Hiprtc::Get)sym("hiprtcGetCode");
        h.err       = (Hiprtc::ErrStr)sym("hiprtcGetErrorString");
        if (all)
            ok = &h;
    });
    if (!ok && why)
        *why = err;
    return ok;
}

} // namespace

int rtc_key(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, RtcKey *k)
{
    const unsigned mx = dim == 3 ? (unsigned)kRtcMaxExt3 : (unsigned)kRtcMaxExt2;
    if ((dim != 2 && dim != 3) || (scalar_bytes != 4 && scalar_bytes != 8))
        return SF_EINVAL;
    if (nq0 < 2 || nq1 < 2 || nq0 > mx || nq1 > mx || (dim == 3 && (nq2 < 2 || nq2 > mx)))
        return SF_EINVAL;
    *k = RtcKey{dim, (int)nq0, (int)nq1, dim == 3 ? (int)nq2 : 0, scalar_bytes};
    return SF_OK;
}

int rtc_tensor_key(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes, RtcKey *k)
{
    if ((dim != 2 && dim != 3) || (scalar_bytes != 4 && scalar_bytes != 8) || (trans != 0 && trans != 1))
        return SF_EINVAL;
    const unsigned mx = dim == 3 ? (unsigned)kTensorMaxExt3 : (unsigned)kTensorMaxExt2;
    for (int d = 0; d < dim; ++d)
        if (ni[d] < 1 || no[d] < 1 || ni[d] > mx || no[d] > mx)
            return SF_EINVAL;
    *k       = RtcKey{dim, (int)no[0], (int)no[1], dim == 3 ? (int)no[2] : 0, scalar_bytes};
    k->kind  = 1;
    k->ni0   = (int)ni[0];
    k->ni1   = (int)ni[1];
    k->ni2   = dim == 3 ? (int)ni[2] : 0;
    k->trans = trans;
    return SF_OK;
}

RtcCfg rtc_cfg_of(const RtcKey &k)
{
    if (k.kind == 1)
    {
        const int ni[3] = {k.ni0, k.ni1, k.dim == 3 ? k.ni2 : 1}, no[3] = {k.nq0, k.nq1, k.dim == 3 ? k.nq2 : 1};
        return tensor_cfg(k.dim, ni, no, k.sbytes);
    }
    return rtc_cfg(k.dim, k.nq0, k.nq1, k.nq2, k.sbytes);
}

std::string rtc_name_expression(const RtcKey &k)
{
    const RtcCfg c = rtc_cfg_of(k);
    char buf[200];
    const char *t = k.sbytes == 8 ? "double" : "float";
    if (k.kind == 1 && k.dim == 3)
        std::snprintf(buf, sizeof buf, "sf::hex_tensor_wave_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %s>",
                      k.ni0, k.nq0, k.ni1, k.nq1, k.ni2, k.nq2, k.trans, c.ec, c.wpb, c.bmode, c.minw, c.xg, t);
    else if (k.kind == 1)
        std::snprintf(buf, sizeof buf, "sf::quad_tensor_wave_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %s>", k.ni0,
                      k.nq0, k.ni1, k.nq1, k.trans, c.ec, c.wpb, c.bmode, c.minw, c.xg, t);
    else if (k.dim == 3)
        std::snprintf(buf, sizeof buf, "sf::hex_wave3_kernel<%d, %d, %d, %d, %d, %d, %d, %d, %s>", k.nq0, k.nq1, k.nq2,
                      c.ec, c.wpb, c.bmode, c.minw, c.xg, t);
    else
        std::snprintf(buf, sizeof buf, "sf::quad_wave2_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", k.nq0, k.nq1, c.ec,
                      c.wpb, c.bmode, c.minw, c.xg, t);
    return buf;
}

std::vector<std::string> rtc_options(const std::string &arch)
{
    return {"--offload-arch=" + arch, "-O3", "-std=c++17", "-Rpass-analysis=kernel-resource-usage"};
}

std::string rtc_describe(const RtcKey &k)
{
    char buf[96];
    const char *tr = k.trans ? ":t" : "";
    if (k.kind == 1 && k.dim == 3)
        std::snprintf(buf, sizeof buf, "%s 3D %d>%dx%d>%dx%d>%d%s", k.sbytes == 8 ? "fp64" : "fp32", k.ni0, k.nq0, k.ni1,
                      k.nq1, k.ni2, k.nq2, tr);
    else if (k.kind == 1)
        std::snprintf(buf, sizeof buf, "%s 2D %d>%dx%d>%d%s", k.sbytes == 8 ? "fp64" : "fp32", k.ni0, k.nq0, k.ni1, k.nq1,
                      tr);
    else if (k.dim == 3)
        std::snprintf(buf, sizeof buf, "%s 3D %dx%dx%d", k.sbytes == 8 ? "fp64" : "fp32", k.nq0, k.nq1, k.nq2);
    else
        std::snprintf(buf, sizeof buf, "%s 2D %dx%d", k.sbytes == 8 ? "fp64" : "fp32", k.nq0, k.nq1);
    return buf;
}

int rtc_compile(const RtcKey &k, const std::string &arch, RtcCode *out)
{
    *out = RtcCode{};
    // gfx950 only, and never an xnack+ code object
    if (arch.compare(0, 6, "gfx950") != 0 || arch.find("xnack+") != std::string::npos)
    {
        out->log = "refused target " + arch + ": only gfx950 (xnack-) code objects are built";
        return SF_ECOMPILE;
    }
    const RtcCfg c = rtc_cfg_of(k);
    if (!c.ok)
    {
        out->log = rtc_describe(k) + ": one wave's LDS slab exceeds 64 KiB";
        return SF_ECOMPILE;
    }
    std::string why;
    const Hiprtc *h = hiprtc(&why);
    if (!h)
    {
        out->log = why;
        return SF_ECOMPILE;
    }
    const char *names[kRtcNumHeaders + kNumStandIns];
    const char *texts[kRtcNumHeaders + kNumStandIns];
    for (int i = 0; i < kRtcNumHeaders; ++i)
        names[i] = kRtcHeaderNames[i], texts[i] = kRtcHeaderTexts[i];
    for (int i = 0; i < kNumStandIns; ++i)
        names[kRtcNumHeaders + i] = kStandInNames[i], texts[kRtcNumHeaders + i] = kStandInTexts[i];
    const char *src = "#include \"bwdtrans_aniso.h\"\n";
    const std::string expr = rtc_name_expression(k);
    const std::vector<std::string> opts = rtc_options(arch);
    std::vector<const char *> argv;
    for (const std::string &o : opts)
        argv.push_back(o.c_str());

    const auto t0 = std::chrono::steady_clock::now();
    void *prog    = nullptr;
    int rc        = h->create(&prog, src, "sf_rtc.hip", kRtcNumHeaders + kNumStandIns, texts, names);
    if (rc != 0)
    {
        out->log = std::string("hiprtcCreateProgram: ") + h->err(rc);
        return SF_ECOMPILE;
    }
    rc = h->add_name(prog, expr.c_str());
    const int crc = rc == 0 ? h->compile(prog, (int)argv.size(), argv.data()) : rc;
    out->seconds  = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    size_t n = 0;
    if (h->log_size(prog, &n) == 0 && n > 1)
    {
        std::string log(n, '\0');
        if (h->log(prog, &log[0]) == 0)
            out->log = log.c_str();
    }
    const size_t at = out->log.find("ScratchSize [bytes/lane]: ");
    if (at != std::string::npos)
        out->scratch = std::strtol(out->log.c_str() + at + 26, nullptr, 10);
    int result = SF_ECOMPILE;
    if (crc == 0)
    {
        const char *lowered = nullptr;
        size_t sz           = 0;
        if (h->lowered(prog, expr.c_str(), &lowered) == 0 && lowered && h->code_size(prog, &sz) == 0 && sz > 0)
        {
            out->lowered_name = lowered;
            out->code.resize(sz);
            if (h->code(prog, out->code.data()) == 0)
                result = SF_OK;
            else
                out->code.clear();
        }
    }
    else
        out->log += std::string("\nhiprtc: ") + h->err(crc) + " (" + expr + ")";
    h->destroy(&prog);
    return result;
}

uint64_t rtc_source_hash()
{
    uint64_t x = 0xcbf29ce484222325ull;
    auto mix   = [&](const char *s, size_t n) {
        for (size_t i = 0; i < n; ++i)
            x = (x ^ (unsigned char)s[i]) * 0x100000001b3ull;
    };
    for (int i = 0; i < kRtcNumHeaders; ++i)
    {
        mix(kRtcHeaderNames[i], std::strlen(kRtcHeaderNames[i]) + 1);
        mix(kRtcHeaderTexts[i], std::strlen(kRtcHeaderTexts[i]) + 1);
    }
    return x;
}

} // namespace sf
