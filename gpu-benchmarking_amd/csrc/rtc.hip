// rtc.hip -- load / launch half of the run-time specialisation: sf_specialise() compiles (once per process, through
// rtc_compile.cc) and loads (once per device) the wave-per-chunk kernel of bwdtrans_aniso.h for the
// extents a caller names; AUTO then launches it for shapes the compiled tables miss.  sf_specialise_tensor() does the
// same for the tensor kernels of that header (independent input / output extents, sf_tensor_*), under keys of their own.
// Nothing here compiles or loads behind a launch: a launch only finds what sf_specialise() made ready.
#include "bwdtrans_aniso.h"
#include "rtc_compile.h"
#include "sf_dispatch.h"

#include <atomic>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>

namespace sf
{

// the host's launch configuration against the templates' own geometry, 2D and odd 3D shapes (the 33 compile-time
// triples are pinned in bwdtrans_rt.hip)
template <int A, int B, int S> constexpr bool rtc_pins2()
{
    constexpr RtcCfg c = rtc_cfg(2, A, B, 0, S);
    using T            = typename std::conditional<S == 8, double, float>::type;
    using G            = BwdGeom<2, c.ec, T, A, B>;
    return c.slab == G::SLAB && c.lds == slab_lds_bytes<G, c.wpb>();
}
template <int A, int B, int C, int S> constexpr bool rtc_pins3()
{
    constexpr RtcCfg c = rtc_cfg(3, A, B, C, S);
    using T            = typename std::conditional<S == 8, double, float>::type;
    using G            = BwdGeom<3, c.ec, T, A, B, C>;
    return c.slab == G::SLAB && c.lds == slab_lds_bytes<G, c.wpb>();
}
static_assert(kRtcBasisSmem == BASIS_SMEM && kRtcBasisCols == BASIS_SMEM_COLS, "basis modes");
static_assert(rtc_pins2<4, 9, 8>() && rtc_pins2<16, 3, 8>() && rtc_pins2<12, 20, 8>() && rtc_pins2<23, 5, 8>() &&
                  rtc_pins2<2, 24, 8>() && rtc_pins2<24, 24, 8>() && rtc_pins2<4, 9, 4>() && rtc_pins2<7, 2, 4>(),
              "2D launch configuration");
static_assert(rtc_pins3<6, 6, 12, 8>() && rtc_pins3<12, 10, 8, 8>() && rtc_pins3<5, 9, 7, 8>() &&
                  rtc_pins3<3, 5, 4, 8>() && rtc_pins3<2, 3, 2, 8>() && rtc_pins3<16, 12, 14, 8>() &&
                  rtc_pins3<3, 5, 4, 4>() && rtc_pins3<6, 6, 12, 4>(),
              "3D launch configuration");

// tensor_cfg against SweepGeom for the shapes the tests name off the table (the table's own are pinned in tensor_launch.h)
template <int DIM, int I0, int O0, int I1, int O1, int I2, int O2, int S> constexpr bool tensor_pins()
{
    constexpr int ni[3] = {I0, I1, I2}, no[3] = {O0, O1, O2};
    constexpr RtcCfg c  = tensor_cfg(DIM, ni, no, S);
    using T             = typename std::conditional<S == 8, double, float>::type;
    using G             = SweepGeom<DIM, c.ec, T, I0, O0, I1, O1, I2, O2>;
    return c.slab == G::SLAB && c.lds == slab_lds_bytes<G, c.wpb>();
}
static_assert(tensor_pins<3, 4, 7, 4, 7, 4, 7, 8>() && tensor_pins<3, 7, 4, 7, 4, 7, 4, 8>() &&
                  tensor_pins<3, 5, 8, 3, 3, 6, 4, 8>() && tensor_pins<3, 7, 8, 7, 8, 7, 8, 8>() &&
                  tensor_pins<3, 3, 4, 3, 4, 3, 4, 8>() && tensor_pins<3, 8, 7, 8, 7, 8, 7, 8>() &&
                  tensor_pins<3, 4, 3, 4, 3, 4, 3, 8>() && tensor_pins<3, 3, 5, 4, 4, 6, 2, 8>() &&
                  tensor_pins<3, 1, 4, 2, 2, 5, 1, 8>() && tensor_pins<3, 16, 16, 2, 3, 1, 1, 8>() &&
                  tensor_pins<3, 1, 16, 16, 1, 16, 1, 8>() && tensor_pins<3, 4, 7, 4, 7, 4, 7, 4>() &&
                  tensor_pins<3, 5, 8, 3, 3, 6, 4, 4>(),
              "3D tensor launch configuration");
static_assert(tensor_pins<2, 1, 4, 9, 3, 1, 1, 8>() && tensor_pins<2, 10, 15, 6, 9, 1, 1, 8>() &&
                  tensor_pins<2, 7, 8, 7, 8, 1, 1, 8>() && tensor_pins<2, 15, 16, 15, 16, 1, 1, 8>() &&
                  tensor_pins<2, 8, 7, 8, 7, 1, 1, 8>() && tensor_pins<2, 16, 15, 16, 15, 1, 1, 8>() &&
                  tensor_pins<2, 24, 20, 7, 24, 1, 1, 8>() && tensor_pins<2, 9, 6, 9, 6, 1, 1, 4>() &&
                  tensor_pins<2, 10, 15, 6, 9, 1, 1, 4>(),
              "2D tensor launch configuration");

namespace
{

struct Compiled // one code object per (arch, shape)
{
    int rc;
    RtcCode code;
    unsigned serial; // n-th compile of the process
};

struct Loaded // one module per (device, shape)
{
    int state = 0; // 1 ready, SF_ECOMPILE failed
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    RtcCfg cfg{};
    std::atomic<uint64_t> launches{0};
};

struct DevKey
{
    int dev;
    RtcKey k;
    bool operator<(const DevKey &o) const
    {
        return dev != o.dev ? dev < o.dev : k < o.k;
    }
};

std::mutex g_mu; // covers compile and load
std::atomic<int> g_ready{0}; // modules ready on any device: AUTO's only cost while it is 0
std::map<std::pair<std::string, RtcKey>, std::unique_ptr<Compiled>> g_code;
std::map<DevKey, std::unique_ptr<Loaded>> g_loaded;
unsigned g_compiles = 0;
thread_local std::string t_log;

// the ready module of `k` on the current device, or nullptr
Loaded *ready(const RtcKey &k)
{
    if (g_ready.load(std::memory_order_relaxed) == 0)
        return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return nullptr;
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_loaded.find(DevKey{dev, k});
    return (it != g_loaded.end() && it->second->state == 1) ? it->second.get() : nullptr;
}

int launch(Loaded &L, int dim, const void *b0, const void *b1, const void *b2, const void *in, void *out,
           uint64_t nelmt, hipStream_t s)
{
    if (nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (nelmt + L.cfg.ec - 1) / L.cfg.ec;
    const uint64_t grid   = (nchunk + L.cfg.wpb - 1) / L.cfg.wpb;
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    void *args3[] = {&b0, &b1, &b2, &in, &out, &nelmt};
    void *args2[] = {&b0, &b1, &in, &out, &nelmt};
    hipError_t e  = hipModuleLaunchKernel(L.fn, (unsigned)grid, 1, 1, kWave * L.cfg.wpb, 1, 1, (unsigned)L.cfg.lds, s,
                                          dim == 3 ? args3 : args2, nullptr);
    if (e != hipSuccess)
        return (int)e;
    L.launches.fetch_add(1, std::memory_order_relaxed);
    return SF_OK;
}

// compile (once per process and arch) and load (once per device) the kernel of `k`
int specialise(const RtcKey &k)
{
    int dev      = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return (int)e;
    hipDeviceProp_t p;
    if ((e = hipGetDeviceProperties(&p, dev)) != hipSuccess)
        return (int)e;
    const std::string arch = p.gcnArchName; // verbatim, e.g. gfx950:sramecc+:xnack-

    std::lock_guard<std::mutex> g(g_mu);
    std::unique_ptr<Compiled> &cc = g_code[{arch, k}];
    if (!cc)
    {
        cc.reset(new Compiled);
        cc->rc     = rtc_compile(k, arch, &cc->code);
        cc->serial = ++g_compiles;
    }
    char head[320];
    std::snprintf(head, sizeof head, "sf_specialise%s %s, device %d (%s): compile #%u, %.3f s\n%s\n",
                  k.kind == 1 ? "_tensor" : "", rtc_describe(k).c_str(), dev, arch.c_str(), cc->serial, cc->code.seconds,
                  rtc_name_expression(k).c_str());
    t_log = head + cc->code.log;

    auto it = g_loaded.find(DevKey{dev, k});
    if (it != g_loaded.end())
        return it->second->state == 1 ? SF_OK : SF_ECOMPILE;
    std::unique_ptr<Loaded> L(new Loaded);
    L->cfg = rtc_cfg_of(k);
    if (cc->rc != SF_OK)
    {
        L->state = SF_ECOMPILE;
        g_loaded[DevKey{dev, k}] = std::move(L);
        return SF_ECOMPILE;
    }
    if ((e = hipModuleLoadData(&L->mod, cc->code.code.data())) != hipSuccess)
        return (int)e; // nothing cached: a later call may try again
    if ((e = hipModuleGetFunction(&L->fn, L->mod, cc->code.lowered_name.c_str())) != hipSuccess)
    {
        (void)hipModuleUnload(L->mod);
        return (int)e;
    }
    // spill guard: a specialisation that needs scratch is refused (AUTO keeps today's route)
    int scratch = 0;
    if ((e = hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, L->fn)) != hipSuccess || scratch > 0 ||
        cc->code.scratch > 0)
    {
        scratch = scratch > 0 ? scratch : (int)cc->code.scratch;
        (void)hipModuleUnload(L->mod);
        L->mod = nullptr, L->fn = nullptr;
        if (e != hipSuccess)
            return (int)e;
        char why[96];
        std::snprintf(why, sizeof why, "refused: the kernel spills (%d bytes of scratch per lane)\n", scratch);
        t_log += why;
        L->state = SF_ECOMPILE;
        g_loaded[DevKey{dev, k}] = std::move(L);
        return SF_ECOMPILE;
    }
    L->state = 1;
    g_loaded[DevKey{dev, k}] = std::move(L);
    g_ready.fetch_add(1, std::memory_order_relaxed);
    return SF_OK;
}

int state(const RtcKey &k, uint64_t *launches)
{
    int dev      = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return (int)e;
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_loaded.find(DevKey{dev, k});
    if (launches)
        *launches = it == g_loaded.end() ? 0 : it->second->launches.load(std::memory_order_relaxed);
    return it == g_loaded.end() ? 0 : it->second->state;
}

} // namespace

int rtc_specialise(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes)
{
    RtcKey k;
    if (rtc_key(dim, nq0, nq1, nq2, scalar_bytes, &k) != SF_OK)
        return SF_EINVAL;
    return specialise(k);
}

int rtc_state(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, uint64_t *launches)
{
    RtcKey k;
    if (rtc_key(dim, nq0, nq1, nq2, scalar_bytes, &k) != SF_OK)
        return SF_EINVAL;
    return state(k, launches);
}

// The tensor kernels.  A request while a blocking stream of the device is capturing is refused before anything is
// compiled or loaded (a module load is not a capturable call); the Python binding refuses the same for the stream it
// knows to be capturing.
int rtc_specialise_tensor(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes)
{
    RtcKey k;
    if (rtc_tensor_key(dim, ni, no, trans, scalar_bytes, &k) != SF_OK)
        return SF_EINVAL;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const hipError_t ce        = hipStreamIsCapturing(nullptr, &cap);
    (void)hipGetLastError(); // any other error is the device's: specialise() reports it
    if (ce == hipErrorStreamCaptureImplicit || (ce == hipSuccess && cap != hipStreamCaptureStatusNone))
    {
        t_log = "sf_specialise_tensor " + rtc_describe(k) + ": refused, a stream capture is under way\n";
        return SF_ECOMPILE;
    }
    return specialise(k);
}

int rtc_tensor_state(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes,
                     uint64_t *launches)
{
    RtcKey k;
    if (rtc_tensor_key(dim, ni, no, trans, scalar_bytes, &k) != SF_OK)
        return SF_EINVAL;
    return state(k, launches);
}

int launch_tensor_specialised(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes,
                              const void *m0, const void *m1, const void *m2, const void *in, void *out, uint64_t nelmt,
                              hipStream_t s)
{
    if (g_ready.load(std::memory_order_relaxed) == 0) // the common case: one relaxed load
        return SF_ENOTBUILT;
    RtcKey k;
    if (rtc_tensor_key(dim, ni, no, trans, scalar_bytes, &k) != SF_OK)
        return SF_ENOTBUILT;
    Loaded *L = ready(k);
    return L ? launch(*L, dim, m0, m1, m2, in, out, nelmt, s) : SF_ENOTBUILT;
}

int launch_specialised(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, const void *b0,
                       const void *b1, const void *b2, const void *in, void *out, uint64_t nelmt, hipStream_t s)
{
    if (g_ready.load(std::memory_order_relaxed) == 0) // the common case: one relaxed load
        return SF_ENOTBUILT;
    RtcKey k;
    if (rtc_key(dim, nq0, nq1, nq2, scalar_bytes, &k) != SF_OK)
        return SF_ENOTBUILT;
    Loaded *L = ready(k);
    return L ? launch(*L, dim, b0, b1, b2, in, out, nelmt, s) : SF_ENOTBUILT;
}

const char *rtc_last_log()
{
    return t_log.c_str();
}

int rtc_release()
{
    std::lock_guard<std::mutex> g(g_mu);
    int cur = 0;
    const bool have = hipGetDevice(&cur) == hipSuccess;
    int rc          = SF_OK;
    for (auto &kv : g_loaded)
        if (kv.second->mod)
        {
            hipError_t e = hipSetDevice(kv.first.dev);
            if (e == hipSuccess)
                e = hipModuleUnload(kv.second->mod);
            if (e != hipSuccess && rc == SF_OK)
                rc = (int)e;
        }
    if (have && !g_loaded.empty())
        (void)hipSetDevice(cur);
    g_loaded.clear();
    g_ready.store(0, std::memory_order_relaxed);
    return rc;
}

} // namespace sf
