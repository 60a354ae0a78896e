// wave_launch.h -- host-side launchers of the wave kernels (shared by the library and tools/sf_tune).
#pragma once

#include "bwdtrans_mfma.h"
#include "bwdtrans_mfma4.h"
#include "bwdtrans_hmfma4.h"
#include "bwdtrans_wave.h"
#include "chunked_launch.h"
#include "sf_dispatch.h" // counter_acquire (batch counter of the persistent 2D kernels)

namespace sf
{

// zeroes a launch's 64-byte slot of the counter ring (eight words; the kernel's batch counter is the first)
static __global__ void counter_reset_kernel(unsigned long long *ctr)
{
    __hip_atomic_store(ctr + threadIdx.x, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP = 0, int OUTM = OUT_ST8, int MEMF = 0,
          typename T = double>
inline int launch_hex_wave(const HexArgsT<T> &a, hipStream_t s, int grid_override = 0)
{
    static OccCache cache = {};
    constexpr size_t lds = wave_lds_bytes<NQ, EC, 3, WPB, BMODE, OUTM, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    return launch_chunked<WPB, EC, KMAP>(hex_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUTM, MEMF, T>, cache, lds,
                                         grid_override, s, a.nelmt, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
}

template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP = 0, int OUTM = OUT_ST8, int MEMF = 0,
          typename T = double>
inline int launch_quad_wave(const QuadArgsT<T> &a, hipStream_t s, int grid_override = 0)
{
    static OccCache cache = {};
    constexpr size_t lds = wave_lds_bytes<NQ, EC, 2, WPB, BMODE, OUTM, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    return launch_chunked<WPB, EC, KMAP>(quad_wave_kernel<NQ, EC, WPB, BMODE, MINW, KMAP, OUTM, MEMF, T>, cache, lds,
                                         grid_override, s, a.nelmt, a.b0, a.b1, a.in, a.out, a.nelmt);
}

template <int NQ, int EC, int WPB, int MINW, int KMAP, bool OUTL = false, int XG = 0, typename T = double>
inline int launch_quad_mfma(const QuadArgsT<T> &a, hipStream_t s, int grid_override = 0)
{
    static OccCache cache = {};
    constexpr size_t lds = mfma_lds_bytes<NQ, EC, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    return launch_chunked<WPB, EC, KMAP>(quad_mfma_kernel<NQ, EC, WPB, MINW, KMAP, OUTL, XG, T>, cache, lds,
                                         grid_override, s, a.nelmt, a.b0, a.b1, a.in, a.out, a.nelmt);
}

template <int NQ, int EB, int WPB, int MINW, int GJ, int KMAP, int XG, bool SHB, int DYNB, bool PEEL = true>
inline int launch_quad_mfma4_impl(const QuadArgs &a, hipStream_t s)
{
    static OccCache cache = {};
    auto kern            = quad_mfma4_kernel<NQ, EB, WPB, MINW, GJ, KMAP, XG, SHB, DYNB, PEEL>;
    constexpr size_t lds = mfma4_lds_bytes<NQ, EB, WPB, SHB>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    static_assert(DYNB == 0 || KMAP == 0, "the batch counter feeds a persistent grid");
    unsigned long long *ctr = nullptr;
    std::unique_lock<std::mutex> unit; // held from the acquire to the launch of the kernel that draws from the counter
    if constexpr (DYNB > 0)
    {
        // acquire + reset + launch are one enqueue unit (as scratch and launch are in bwdtrans_generic.hip): eager
        // launches on a stream share that stream's counter, so two host threads on one stream that enqueued reset,
        // reset, kernel, kernel would leave the second kernel a drained counter -- every wave draws "no batch" and the
        // output is never written
        unit = std::unique_lock<std::mutex>(counter_mutex());
        // the batch counter comes from the device's counter ring (never evicted: a pointer baked into a captured graph
        // stays valid until sf_shutdown); no counter to be had (ring exhausted, or first use inside a capture) -> the
        // same kernel with a fixed share per wave
        if (counter_acquire(s, &ctr) != SF_OK)
        {
            unit.unlock();
            return launch_quad_mfma4_impl<NQ, EB, WPB, MINW, GJ, KMAP, XG, SHB, 0, PEEL>(a, s);
        }
        // zeroed by a one-thread kernel, not a memset: under stream capture a memset node on a pointer INSIDE an
        // allocation did not zero the counter on ROCm 7.2 (the replayed grid then saw a stale ticket and exited)
        counter_reset_kernel<<<1, 8, 0, s>>>(ctr);
    }
    return launch_chunked<WPB, EB, KMAP>(kern, cache, lds, 0, s, a.nelmt, a.b0, a.b1, a.in, a.out, a.nelmt, ctr,
                                         (unsigned long long *)nullptr);
}

// SHBONLY: the configuration only fits the LDS with one basis copy (b0 == b1)
template <int NQ, int EB, int WPB, int MINW, int GJ, int KMAP, int XG = 0, bool SHBONLY = false, int DYNB = 0,
          bool PEEL = true>
inline int launch_quad_mfma4(const QuadArgs &a, hipStream_t s)
{
    if (a.nelmt == 0)
        return SF_OK;
    if (a.b0 == a.b1)
        return launch_quad_mfma4_impl<NQ, EB, WPB, MINW, GJ, KMAP, XG, true, DYNB, PEEL>(a, s);
    if constexpr (SHBONLY)
        return SF_ENOTBUILT;
    else
        return launch_quad_mfma4_impl<NQ, EB, WPB, MINW, GJ, KMAP, XG, false, DYNB, PEEL>(a, s);
}

template <int NQ, int EC, int WPB, int MINW, int KMAP, int XG = 0, typename T = double>
inline int launch_hex_mfma(const HexArgsT<T> &a, hipStream_t s, int grid_override = 0)
{
    static OccCache cache = {};
    constexpr size_t lds = hex_mfma_lds_bytes<NQ, EC, WPB, T>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    return launch_chunked<WPB, EC, KMAP>(hex_mfma_kernel<NQ, EC, WPB, MINW, KMAP, XG, T>, cache, lds, grid_override, s,
                                         a.nelmt, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt);
}

// one element per chunk
template <int NQ, int WPB, int MINW, int KMAP, int XG = 0, bool DIRECT = false, bool NTS = true, bool PEEL = true>
inline int launch_hex_mfma4(const HexArgs &a, hipStream_t s, int grid_override = 0)
{
    static OccCache cache = {};
    constexpr size_t lds = hex_mfma4_lds_bytes<NQ, WPB, DIRECT>();
    static_assert(lds <= 160 * 1024, "LDS slab exceeds 160 KiB");
    return launch_chunked<WPB, 1, KMAP>(hex_mfma4_kernel<NQ, WPB, MINW, KMAP, XG, false, DIRECT, NTS, PEEL>, cache, lds,
                                        grid_override, s, a.nelmt, a.b0, a.b1, a.b2, a.in, a.out, a.nelmt, nullptr);
}

} // namespace sf
