// chunked_launch.h -- the one chunked launch behind every wave launcher (wave_launch.h, bwdtrans_rt.hip, iproduct.hip and
// the *_launch.h of the fused operators) and the occupancy cache it keeps per kernel.  Host code only: it declares no
// kernel, so a translation unit that includes it gains none.
#pragma once

#include "sf_dispatch.h" // launch_rc, device_info

#include <atomic>

namespace sf
{

constexpr int kMaxDev = 64;

// Persistent grid: as many workgroups as the device keeps resident (occupancy query, cached per
// device), never more than there are chunks.  The caches are atomics: two host threads that race on the first launch
// both run the query and store the same answer.
using OccCache = std::atomic<int>[kMaxDev];
template <class K> inline int resident_blocks(K kern, int threads, size_t lds, std::atomic<int> *cache)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDev)
        dev = 0;
    int cached = cache[dev].load(std::memory_order_acquire);
    if (cached == 0)
    {
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)kern,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        int bpc = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kern, threads, lds) != hipSuccess ||
            bpc < 1)
        {
            (void)hipGetLastError();
            bpc = 1;
        }
        cache[dev].store(bpc, std::memory_order_release);
        cached = bpc;
    }
    return cached * device_info().num_cu;
}

// The one chunked launch behind every wave launcher.
// A chunk is EC elements (1: the kernel counts elements), a workgroup has WPB waves; KMAP != 0: short-lived waves of
// |KMAP| chunks each on a grid that covers the batch; KMAP == 0: a persistent grid of the resident workgroups (or
// grid_override), never more than there are chunks.  `cache` is the occupancy cache of this kernel instantiation; the
// occupancy query runs on every path because it also raises the kernel's LDS limit, once per device.
template <int WPB, int EC, int KMAP, class K, class... A>
inline int launch_chunked(K kern, std::atomic<int> *cache, size_t lds, int grid_override, hipStream_t s, uint64_t nelmt,
                          A... args)
{
    if (nelmt == 0)
        return SF_OK;
    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const uint64_t per    = (uint64_t)WPB * (KMAP > 0 ? KMAP : (KMAP < 0 ? -KMAP : 1));
    const uint64_t need   = (nchunk + per - 1) / per;
    uint64_t grid         = (uint64_t)resident_blocks(kern, kWave * WPB, lds, cache);
    if (grid_override > 0)
        grid = (uint64_t)grid_override;
    if (grid > need || KMAP != 0)
        grid = need;
    if (grid > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)grid, kWave * WPB, lds, s>>>(args...);
    return launch_rc();
}

// The launch of the nq = 2 stream kernels: one thread per 16-byte output vector, workgroups of 256.
template <class K, class... A> inline int launch_stream(K kern, uint64_t nthreads, hipStream_t s, A... args)
{
    if (nthreads == 0)
        return SF_OK;
    const uint64_t blocks = (nthreads + 255) / 256;
    if (blocks > 0x7fffffffull)
        return SF_EINVAL;
    kern<<<(unsigned)blocks, 256, 0, s>>>(args...);
    return launch_rc();
}

} // namespace sf
