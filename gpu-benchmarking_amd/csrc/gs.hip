// gs.hip -- gather-scatter between element-local coefficients and global degrees of freedom: Q (global_to_local), Q^T
// (assemble) and Q Q^T (gs) of a local-to-global map, and the setup that inverts the map (include/sumfact.h: sf_gs_setup,
// sf_global_to_local_*, sf_assemble_*, sf_gs_*).  No float atomics: Q^T walks an inverted index -- per global degree of
// freedom, the list of its local coefficients in ascending order -- one lane per row, with plain loads and one store, so
// the sum has one fixed order and is bitwise reproducible.  The index is `rows` (nglobal words: row g is
// perm[rows[g-1] .. rows[g]), rows[-1] = 0) and `perm` (nlocal words); the setup builds it with integer atomics only.
#include "sf_dispatch.h"

namespace sf
{
namespace
{
constexpr int kGsThreads = 256;
// the scan's tile: kGsThreads lanes with kScanItems consecutive counts each
constexpr int kScanItems      = 8;
constexpr unsigned kScanTile  = kGsThreads * kScanItems;
constexpr int kGsWaves        = kGsThreads / kWave;

// ---- setup -------------------------------------------------------------------------------------------------------------
// rows[g] = number of local coefficients of g; an entry >= nglobal raises *bad and is counted nowhere
__global__ __launch_bounds__(kGsThreads) void gs_count_kernel(const int32_t *__restrict__ l2g, size_t nlocal,
                                                              unsigned nglobal, unsigned *__restrict__ rows,
                                                              unsigned *__restrict__ bad)
{
    const size_t i = (size_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (i >= nlocal)
        return;
    const int32_t g = l2g[i];
    if (g < 0)
        return;
    if ((unsigned)g >= nglobal)
        *bad = 1u; // every writer stores the same word
    else
        atomicAdd(rows + g, 1u);
}

// exclusive scan of one value per lane across the block; *total: the block's sum
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *total)
{
    __shared__ unsigned wave_sum[kGsWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d *= 2)
    {
        const unsigned up = __shfl_up(incl, d, kWave);
        if (lane >= d)
            incl += up;
    }
    __syncthreads(); // wave_sum of an earlier call has been read
    if (lane == kWave - 1)
        wave_sum[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kGsWaves; ++w)
    {
        before += w < wave ? wave_sum[w] : 0u;
        all += wave_sum[w];
    }
    *total = all;
    return before + incl - v;
}

// tile[b] = sum of the counts of tile b
__global__ __launch_bounds__(kGsThreads) void gs_tile_sum_kernel(const unsigned *__restrict__ rows, unsigned nglobal,
                                                                 unsigned *__restrict__ tile)
{
    const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    unsigned sum       = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        sum += first + k < nglobal ? rows[first + k] : 0u;
    unsigned total;
    (void)block_exclusive_scan(sum, &total);
    if (threadIdx.x == 0)
        tile[blockIdx.x] = total;
}

// tile[0 .. ntiles) -> its exclusive scan, in place: one block, kGsThreads entries per step
__global__ __launch_bounds__(kGsThreads) void gs_tile_scan_kernel(unsigned *__restrict__ tile, unsigned ntiles)
{
    unsigned carry = 0;
    for (unsigned base = 0; base < ntiles; base += kGsThreads)
    {
        const unsigned t = base + threadIdx.x;
        const unsigned v = t < ntiles ? tile[t] : 0u;
        unsigned total;
        const unsigned ex = block_exclusive_scan(v, &total);
        if (t < ntiles)
            tile[t] = carry + ex;
        carry += total;
    }
}

// rows[g] = the begin of row g: the exclusive scan of the counts, in place
__global__ __launch_bounds__(kGsThreads) void gs_scan_apply_kernel(unsigned *__restrict__ rows, unsigned nglobal,
                                                                   const unsigned *__restrict__ tile)
{
    const size_t first = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    unsigned c[kScanItems], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
    {
        c[k] = first + k < nglobal ? rows[first + k] : 0u;
        sum += c[k];
    }
    unsigned total;
    unsigned run = tile[blockIdx.x] + block_exclusive_scan(sum, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
    {
        if (first + k < nglobal)
            rows[first + k] = run;
        run += c[k];
    }
}

// perm[cursor of l2g[i]] = i; the cursor of row g starts at its begin and ends at its end, so that rows holds the row
// ends afterwards
__global__ __launch_bounds__(kGsThreads) void gs_fill_kernel(const int32_t *__restrict__ l2g, size_t nlocal,
                                                             unsigned nglobal, unsigned *__restrict__ rows,
                                                             int32_t *__restrict__ perm)
{
    const size_t i = (size_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (i >= nlocal)
        return;
    const int32_t g = l2g[i];
    if (g < 0 || (unsigned)g >= nglobal)
        return;
    const unsigned at = atomicAdd(rows + g, 1u);
    if (at < nlocal)
        perm[at] = (int32_t)i;
}

// the cursors filled each row in whatever order the atomics ran: put every row of two or more back in ascending order
// (one lane per row, insertion sort: the rows of a finite-element mesh hold a few dozen entries at most)
__global__ __launch_bounds__(kGsThreads) void gs_sort_kernel(const unsigned *__restrict__ rows, unsigned nglobal,
                                                             size_t nlocal, int32_t *__restrict__ perm)
{
    const size_t g = (size_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (g >= nglobal)
        return;
    const size_t begin = g ? rows[g - 1] : 0u, end = rows[g];
    if (end > nlocal) // a refused map: its rows are not looked at
        return;
    for (size_t k = begin + 1; k < end; ++k)
    {
        const int32_t key = perm[k];
        size_t j          = k;
        while (j > begin)
        {
            const int32_t left = perm[j - 1];
            if (left <= key)
                break;
            perm[j] = left;
            --j;
        }
        if (j != k)
            perm[j] = key;
    }
}

// ---- Q: local[i] = sign[i] global[l2g[i]], 0 where l2g[i] < 0 ----------------------------------------------------------
// Four coefficients per lane, kGsThreads apart: every load, gather and store of a wave covers 64 CONSECUTIVE coefficients.
// The four are independent (four gathers in flight per lane), and a wave's gather touches the few lines that 64
// neighbouring coefficients map to.  The streams read or written once (l2g, sign, local) are non-temporal; the gathers
// are plain loads, so that they stay in L1 / L2 -- neighbouring elements read the same faces again.  Scalar accesses
// only: nothing to peel, any scalar alignment runs the same kernel.  (Four CONSECUTIVE coefficients per lane behind one
// 16-byte load of the map spread a wave's gather over 256 coefficients and four times the lines: 0.41 ms against 0.27 on
// the 64^3 hex mesh in fp64.)
constexpr int kG2lPerLane = 4;
template <typename T, bool SIGN>
__global__ __launch_bounds__(kGsThreads) void gs_g2l_kernel(size_t nlocal, const int32_t *__restrict__ l2g,
                                                            const T *__restrict__ sign, const T *__restrict__ global,
                                                            T *__restrict__ local)
{
    const size_t base = (size_t)blockIdx.x * (kGsThreads * kG2lPerLane) + threadIdx.x;
    int32_t g[kG2lPerLane];
    T v[kG2lPerLane];
#pragma unroll
    for (int c = 0; c < kG2lPerLane; ++c)
    {
        const size_t i = base + (size_t)c * kGsThreads;
        g[c]           = i < nlocal ? __builtin_nontemporal_load(l2g + i) : -1;
    }
#pragma unroll
    for (int c = 0; c < kG2lPerLane; ++c)
        v[c] = g[c] < 0 ? (T)0 : global[(size_t)g[c]];
#pragma unroll
    for (int c = 0; c < kG2lPerLane; ++c)
    {
        const size_t i = base + (size_t)c * kGsThreads;
        if (i >= nlocal)
            continue;
        if constexpr (SIGN)
            v[c] *= __builtin_nontemporal_load(sign + i);
        __builtin_nontemporal_store(v[c], local + i);
    }
}

// ---- Q^T and Q Q^T: one lane per global row, consecutive lanes on consecutive rows -------------------------------------
template <typename T, bool SIGN>
__device__ __forceinline__ T signed_term(const T *__restrict__ sign, const T *local, size_t i)
{
    if constexpr (SIGN)
        return sign[i] * local[i];
    else
        return local[i];
}

// the row's terms added in ascending position, starting from the first
template <typename T, bool SIGN>
__device__ __forceinline__ T row_sum(const int32_t *__restrict__ perm, const T *__restrict__ sign, const T *local,
                                     size_t begin, size_t end)
{
    T acc = signed_term<T, SIGN>(sign, local, (size_t)perm[begin]);
    for (size_t k = begin + 1; k < end; ++k)
        acc += signed_term<T, SIGN>(sign, local, (size_t)perm[k]);
    return acc;
}

template <typename T, bool SIGN>
__global__ __launch_bounds__(kGsThreads) void gs_assemble_kernel(size_t nglobal, const int32_t *__restrict__ rows,
                                                                 const int32_t *__restrict__ perm,
                                                                 const T *__restrict__ sign, const T *__restrict__ local,
                                                                 T *__restrict__ global)
{
    const size_t g = (size_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (g >= nglobal)
        return;
    const size_t begin = g ? (size_t)rows[g - 1] : 0, end = (size_t)rows[g];
    global[g]          = begin < end ? row_sum<T, SIGN>(perm, sign, local, begin, end) : (T)0;
}

// in place: a row of one or none is left alone (only `rows` is read for it); the rows are disjoint
template <typename T, bool SIGN>
__global__ __launch_bounds__(kGsThreads) void gs_gs_kernel(size_t nglobal, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ perm, const T *__restrict__ sign,
                                                           T *local)
{
    const size_t g = (size_t)blockIdx.x * kGsThreads + threadIdx.x;
    if (g >= nglobal)
        return;
    const size_t begin = g ? (size_t)rows[g - 1] : 0, end = (size_t)rows[g];
    if (end < begin + 2)
        return;
    const T sum = row_sum<T, SIGN>(perm, sign, local, begin, end);
    for (size_t k = begin; k < end; ++k)
    {
        const size_t i = (size_t)perm[k];
        if constexpr (SIGN)
            local[i] = sign[i] * sum;
        else
            local[i] = sum;
    }
}

inline unsigned blocks_for(size_t n, size_t per_block)
{
    return (unsigned)((n + per_block - 1) / per_block);
}
} // namespace

int gs_setup(size_t nlocal, size_t nglobal, const int32_t *l2g, int32_t *rows, int32_t *perm, hipStream_t s)
{
    unsigned *r          = reinterpret_cast<unsigned *>(rows);
    const unsigned ng    = (unsigned)nglobal;
    const unsigned tiles = blocks_for(nglobal, kScanTile);
    unsigned bad         = 0;
    hipError_t e;
    {
        // the scratch (the scan's tile sums and the flag of a refused map) is this stream's from here to the copy
        std::lock_guard<std::recursive_mutex> lock(scratch_mutex());
        void *p = nullptr;
        int rc  = scratch_acquire(s, 2, sizeof(unsigned) * ((size_t)tiles + 1), &p);
        if (rc != SF_OK)
            return rc;
        unsigned *tile = static_cast<unsigned *>(p), *flag = tile + tiles;
        e = hipMemsetAsync(rows, 0, sizeof(int32_t) * nglobal, s);
        if (e == hipSuccess) // the words of perm that no row owns (one per negative entry) are -1: the same bytes every time
            e = hipMemsetAsync(perm, 0xff, sizeof(int32_t) * nlocal, s);
        if (e == hipSuccess)
            e = hipMemsetAsync(flag, 0, sizeof(unsigned), s);
        if (e != hipSuccess)
            return (int)e;
        const unsigned lblocks = blocks_for(nlocal, kGsThreads);
        gs_count_kernel<<<lblocks, kGsThreads, 0, s>>>(l2g, nlocal, ng, r, flag);
        gs_tile_sum_kernel<<<tiles, kGsThreads, 0, s>>>(r, ng, tile);
        gs_tile_scan_kernel<<<1, kGsThreads, 0, s>>>(tile, tiles);
        gs_scan_apply_kernel<<<tiles, kGsThreads, 0, s>>>(r, ng, tile);
        gs_fill_kernel<<<lblocks, kGsThreads, 0, s>>>(l2g, nlocal, ng, r, perm);
        gs_sort_kernel<<<blocks_for(nglobal, kGsThreads), kGsThreads, 0, s>>>(r, ng, nlocal, perm);
        rc = launch_rc();
        if (rc != SF_OK)
            return rc;
        e = hipMemcpyAsync(&bad, flag, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s); // blocking, and `bad` is pageable: waited for under the lock
    }
    if (e != hipSuccess)
        return (int)e;
    return bad ? SF_EINVAL : SF_OK;
}

template <typename T>
int launch_global_to_local(size_t nlocal, const int32_t *l2g, const T *sign, const T *global, T *local, hipStream_t s)
{
    const unsigned blocks = blocks_for(nlocal, (size_t)kGsThreads * kG2lPerLane);
    if (sign)
        gs_g2l_kernel<T, true><<<blocks, kGsThreads, 0, s>>>(nlocal, l2g, sign, global, local);
    else
        gs_g2l_kernel<T, false><<<blocks, kGsThreads, 0, s>>>(nlocal, l2g, sign, global, local);
    return launch_rc();
}

template <typename T>
int launch_assemble(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, const T *local, T *global,
                    hipStream_t s)
{
    const unsigned blocks = blocks_for(nglobal, kGsThreads);
    if (sign)
        gs_assemble_kernel<T, true><<<blocks, kGsThreads, 0, s>>>(nglobal, rows, perm, sign, local, global);
    else
        gs_assemble_kernel<T, false><<<blocks, kGsThreads, 0, s>>>(nglobal, rows, perm, sign, local, global);
    return launch_rc();
}

template <typename T>
int launch_gs(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, T *local, hipStream_t s)
{
    const unsigned blocks = blocks_for(nglobal, kGsThreads);
    if (sign)
        gs_gs_kernel<T, true><<<blocks, kGsThreads, 0, s>>>(nglobal, rows, perm, sign, local);
    else
        gs_gs_kernel<T, false><<<blocks, kGsThreads, 0, s>>>(nglobal, rows, perm, sign, local);
    return launch_rc();
}

template int launch_global_to_local<double>(size_t, const int32_t *, const double *, const double *, double *, hipStream_t);
template int launch_global_to_local<float>(size_t, const int32_t *, const float *, const float *, float *, hipStream_t);
template int launch_assemble<double>(size_t, const int32_t *, const int32_t *, const double *, const double *, double *,
                                     hipStream_t);
template int launch_assemble<float>(size_t, const int32_t *, const int32_t *, const float *, const float *, float *,
                                    hipStream_t);
template int launch_gs<double>(size_t, const int32_t *, const int32_t *, const double *, double *, hipStream_t);
template int launch_gs<float>(size_t, const int32_t *, const int32_t *, const float *, float *, hipStream_t);
} // namespace sf
