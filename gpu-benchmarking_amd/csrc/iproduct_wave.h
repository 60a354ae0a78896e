// iproduct_wave.h -- IProductWRTBase, the transpose of BwdTrans, as wave-per-chunk kernels for gfx950.
//
//   3D: out[e][r][q][p] = sum_k sum_j sum_i in[e][k][j][i] * B0[p][i] * B1[q][j] * B2[r][k]
//   2D: out[e][q][p]    = sum_j sum_i       in[e][j][i]    * B0[p][i] * B1[q][j]
//
// Same bases (row-major nm x nq), extents and element-major layouts as the BwdTrans kernels of bwdtrans_wave.h, with the
// roles of `in` (nq^d points per element) and `out` (nm^d modes per element) swapped.  Everything but the contraction is
// the BwdTrans machinery: one wavefront owns a chunk of EC elements, the chunk is fetched one chunk ahead into staging
// registers (chunk_fetch) and staged into the wave's LDS slab with odd pencil strides (chunk_stage), each sweep is "lane
// owns a pencil", and the chunk's output image leaves through the slab as one flat 16-byte-per-lane stream (OUT_LDS,
// chunk_flush) -- the only sensible output path, since nm^d is odd at every even order (343 at nq = 8).
//
// Sweep order i -> p (B0), then j -> q (B1), then k -> r (B2); each sum is taken in ascending index.  A sweep contracts a
// pencil of nq values into nm values with the DOT-PRODUCT form acc[p] = sum_i u[i] * B[p][i]: the caller's basis array is
// read as it is, row by row (row p = B[p][0 .. nq), contiguous), through the two-deep SGPR ring of contract() -- no
// transposed copy, no workspace, so every launch is capture-safe.
#pragma once

#include "bwdtrans_wave.h"

namespace sf
{

template <int NQ, int EC, int DIM, typename T = double> struct IprodGeom
{
    using Scalar = T;
    using Vec    = typename VecOf<T>::type;
    static constexpr int VW  = VecOf<T>::W;
    static constexpr int NM  = NQ - 1;
    static constexpr int NQP = NQ | 1; // padded pencil stride of the intermediates (odd number of scalars)
    static constexpr int NQT = (DIM == 3) ? NQ * NQ * NQ : NQ * NQ; // points per element (input)
    static constexpr int NMT = (DIM == 3) ? NM * NM * NM : NM * NM; // modes per element (output)
    // input pencils keep the global layout when NQ is odd (already conflict-free)
    static constexpr int IN_STRIDE = (NQ % 2 == 0) ? NQ + 1 : NQ;
    static constexpr int IN_DBL    = EC * NQT; // scalars per chunk read from HBM
    static constexpr bool VEC2     = (IN_DBL % VW) == 0;
    // pencils per chunk in each sweep
    static constexpr int P0 = (DIM == 3) ? EC * NQ * NQ : EC * NQ; // (e,k,j) | (e,j)
    static constexpr int P1 = (DIM == 3) ? EC * NM * NQ : EC * NM; // (e,p,k) | (e,p)
    static constexpr int P2 = EC * NM * NM;                       // (e,q,p)   (3D only)
    static constexpr int PASS0 = cdiv(P0, kWave);
    static constexpr int PASS1 = cdiv(P1, kWave);
    static constexpr int PASS2 = cdiv(P2, kWave);
    static constexpr int SLAB_IN = P0 * IN_STRIDE;
    static constexpr int SLAB_W1 = P1 * NQP;
    static constexpr int SLAB_W2 = (DIM == 3) ? P2 * NQP : 0;
    static constexpr int SLAB0   = CMax<CMax<SLAB_IN, SLAB_W1>::value, SLAB_W2>::value;
    static constexpr int OUT_DBL = EC * NMT; // scalars per chunk written to HBM
    // slab per wave (scalars): the three images and the output image, one after another, kept 16-B aligned
    static constexpr int SLAB = (CMax<SLAB0, OUT_DBL>::value + VW - 1) / VW * VW;
    static constexpr int NLD  = VEC2 ? cdiv(IN_DBL / VW, kWave) : cdiv(IN_DBL, kWave);
    static constexpr bool ALIGN_OK = VEC2 && cdiv(IN_DBL / VW + 7, kWave) == NLD;
};

// The view that the chunk I/O of bwdtrans_wave.h (chunk_fetch, chunk_stage, chunk_flush) takes of a geometry: there NM
// is the length of an input pencil and NMT the input scalars per element -- here they are NQ and NQT.
template <class G> struct IprodIo
{
    using Scalar = typename G::Scalar;
    using Vec    = typename G::Vec;
    static constexpr int VW = G::VW, NM = G::NM + 1, NMT = G::NQT, IN_DBL = G::IN_DBL, IN_STRIDE = G::IN_STRIDE;
    static constexpr int NLD = G::NLD, OUT_DBL = G::OUT_DBL;
    static constexpr bool VEC2 = G::VEC2, ALIGN_OK = G::ALIGN_OK;
};

template <int NQ, int EC, int DIM, int WPB, typename T = double> constexpr size_t iprod_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * IprodGeom<NQ, EC, DIM, T>::SLAB;
}

// ------------------------------------------------------------------------------------------------
// Dot-product contraction, columns [I0, I0+NB) of every basis row: acc[s][p] (+)= sum_i u[s][i] * B[p*NIN + i], ascending
// i (I0 == 0 starts the sums).  The rows go through a two-deep SGPR ring in the order of contract(): (1) touch row p (the
// wait for its scalar loads lands here), (2) request row p+1, (3) the FMAs of row p, (4) an order fence on row p's
// results, so that neither the next row's loads nor its FMAs move across.  BASIS_SMEM streams whole rows (NB = NIN);
// BASIS_SMEM_COLS{,16} take the rows in blocks of 8 / 16 columns, then the next block.
// ------------------------------------------------------------------------------------------------
template <int NIN, int NOUT, int NPASS, int I0, int KB, typename T>
__device__ __forceinline__ void contract_dot_cols(const T (&u)[NPASS][NIN], T (&acc)[NPASS][NOUT],
                                                  const T *__restrict__ bas, int &zero)
{
    constexpr int NB = (NIN - I0) < KB ? (NIN - I0) : KB;
    T b[2][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
        b[0][i] = bas[zero + I0 + i];
#pragma unroll
    for (int p = 0; p < NOUT; ++p)
    {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            asm volatile("" : "+s"(zero) : "s"(b[p % 2][i]));
        if (p + 1 < NOUT)
        {
#pragma unroll
            for (int i = 0; i < NB; ++i)
                b[(p + 1) % 2][i] = bas[zero + (p + 1) * NIN + I0 + i];
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            T a = (I0 == 0) ? u[s][0] * b[p % 2][0] : fma_t(u[s][I0], b[p % 2][0], acc[s][p]);
#pragma unroll
            for (int i = 1; i < NB; ++i)
                a = fma_t(u[s][I0 + i], b[p % 2][i], a);
            acc[s][p] = a;
        }
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
            asm volatile("" : "+s"(zero) : "v"(acc[s][p]));
    }
    if constexpr (I0 + NB < NIN)
        contract_dot_cols<NIN, NOUT, NPASS, I0 + NB, KB, T>(u, acc, bas, zero);
}

template <int NIN, int NOUT, int NPASS, int BMODE, typename T>
__device__ __forceinline__ void contract_dot(const T (&u)[NPASS][NIN], T (&acc)[NPASS][NOUT], const T *__restrict__ bas)
{
    static_assert(BMODE == BASIS_SMEM || BMODE == BASIS_SMEM_COLS || BMODE == BASIS_SMEM_COLS16,
                  "the transposed kernels take the basis as scalar operands");
    // opaque zero offset: the pointer stays a provably global kernel argument (s_load), the loads stay in the loop
    int zero = 0;
    asm volatile("s_mov_b32 %0, 0" : "=s"(zero));
    constexpr int KB = BMODE == BASIS_SMEM ? NIN : (BMODE == BASIS_SMEM_COLS ? 8 : 16);
    contract_dot_cols<NIN, NOUT, NPASS, 0, KB, T>(u, acc, bas, zero);
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_iprod_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G          = IprodGeom<NQ, EC, 3, T>;
    using IO         = IprodIo<G>;
    constexpr int NM = G::NM, NQP = G::NQP, NM2 = NM * NM, NQ2 = NQ * NQ;
    static_assert(OUTM == OUT_LDS, "the output (nm^3 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

        chunk_stage<IO, AL>(st, slab, lane,
                            IO::VEC2 ? (AL ? align_shift(in + c * IO::IN_DBL) : 0) : line_offset<T>(in + c * IO::IN_DBL));
        wave_lds_fence();
        if (n + 1 < it.count)
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, c + it.step, nelmt, lane);

        // ---- direction 0: w1[(e,p,k)][j] = sum_i in[(e,k,j)][i] * B0[p][i] ------------------------
        {
            T u[G::PASS0][NQ], acc[G::PASS0][NM];
            read_pencils<NQ, G::PASS0, G::P0, G::IN_STRIDE>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS0, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS0; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P0 || t < G::P0)
                {
                    const int e = t / NQ2, kj = t - e * NQ2, k = kj / NQ, j = kj - k * NQ;
                    T *dst = slab + (e * NM * NQ + k) * NQP + j;
#pragma unroll
                    for (int p = 0; p < NM; ++p)
                        dst[p * NQ * NQP] = acc[s][p];
                }
            }
            wave_lds_fence();
        }
        // ---- direction 1: w2[(e,q,p)][k] = sum_j w1[(e,p,k)][j] * B1[q][j] ------------------------
        {
            T u[G::PASS1][NQ], acc[G::PASS1][NM];
            read_pencils<NQ, G::PASS1, G::P1, NQP>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS1, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P1 || t < G::P1)
                {
                    const int e = t / (NM * NQ), pk = t - e * (NM * NQ), p = pk / NQ, k = pk - p * NQ;
                    T *dst = slab + (e * NM2 + p) * NQP + k;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NM * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
        }
        // ---- direction 2: out[e][r][(q,p)] = sum_k w2[(e,q,p)][k] * B2[r][k] ----------------------
        {
            T u[G::PASS2][NQ], acc[G::PASS2][NM];
            read_pencils<NQ, G::PASS2, G::P2, NQP>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS2, BMODE>(u, acc, b2);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS2; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P2 || t < G::P2)
                {
                    const int e = t / NM2, qp = t - e * NM2;
                    T *dst = slab + e * G::NMT + qp;
#pragma unroll
                    for (int r = 0; r < NM; ++r)
                        dst[r * NM2] = acc[s][r];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::NMT, lane);
            wave_lds_fence(); // slab is rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_iprod_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using G          = IprodGeom<NQ, EC, 2, T>;
    using IO         = IprodIo<G>;
    constexpr int NM = G::NM, NQP = G::NQP;
    static_assert(OUTM == OUT_LDS, "the output (nm^2 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;

    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;

    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;

        chunk_stage<IO, AL>(st, slab, lane,
                            IO::VEC2 ? (AL ? align_shift(in + c * IO::IN_DBL) : 0) : line_offset<T>(in + c * IO::IN_DBL));
        wave_lds_fence();
        if (n + 1 < it.count)
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, c + it.step, nelmt, lane);

        // ---- direction 0: w[(e,p)][j] = sum_i in[(e,j)][i] * B0[p][i] -----------------------------
        {
            T u[G::PASS0][NQ], acc[G::PASS0][NM];
            read_pencils<NQ, G::PASS0, G::P0, G::IN_STRIDE>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS0, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS0; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P0 || t < G::P0)
                {
                    const int e = t / NQ, j = t - e * NQ;
                    T *dst = slab + e * NM * NQP + j;
#pragma unroll
                    for (int p = 0; p < NM; ++p)
                        dst[p * NQP] = acc[s][p];
                }
            }
            wave_lds_fence();
        }
        // ---- direction 1: out[e][q][p] = sum_j w[(e,p)][j] * B1[q][j] -----------------------------
        {
            T u[G::PASS1][NQ], acc[G::PASS1][NM];
            read_pencils<NQ, G::PASS1, G::P1, NQP>(u, slab, lane);
            contract_dot<NQ, NM, G::PASS1, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < G::PASS1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= G::P1 || t < G::P1)
                {
                    const int e = t / NM, p = t - e * NM;
                    T *dst = slab + e * G::NMT + p;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NM] = acc[s][q];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)G::OUT_DBL, evalid * G::NMT, lane);
            wave_lds_fence();
        }
    }
}

} // namespace sf
