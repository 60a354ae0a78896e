// mass_wave.h -- the fused mass operator y_e = B^T diag(w_e) B x_e as wave-per-chunk kernels for gfx950.
//
//   3D: out[e][r'][q'][p'] = sum_kji B0[p'][i] B1[q'][j] B2[r'][k] * w[e][k][j][i] * (sum_rqp in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k])
//   2D: out[e][q'][p']     = sum_ji  B0[p'][i] B1[q'][j]           * w[e][j][i]    * (sum_qp  in[e][q][p]    B0[p][i] B1[q][j])
//
// BwdTrans (bwdtrans_wave.h), a pointwise weight and IProductWRTBase (iproduct_wave.h) in ONE kernel: the quadrature-space
// image (nq^d values per element) never exists in HBM, and in 3D not even in LDS.  `in` and `out` hold nm^d modes per
// element (p fastest, the BwdTrans input layout), `w` nq^d values per element (i fastest, the BwdTrans output layout).
// Same bases (row-major nm x nq), same machinery as the two halves, reused by inclusion: one wavefront owns a chunk of
// EC elements, no workgroup barrier, the chunk's input is fetched one chunk ahead (chunk_fetch / chunk_stage), every
// sweep is "lane owns a pencil", the basis rows go through the SGPR ring of contract() / contract_dot(), and the nm^d
// output image leaves through the slab as one flat 16-byte-per-lane stream (chunk_flush).
//
// Sweep order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   forward     p -> i (B0), q -> j (B1), r -> k (B2)        -- the BwdTrans order
//   weight      one multiply per point
//   transposed  k -> r' (B2), j -> q' (B1), i -> p' (B0)     -- the reverse of the forward order
// After the last forward sweep lane t = (e, j, i) holds the k-pencil of its point column in registers; the weights are
// multiplied in there and the first transposed sweep (k -> r') contracts the same registers: no LDS round trip at the
// hand-over.  (2D: lane (e, i) holds the j-pencil; the first transposed sweep is j -> q'.)
//
// Weights: lane (e, j, i) loads w[e][k][j][i], k = 0 .. nq-1, straight from global memory into registers at the top of
// the chunk, right after the input is staged (non-temporal: w is streamed once), so the latency hides behind the
// forward sweeps.  Consecutive lanes read consecutive scalars (runs of nq^2 in 3D -- the whole wave at one element per
// chunk -- and of nq in 2D), every line is fetched from HBM once.  `w` needs only scalar alignment and never touches
// LDS.  Lanes without a point column (t >= P2) or whose element lies beyond the batch (e >= evalid, last chunk) issue
// NO load: w ends where the batch ends.
//
// LDS per chunk, 3D: 6 images (input, two forward intermediates, two transposed intermediates, output) against the 8 of
// the two separate kernels.  The slab is the maximum over them and never exceeds the IProductWRTBase slab of the order.
//
// Shared text.  The front and the back of a fused wave kernel are the same text in every operator built on this one
// (helmholtz_wave.h, affine_wave.h, physderiv_wave.h, iprodderiv_wave.h).  That text lives once, in csrc/frag/*.inc:
// plain kernel-body text that a kernel #includes at the place it runs, so the compiler sees one body per kernel, as if
// it were written out (helper functions changed the code of tuned instantiations, DESIGN s9 item 7).  Every fragment
// opens with its contract: what it computes, the names it expects in scope and declares, the slab before and after.
// The names the kernels agree on: G the geometry whose SLAB the wave owns, M the MassGeom (transposed half, output), F
// the WaveGeom (forward half), IO the chunk I/O view (IN_LEN, IN_ELEM, IN_DBL, IN_STRIDE, NLD, OUT_DBL, VEC2, ALIGN_OK:
// a SweepGeom has them, MassIo takes them from F and M); NP / NPASS the point columns per chunk and their passes.  A
// kernel below reads as its own lines between the includes:
//   wave_slab, wave_chunks, chunk_fetch_first | per chunk: chunk_head, chunk_stage, [the weight loads],
//   chunk_fetch_next, forward0, forward1_3d, [last forward sweep, weight, first transposed sweep],
//   transposed1_3d, transposed0 (which ends with chunk_flush and the closing fence).
// forward0, forward1_3d and transposed1_3d are instances of frag/sweep.inc, the one sweep text of the wave kernels
// (bwdtrans_wave.h): each names its Sweep (F::Sw0, F::Sw1, M::SwT1), its contraction and its basis.  The kernels that
// have one chunk per wave and no loop (bwdtrans_aniso.h) open with wave_slab, wave_one_chunk.
#pragma once

#include "iproduct_wave.h"

namespace sf
{

template <int NQ, int EC, int DIM, typename T = double> struct MassGeom
{
    using F      = WaveGeom<NQ, EC, DIM, T>; // the forward half: input image and forward intermediates
    using Scalar = T;
    using Vec    = typename VecOf<T>::type;
    static constexpr int VW  = VecOf<T>::W;
    static constexpr int NM  = NQ - 1;
    static constexpr int NQP = NQ | 1; // padded pencil stride of the transposed intermediates (odd number of scalars)
    static constexpr int NMT = F::NMT, NQT = F::NQT;
    // pencils per chunk of the transposed sweeps: 3D (e,j,i) -> (e,r',i) -> (e,r',q'); 2D (e,i) -> (e,q')
    static constexpr int PT2 = (DIM == 3) ? EC * NM * NQ : 0;       // pencils over j, read by the sweep j -> q' (3D only)
    static constexpr int PT1 = (DIM == 3) ? EC * NM * NM : EC * NM; // pencils over i, read by the sweep i -> p'
    static constexpr int PASST2 = cdiv(PT2 > 0 ? PT2 : 1, kWave);
    static constexpr int PASST1 = cdiv(PT1, kWave);
    using SwT1 = Sweep<NQ, NM, PT2, NQP, 1, NQ, NQP>; // the sweep j -> q' (3D only): (e,r') in the place of e
    static constexpr int SLAB_T = CMax<PT2, PT1>::value * NQP;
    static constexpr int OUT_DBL = EC * NMT; // scalars per chunk written to HBM
    static constexpr int SLAB =
        (CMax<CMax<F::SLAB0, SLAB_T>::value, OUT_DBL>::value + VW - 1) / VW * VW;
    static_assert(SLAB <= IprodGeom<NQ, EC, DIM, T>::SLAB, "the fused slab stays within the IProductWRTBase slab");
};

// The view that the chunk I/O of bwdtrans_wave.h takes of the geometry: the input side of BwdTrans on both ends.  (A
// SweepGeom is its own view; this one joins the forward half's input to the transposed half's output.)
template <class G> struct MassIo
{
    using F      = typename G::F;
    using Scalar = typename G::Scalar;
    using Vec    = typename G::Vec;
    static constexpr int VW = G::VW, IN_LEN = F::IN_LEN, IN_ELEM = F::IN_ELEM, IN_DBL = F::IN_DBL, IN_STRIDE = F::IN_STRIDE;
    static constexpr int NLD = F::NLD, OUT_DBL = G::OUT_DBL;
    static constexpr bool VEC2 = F::VEC2, ALIGN_OK = F::ALIGN_OK;
};

template <int NQ, int EC, int DIM, int WPB, typename T = double> constexpr size_t mass_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * MassGeom<NQ, EC, DIM, T>::SLAB;
}

// Weights of this lane's point columns: wv[s][n] = w[e][n][pl] for column t = s*64 + lane = (e, pl), pl < PLANE, the n
// of one lane PLANE scalars apart.  Lanes with t >= NP or e >= evalid load nothing and hold zeros.
template <int NQ, int NPASS, int NP, int PLANE, typename T>
__device__ __forceinline__ void load_weights(T (&wv)[NPASS][NQ], const T *__restrict__ wc, int evalid, int lane)
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t = s * kWave + lane;
        const int e = t / PLANE, pl = t - e * PLANE;
#pragma unroll
        for (int n = 0; n < NQ; ++n)
            wv[s][n] = T(0);
        if (((s + 1) * kWave <= NP || t < NP) && e < evalid)
        {
            const T *src = wc + e * (NQ * PLANE) + pl;
#pragma unroll
            for (int n = 0; n < NQ; ++n)
                wv[s][n] = __builtin_nontemporal_load(src + n * PLANE);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_mass_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ w,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt)
{
    using M          = MassGeom<NQ, EC, 3, T>;
    using G          = M; // the slab is the mass slab
    using F          = typename M::F;
    using IO         = MassIo<M>;
    constexpr int NM = M::NM, NMP = F::NMP, NQP = M::NQP, NQ2 = NQ * NQ;
    constexpr int NPASS = F::PASS2, NP = F::P2; // the point columns (e,j,i)
    static_assert(OUTM == OUT_LDS, "the output (nm^3 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // This chunk's weights, requested as soon as the staging registers are consumed: in flight under the three
        // forward sweeps.  (Requested above chunk_stage they would be waited for there: behind the conditional loads
        // hipcc no longer counts and emits s_waitcnt vmcnt(0) for the staging registers.)
        T wv[NPASS][NQ];
        load_weights<NQ, NPASS, NP, NQ2>(wv, w + c * (uint64_t)(EC * M::NQT), evalid, lane);
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
#include "frag/forward1_3d.inc"
        // ---- at the points (forward 2, the weight, transposed 2): lane (e,j,i) keeps its k-pencil in registers ----
        //      v[k] = w[e][k][j][i] * sum_r w2[(e,j,i)][r] * B2[r][k];  t2[(e,r',i)][j] = sum_k v[k] * B2[r'][k]
        {
            T u[NPASS][NQ], acc[NPASS][NM];
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b2);
            }
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int k = 0; k < NQ; ++k)
                    u[s][k] *= wv[s][k];
            // The sweep of frag/transposed_last_3d.inc, written out: with its guard taken from an own[] array the assembly
            // of 18 of the 52 mass instantiations changes (at nq 2 the pairing of the LDS stores).
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b2);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= NP || t < NP)
                {
                    const int e = t / NQ2, ji = t - e * NQ2, j = ji / NQ, i = ji - j * NQ;
                    T *dst = slab + (e * NM * NQ + i) * NQP + j;
#pragma unroll
                    for (int r = 0; r < NM; ++r)
                        dst[r * NQ * NQP] = acc[s][r];
                }
            }
            wave_lds_fence();
        }
#include "frag/transposed1_3d.inc"
#include "frag/transposed0.inc"
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int OUTM, int MEMF = 0, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_mass_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ w, const T *__restrict__ in,
    T *__restrict__ out, uint64_t nelmt)
{
    using M          = MassGeom<NQ, EC, 2, T>;
    using G          = M; // the slab is the mass slab
    using F          = typename M::F;
    using IO         = MassIo<M>;
    constexpr int NM = M::NM, NMP = F::NMP, NQP = M::NQP;
    constexpr int NPASS = F::PASS1, NP = F::P1; // the point columns (e,i)
    static_assert(OUTM == OUT_LDS, "the output (nm^2 per element) leaves through the LDS stream");
    static_assert(KMAP > 0, "short-lived waves only");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/chunk_fetch_first.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
#include "frag/chunk_stage.inc"
        // this chunk's weights (after the staging registers are consumed, see the 3D kernel): lane (e,i) takes
        // w[e][j][i], j = 0 .. nq-1
        T wv[NPASS][NQ];
        load_weights<NQ, NPASS, NP, NQ>(wv, w + c * (uint64_t)(EC * M::NQT), evalid, lane);
#include "frag/chunk_fetch_next.inc"
#include "frag/forward0.inc"
        // ---- at the points (forward 1, the weight, transposed 1): lane (e,i) keeps its j-pencil in registers ----
        //      v[j] = w[e][j][i] * sum_q w1[(e,i)][q] * B1[q][j];  t1[(e,q')][i] = sum_j v[j] * B1[q'][j]
        {
            T u[NPASS][NQ], acc[NPASS][NM];
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b1);
            }
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    u[s][j] *= wv[s][j];
            // the sweep of frag/transposed_last_2d.inc, written out for the same reason as in the 3D kernel
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= NP || t < NP)
                {
                    const int e = t / NQ, i = t - e * NQ;
                    T *dst = slab + e * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
        }
#include "frag/transposed0.inc"
    }
}

} // namespace sf
