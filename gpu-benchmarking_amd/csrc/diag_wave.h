// diag_wave.h -- the diagonal of the fused Helmholtz operator as wave-per-chunk kernels for gfx950.
//
//   diag_e[r][q][p] = sum_kji lambda w_e[k][j][i] T0^0[p][i] T1^0[q][j] T2^0[r][k]
//                   + sum_c f_c sum_kji g_e[c][k][j][i] T0^{s0}[p][i] T1^{s1}[q][j] T2^{s2}[r][k]          (2D: without k, r)
//
// the diagonal of A_e = B^T [lambda diag(w_e) + sum_ab D_a^T diag(G_ab,e) D_b] B (helmholtz_wave.h).  T_d^t are the three
// tables of direction d that sf_diag_tables_* forms, tab_d[t][p][i] row-major nm x nq each: T^0 = B o B, T^1 = E o B,
// T^2 = E o E with E = B D^T the derivative of mode p at point i.  For the plane c = (a, b) of g: s_d = [d == a] +
// [d == b], f_c = 1 if a == b, else 2 (the symmetric pair is stored once).  Seven terms in 3D, four in 2D; every
// contraction is a transposed (IProductWRTBase-shaped) sweep, contract_dot() with the rows of a table as SGPR operands.
//
// There is no input chunk: no fetch, no stage.  The front is a metric stream like that of helmholtz_wave.h -- lane (e, j, i)
// reads g[e][c][k][j][i] and w[e][k][j][i], consecutive lanes consecutive scalars, every line once, non-temporal,
// unconditional loads (lanes without a point column, and lanes whose element lies beyond the batch, read the chunk's last
// valid column: in bounds, the same lines; what they compute never leaves the slab; nothing is read outside g or w;
// HASW = false compiles the w loads out).  Unlike there the ring holds whole k-pencils of PLANES, not slices of all planes
// (load_metric_slice does not fit and the loads are written out): a table row T[r][0 .. nq) is contiguous and goes through
// contract_dot() unchanged, where a slice would need a table COLUMN per step.  diag_ring() planes are in flight per lane;
// a plane's slot is refilled as soon as its pencil is contracted.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; an
// image is a separate sum, merges are additions; the any-extent kernel of diag_generic.hip follows it alike):
//   3D, the planes in the order of g, c = 0 .. 5 = (00, 01, 02, 11, 12, 22):
//   1. k -> r: A_c[r][j][i] = sum_k g_c[k][j][i] T2^{s2}[r][k]; A_1, A_2, A_4 are doubled (exact);
//      lambda != 0: A_5 = A_5 + sum_k (lambda w[k][j][i]) T2^0[r][k]                 (one merge: six images)
//   2. j -> q: S_c[r][q][i] = sum_j A_c[r][j][i] T1^{s1}[q][j], merged by direction-0 table in the order of the planes:
//      B^2 = S_0,  B^1 = S_1 + S_2,  B^0 = (S_3 + S_4) + S_5                          (three merges: three images)
//   3. i -> p: diag[r][q][p] = (sum_i B^0 T0^0[p][i] + sum_i B^1 T0^1[p][i]) + sum_i B^2 T0^2[p][i]      (two merges)
//   2D, the planes in REVERSE order, c = 2, 1, 0 = (11, 01, 00), so that the last sum reads the same:
//   1. j -> q: B^0[q][i] = sum_j g_2 T1^2[q][j] (lambda != 0: + sum_j (lambda w) T1^0[q][j]), B^1 = 2 sum_j g_1 T1^1[q][j],
//      B^2 = sum_j g_0 T1^0[q][j]
//   2. i -> p as step 3 above.
// The images go through the wave's slab ONE at a time and are never all alive: lane (e, j, i) contracts the pencil of a
// plane in registers (step 1), writes A_c to the slab as t2[(e,r,i)][j], lanes (e, r, i) sweep it (step 2) and add it to
// their register image B^{s0}; the three B images then go through the slab as t1[(e,r,q)][i] (frag/sweep_store.inc with
// M::SwT1), lanes (e, r, q) sweep them (step 3) and add; the result leaves through the back of the mass kernel (the
// output image, chunk_flush, the flat 16-byte stream).  2D: lane (e, i) contracts a plane's j-pencil, the image goes to
// the slab as t1[(e,q)][i], lanes (e, q) sweep and add.  frag/transposed_last_*.inc and frag/transposed0.inc do not fit
// (a merge or a doubling sits between their contraction and their store, and the last sweep is a sum of three): those
// sweeps are written out here, in the fragments' layouts.
#pragma once

#include "mass_wave.h"

#include <type_traits>

namespace sf
{

// f(integral_constant<int, I>) for I = FROM .. TO-1, written out at compile time: the walks over the planes index the
// ring with constants (a `#pragma unroll` loop that the unroller gives up on -- 2D nq 15 / 16 with the mass term -- leaves
// the ring in scratch)
template <int FROM, int TO, class F> __device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (FROM < TO)
    {
        f(std::integral_constant<int, FROM>{});
        static_for<FROM + 1, TO>(f);
    }
}

// planes in flight per lane: three pencils while one pass of columns holds them, two otherwise
template <int NPASS> constexpr int diag_ring()
{
    return NPASS > 1 ? 2 : 3;
}

template <int NQ, int EC, int DIM, typename T = double> struct DiagGeom
{
    using M      = MassGeom<NQ, EC, DIM, T>; // the transposed half: pencil counts, SwT1, the output image
    using F      = typename M::F;
    using Scalar = T;
    static constexpr int VW    = VecOf<T>::W;
    static constexpr int NM    = NQ - 1;
    static constexpr int NQP   = NQ | 1;
    static constexpr int NP    = (DIM == 3) ? EC * NQ * NQ : EC * NQ; // point columns of the first contraction
    static constexpr int NPASS = cdiv(NP, kWave);
    static constexpr int NCOMP = (DIM == 3) ? 6 : 3;
    static constexpr int RING  = diag_ring<NPASS>();
    // the transposed intermediates and the output image; no input image, no forward half
    static constexpr int SLAB = (CMax<M::SLAB_T, M::OUT_DBL>::value + VW - 1) / VW * VW;
    static_assert(sizeof(T) * SLAB <= 16 * 1024, "slab per wave");
};

template <int NQ, int EC, int DIM, int WPB, typename T = double> constexpr size_t diag_lds_bytes()
{
    return sizeof(T) * (size_t)WPB * DiagGeom<NQ, EC, DIM, T>::SLAB;
}

// the pencil of one plane along the walked index: u[s][n] = base[off[s] + n*STEP]; off is in bounds for every lane
template <int NQ, int NPASS, int STEP, typename T>
__device__ __forceinline__ void load_plane_pencil(T (&u)[NPASS][NQ], const T *__restrict__ base, const int (&off)[NPASS])
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
#pragma unroll
        for (int n = 0; n < NQ; ++n)
            u[s][n] = __builtin_nontemporal_load(base + off[s] + n * STEP);
}

// b = first ? a : b + a
template <int NPASS, int N, typename T>
__device__ __forceinline__ void merge_image(bool first, T (&b)[NPASS][N], const T (&a)[NPASS][N])
{
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
#pragma unroll
        for (int n = 0; n < N; ++n)
            b[s][n] = first ? a[s][n] : b[s][n] + a[s][n];
}

// The last sweep i -> p of one image B^{s0}, both dimensions: the image sits in the slab as t1[t][i], pencil stride NQP,
// t = (e,r,q) (quad: (e,q)); o = first ? sum : o + sum.
template <class M, int NQ, int NM, int NQP, int BMODE, typename T>
__device__ __forceinline__ void diag_sweep_i(bool first, T (&o)[M::PASST1][NM], const T *slab, const T *__restrict__ tab,
                                             int lane)
{
    T u[M::PASST1][NQ], res[M::PASST1][NM];
    read_pencils<NQ, M::PASST1, M::PT1, NQP>(u, slab, lane);
    contract_dot<NQ, NM, M::PASST1, BMODE>(u, res, tab);
    merge_image<M::PASST1, NM>(first, o, res);
}

// the output image out[t][p] and the chunk's way out (the tail of frag/transposed0.inc behind a sum of three sweeps)
template <class M, class IO, int NM, int MEMF, typename T>
__device__ __forceinline__ void diag_flush(const T (&o)[M::PASST1][NM], T *slab, T *__restrict__ out, uint64_t c, int evalid,
                                           int lane)
{
    wave_lds_fence();
#pragma unroll
    for (int s = 0; s < M::PASST1; ++s)
    {
        const int t = s * kWave + lane;
        if ((s + 1) * kWave <= M::PT1 || t < M::PT1)
        {
            T *dst = slab + t * NM;
#pragma unroll
            for (int p = 0; p < NM; ++p)
                dst[p] = o[s][p];
        }
    }
    wave_lds_fence();
    chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)M::OUT_DBL, evalid * M::NMT, lane);
    wave_lds_fence();
}

// the tables of the 3D planes in the order of g, (00, 01, 02, 11, 12, 22)
constexpr int diag_s2(int c)
{
    return c == 5 ? 2 : ((c == 2 || c == 4) ? 1 : 0);
}
constexpr int diag_s1(int c)
{
    return c == 3 ? 2 : ((c == 1 || c == 4) ? 1 : 0);
}
constexpr int diag_s0(int c)
{
    return c == 0 ? 2 : ((c == 1 || c == 2) ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_diag_wave_kernel(
    const T *__restrict__ t0, const T *__restrict__ t1, const T *__restrict__ t2, const T *__restrict__ g,
    const T *__restrict__ w, T lam, T *__restrict__ out, uint64_t nelmt)
{
    using G          = DiagGeom<NQ, EC, 3, T>;
    using M          = typename G::M;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ, TS = NM * NQ; // TS: one table
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // what frag/lane_roles_3d.inc asks for; no point image is kept here
    constexpr int NPL = HASW ? 7 : 6;          // the planes of g, then w
    static_assert(KMAP > 0, "short-lived waves only");
    static_assert(RING <= 6, "the ring is filled from the planes of g");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_3d.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        const T *gc = g + c * (uint64_t)(EC * G::NCOMP * NQT);
        const T *wc = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int goff[NPASS], woff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            goff[s]     = e * (G::NCOMP * NQT) + colp[s];
            woff[s]     = e * NQT + colp[s];
        }
        // the ring: the k-pencils of the first planes
        T pen[RING][NPASS][NQ];
#pragma unroll
        for (int r = 0; r < RING; ++r)
            load_plane_pencil<NQ, NPASS, NQ2>(pen[r], gc + r * NQT, goff);

        T acc[NPASS][NM];            // A_c of lane (e,j,i), over r
        T B[3][M::PASST2][NM] = {};  // B^{s0} of lane (e,r,i), over q
        static_for<0, NPL>([&](auto plc) __attribute__((always_inline)) {
            constexpr int pl = decltype(plc)::value;
            // ---- step 1, k -> r, out of the ring ---------------------------------------------------
            if (pl < 6)
            {
                contract_dot<NQ, NM, NPASS, BMODE>(pen[pl % RING], acc, t2 + diag_s2(pl) * TS);
                if (pl == 1 || pl == 2 || pl == 4)
                {
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
#pragma unroll
                        for (int r = 0; r < NM; ++r)
                            acc[s][r] = acc[s][r] + acc[s][r];
                }
            }
            else
            {
                T tmp[NPASS][NM];
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
#pragma unroll
                    for (int k = 0; k < NQ; ++k)
                        pen[pl % RING][s][k] = lam * pen[pl % RING][s][k];
                contract_dot<NQ, NM, NPASS, BMODE>(pen[pl % RING], tmp, t2);
                merge_image<NPASS, NM>(false, acc, tmp);
            }
            if (pl + RING < NPL)
            {
                if (pl + RING < 6)
                    load_plane_pencil<NQ, NPASS, NQ2>(pen[pl % RING], gc + (pl + RING) * NQT, goff);
                else
                    load_plane_pencil<NQ, NPASS, NQ2>(pen[pl % RING], wc, woff);
            }
            __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a plane
            if (pl == 5 && HASW)
                return; // A_5 waits for the mass term
            // ---- step 2, j -> q: A_c through the slab as t2[(e,r,i)][j], added to B^{s0} --------------
            constexpr int cc = pl < 6 ? pl : 5;
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ2, ji = t - e * NQ2, j = ji / NQ, i = ji - j * NQ;
                    T *dst = slab + (e * NM * NQ + i) * NQP + j;
#pragma unroll
                    for (int r = 0; r < NM; ++r)
                        dst[r * NQ * NQP] = acc[s][r];
                }
            }
            wave_lds_fence();
            {
                T u[M::PASST2][NQ], res[M::PASST2][NM];
                read_pencils<NQ, M::PASST2, M::PT2, NQP>(u, slab, lane);
                contract_dot<NQ, NM, M::PASST2, BMODE>(u, res, t1 + diag_s1(cc) * TS);
                merge_image<M::PASST2, NM>(cc == 0 || cc == 1 || cc == 3, B[diag_s0(cc)], res);
            }
        });
        // ---- step 3, i -> p: the three images through the slab as t1[(e,r,q)][i] -------------------------
        T o[M::PASST1][NM];
#pragma unroll
        for (int s0 = 0; s0 < 3; ++s0)
        {
            {
                T(&acc)[M::PASST2][NM] = B[s0];
#define SWEEP M::SwT1
#include "frag/sweep_store.inc"
            }
            diag_sweep_i<M, NQ, NM, NQP, BMODE>(s0 == 0, o, slab, t0 + s0 * TS, lane);
        }
        diag_flush<M, IO, NM, MEMF>(o, slab, out, c, evalid, lane);
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, bool HASW, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_diag_wave_kernel(
    const T *__restrict__ t0, const T *__restrict__ t1, const T *__restrict__ g, const T *__restrict__ w, T lam,
    T *__restrict__ out, uint64_t nelmt)
{
    using G          = DiagGeom<NQ, EC, 2, T>;
    using M          = typename G::M;
    using IO         = MassIo<M>;
    constexpr int NM = G::NM, NQP = G::NQP, NQT = NQ * NQ, TS = NM * NQ;
    constexpr int NPASS = G::NPASS, NP = G::NP, RING = G::RING;
    constexpr int ES  = NQ * NQP;      // what frag/lane_roles_2d.inc asks for
    constexpr int NPL = HASW ? 4 : 3;  // g_2 (11), [w], g_1 (01), g_0 (00)
    static_assert(KMAP > 0, "short-lived waves only");
    static_assert(RING <= 3, "the ring is filled from the planes of g or w");

#include "frag/wave_slab.inc"
#include "frag/wave_chunks.inc"
#include "frag/lane_roles_2d.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        const T *gc = g + c * (uint64_t)(EC * G::NCOMP * NQT);
        const T *wc = HASW ? w + c * (uint64_t)(EC * NQT) : nullptr;
        int goff[NPASS], woff[NPASS];
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            goff[s]     = e * (G::NCOMP * NQT) + colp[s];
            woff[s]     = e * NQT + colp[s];
        }
        // position pl of the walk -> plane of g (-1: w)
        auto plane = [](int pl) constexpr { return pl == 0 ? 2 : (HASW ? (pl == 1 ? -1 : 3 - pl) : 2 - pl); };
        T pen[RING][NPASS][NQ];
#pragma unroll
        for (int r = 0; r < RING; ++r)
        {
            if (plane(r) >= 0)
                load_plane_pencil<NQ, NPASS, NQ>(pen[r], gc + plane(r) * NQT, goff);
            else
                load_plane_pencil<NQ, NPASS, NQ>(pen[r], wc, woff);
        }

        T acc[NPASS][NM];     // B^{s0} of lane (e,i), over q
        T o[M::PASST1][NM];   // the diagonal of lane (e,q), over p
        static_for<0, NPL>([&](auto plc) __attribute__((always_inline)) {
            constexpr int pl = decltype(plc)::value;
            constexpr int cc = plane(pl);
            // ---- step 1, j -> q, out of the ring -----------------------------------------------------
            if (cc >= 0)
            {
                contract_dot<NQ, NM, NPASS, BMODE>(pen[pl % RING], acc, t1 + cc * TS); // plane c takes T1^c
                if (cc == 1)
                {
#pragma unroll
                    for (int s = 0; s < NPASS; ++s)
#pragma unroll
                        for (int q = 0; q < NM; ++q)
                            acc[s][q] = acc[s][q] + acc[s][q];
                }
            }
            else
            {
                T tmp[NPASS][NM];
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        pen[pl % RING][s][j] = lam * pen[pl % RING][s][j];
                contract_dot<NQ, NM, NPASS, BMODE>(pen[pl % RING], tmp, t1);
                merge_image<NPASS, NM>(false, acc, tmp);
            }
            if (pl + RING < NPL)
            {
                if (plane(pl + RING) >= 0)
                    load_plane_pencil<NQ, NPASS, NQ>(pen[pl % RING], gc + plane(pl + RING) * NQT, goff);
                else
                    load_plane_pencil<NQ, NPASS, NQ>(pen[pl % RING], wc, woff);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (pl == 0 && HASW)
                return; // B^0 waits for the mass term
            // ---- step 2, i -> p: B^{s0} through the slab as t1[(e,q)][i], s0 = 0, 1, 2 in this order ----
            constexpr int s0 = cc < 0 ? 0 : 2 - cc;
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ, i = t - e * NQ;
                    T *dst = slab + e * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
            diag_sweep_i<M, NQ, NM, NQP, BMODE>(s0 == 0, o, slab, t0 + s0 * TS, lane);
        });
        diag_flush<M, IO, NM, MEMF>(o, slab, out, c, evalid, lane);
    }
}

} // namespace sf
