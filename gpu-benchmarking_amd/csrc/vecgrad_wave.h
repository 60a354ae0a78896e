// vecgrad_wave.h -- the gradient, divergence and curl of a vector field at the quadrature points, as wave-per-chunk
// kernels for gfx950.
//
//   u_a = B in_a,   J[a][b] = D_b u_a,   grad[a][j] = sum_b df[j*d + b] J[a][b] = d u_a / d x_j      (a, b, j = 0 .. d-1)
//   div = grad[0][0] + grad[1][1] [+ grad[2][2]]
//   3D: curl0 = grad[2][1] - grad[1][2],  curl1 = grad[0][2] - grad[2][0],  curl2 = grad[1][0] - grad[0][1]
//   2D: curl0 = grad[1][0] - grad[0][1]
//
// B the tensor-product BwdTrans basis, D_b the collocation derivative matrix of direction b, df the d*d planes of the
// inverse Jacobian (c = a*d + b for d xi_b / d x_a, the layout of physderiv_wave.h), in_a the nm^d modes of field a of the
// element.  grad[e][c][k][j][i] holds d*d planes per element in the layout of df, c = a*d + j; div and curl_n are one
// plane per element each, laid out like the output of BwdTrans.  No point image reaches HBM but the outputs.
// The front is the unit of one coordinate of geom_wave.h, frag/geom_coordinate_{2d,3d}.inc, once per field with GEOM_X =
// in_a over the slab of GeomGeom (the images of the fields 0 .. d-2 kept behind the front's slab), as advect_wave.h with
// NF = d: dk[a] is the register pencil d u_a / d xi_(d-1) of the column's lane and holds the bits it holds there.  The
// ring of df is that of physderiv_wave.h (load_df_slice), the stores are those of geom_wave.h.
// Shared text (csrc/frag/*.inc, the sequence geom_wave.h lists): wave_open; per chunk chunk_head, ring_offsets (the ring's
// clamped column offsets), fields_front_{2d,3d} with the ring primed in front of the last field's unit; in the walk
// walk_stores, point_jacobian_{2d,3d} and planes_store (grad).  This header's own: the ring and the arithmetic of the
// walk.
//
// Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
//   1. forward sweeps p -> i, q -> j, r -> k of in_a                              (u_a, the point values)
//   2. J[a][b] = D_b u_a
//   3. grad[a][j] = sum_b df[j*d + b] J[a][b], b ascending          (step 3 of physderiv_wave.h applied to field a)
//   4. div: plain additions of the rounded entries, a ascending
//   5. curl: plain subtractions of the rounded entries
//
// The walk.  Lane (e, j, i) walks k (2D: lane (e, i) walks j).  Per slice it takes the d*d values of df of its point
// from a ring of kHelmRing slices, reads the image entries of J, forms the d*d entries of grad and stores what is asked
// for.  The loads of the ring are non-temporal and unconditional: lanes without a point column and lanes whose element
// lies beyond the batch read the address of the chunk's last valid column (in bounds, the same lines); what they compute
// is not stored.  Nothing is read outside df, which needs only scalar alignment.  The first slices are requested in
// front of the last field's unit, in flight under its sweeps.
//
// Output.  Lane (e, j, i) stores its point of every requested plane: consecutive lanes write consecutive scalars of a
// plane, the planes of a column follow one another.  Plain stores (DESIGN s4.4).  Lanes without a point column and
// elements beyond the batch store nothing.  MASK names the outputs an instantiation can write (kVecGrad, kVecDiv,
// kVecCurl); every store of an instantiation is behind a wave-uniform null check of its pointer, so a request that is
// routed to a superset writes the requested planes only.
#pragma once

#include "geom_wave.h"
#include "physderiv_wave.h"

namespace sf
{

constexpr int kVecGrad = 1, kVecDiv = 2, kVecCurl = 4, kVecAll = 7;

// ------------------------------------------------------------------------------------------------
// 3D hex
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int MASK, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void hex_vecgrad_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, const T *__restrict__ x0,
    const T *__restrict__ x1, const T *__restrict__ x2, T *__restrict__ grad, T *__restrict__ div, T *__restrict__ curl0,
    T *__restrict__ curl1, T *__restrict__ curl2, uint64_t nelmt)
{
    using G            = GeomGeom<NQ, EC, 3, T>;
    constexpr int RING = G::RING, NCOMP = 9;
#define OPEN_DIM 3
#define OPEN_KEPT_BASE G::KEPT_BASE // d u_0 / d xi_1, d u_0 / d xi_0, d u_1 / d xi_1, d u_1 / d xi_0
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[3][NPASS][NQ]; // d u_a / d xi_2 over k
        // the ring of df: every lane's offsets are in bounds
        const T *dc = df + c * (uint64_t)(EC * NCOMP * NQT);
#define RING_OFF doff[NPASS]
#define RING_SET doff[s] = e * (NCOMP * NQT) + colp[s];
#include "frag/ring_offsets.inc"
        T dv[RING][NPASS][NCOMP];
#define FRONT_PRIME                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < RING; ++r) load_df_slice<NPASS, NCOMP, NQ2, NQT>(dv[r], dc, doff, r);
#include "frag/fields_front_3d.inc"
        // ---- the walk over k: grad of the point, its stores ---------------------------------------------
        {
#include "frag/walk_stores.inc"
#pragma unroll
            for (int k = 0; k < NQ; ++k)
            {
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T(&dd)[NCOMP] = dv[k % RING][s];
#include "frag/point_jacobian_3d.inc"
                    T g[3][3];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                            g[a][j] = fma_t(dd[3 * j + 2], J[a][2], fma_t(dd[3 * j + 1], J[a][1], dd[3 * j] * J[a][0]));
                    if (put[s])
                    {
                        const int oo = ooff[s] + k * NQ2;
                        if constexpr ((MASK & kVecGrad) != 0)
                            if (grad)
#define PLANES_DST grad
#define PLANES_N 9
#define PLANES_VAL(cc) g[(cc) / 3][(cc) % 3]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kVecDiv) != 0)
                            if (div)
                                div[e0 * NQT + oo] = (g[0][0] + g[1][1]) + g[2][2];
                        if constexpr ((MASK & kVecCurl) != 0)
                            if (curl0)
                            {
                                curl0[e0 * NQT + oo] = g[2][1] - g[1][2];
                                curl1[e0 * NQT + oo] = g[0][2] - g[2][0];
                                curl2[e0 * NQT + oo] = g[1][0] - g[0][1];
                            }
                    }
                }
                if (k + RING < NQ)
                    load_df_slice<NPASS, NCOMP, NQ2, NQT>(dv[k % RING], dc, doff, k + RING);
                __builtin_amdgcn_sched_barrier(0); // the ring stays a ring: no load moves up across a slice
            }
            wave_lds_fence(); // the images of the last field are rewritten by the next chunk's staging
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2D quad
// ------------------------------------------------------------------------------------------------
template <int NQ, int EC, int WPB, int BMODE, int MINW, int KMAP, int MEMF, int MASK, typename T = double>
__global__ __launch_bounds__(kWave *WPB, MINW) void quad_vecgrad_wave_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ d0, const T *__restrict__ d1,
    const T *__restrict__ df, const T *__restrict__ x0, const T *__restrict__ x1, T *__restrict__ grad,
    T *__restrict__ div, T *__restrict__ curl0, uint64_t nelmt)
{
    using G            = GeomGeom<NQ, EC, 2, T>;
    constexpr int RING = G::RING, NCOMP = 4;
#define OPEN_DIM 2
#define OPEN_KEPT_BASE G::KEPT_BASE // d u_0 / d xi_0
#define OPEN_LANE_SETUP
#include "frag/wave_open.inc"

    uint64_t c = it.first;
    for (uint64_t n = 0; n < it.count; ++n, c += it.step)
    {
#include "frag/chunk_head.inc"
        T dk[2][NPASS][NQ]; // d u_a / d xi_1 over j
        // the ring of df, as in the 3D kernel
        const T *dc = df + c * (uint64_t)(EC * NCOMP * NQT);
#define RING_OFF doff[NPASS]
#define RING_SET doff[s] = e * (NCOMP * NQT) + colp[s];
#include "frag/ring_offsets.inc"
        T dv[RING][NPASS][NCOMP];
#define FRONT_PRIME                                                                                                    \
    _Pragma("unroll") for (int r = 0; r < RING; ++r) load_df_slice<NPASS, NCOMP, NQ, NQT>(dv[r], dc, doff, r);
#include "frag/fields_front_2d.inc"
        // ---- the walk over j ---------------------------------------------------------------------------
        {
#include "frag/walk_stores.inc"
#pragma unroll
            for (int j = 0; j < NQ; ++j)
            {
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
                {
                    const T(&dd)[NCOMP] = dv[j % RING][s];
#include "frag/point_jacobian_2d.inc"
                    T g[2][2];
#pragma unroll
                    for (int a = 0; a < 2; ++a)
#pragma unroll
                        for (int x = 0; x < 2; ++x)
                            g[a][x] = fma_t(dd[2 * x + 1], J[a][1], dd[2 * x] * J[a][0]);
                    if (put[s])
                    {
                        const int oo = ooff[s] + j * NQ;
                        if constexpr ((MASK & kVecGrad) != 0)
                            if (grad)
#define PLANES_DST grad
#define PLANES_N 4
#define PLANES_VAL(cc) g[(cc) / 2][(cc) % 2]
#include "frag/planes_store.inc"
                        if constexpr ((MASK & kVecDiv) != 0)
                            if (div)
                                div[e0 * NQT + oo] = g[0][0] + g[1][1];
                        if constexpr ((MASK & kVecCurl) != 0)
                            if (curl0)
                                curl0[e0 * NQT + oo] = g[1][0] - g[0][1];
                    }
                }
                if (j + RING < NQ)
                    load_df_slice<NPASS, NCOMP, NQ, NQT>(dv[j % RING], dc, doff, j + RING);
                __builtin_amdgcn_sched_barrier(0);
            }
            wave_lds_fence(); // the image of the last field is rewritten by the next chunk's staging
        }
    }
}

} // namespace sf
