// helmholtz_generic.h -- the any-extent kernel body of the fused Helmholtz operator, shared by helmholtz_generic.hip (a
// metric per point) and affine_generic.hip (constants per element).  What the kernels do, their order of operations and
// their LDS images are described at the top of those two units; the body is that of helmholtz_generic.hip with the
// flux-and-mass step taken out into flux_points(), which asks a policy MET:
//   MET::SCALED, MET::NCOMP   the fluxes and the mass term carry a factor q per point; metric components per point
//   element(e, nqt)           once per element
//   coef(x, nqt, gg)          the NCOMP coefficients of point x, in the order of the planes of g
//   scale(x, nq0, nq1)        q of point x (read only if SCALED)
//   mass(x, q, u)             the mass term of the point value u
#pragma once

#include "any_extent.h"

namespace sf
{

constexpr unsigned kHelmMax3D = 12, kHelmMax2D = 32;
constexpr int kHelmSmallCap = 2048, kHelmLargeCap = 4 * 12 * 12 * 12; // scalars; 2D 32^2 needs 3 * 1024

// fluxes in place (P1 .. P3), the mass term over u (P0): every thread touches its own points only
template <int DIM, int NT, class MET, typename T>
__device__ __forceinline__ void flux_points(const MET &met, int tid, int nq0, int nq1, int nqt, T *P0, T *P1, T *P2, T *P3)
{
    for (int x = tid; x < nqt; x += NT)
    {
        T gg[MET::NCOMP];
        met.coef(x, nqt, gg);
        const T q = met.scale(x, nq0, nq1);
        T f0, f1, f2 = T(0);
        if constexpr (DIM == 3)
        {
            const T x0 = P1[x], x1 = P2[x], x2 = P3[x];
            f0 = sfma(gg[2], x2, sfma(gg[1], x1, gg[0] * x0));
            f1 = sfma(gg[4], x2, sfma(gg[3], x1, gg[1] * x0));
            f2 = sfma(gg[5], x2, sfma(gg[4], x1, gg[2] * x0));
        }
        else
        {
            const T x0 = P1[x], x1 = P2[x];
            f0 = sfma(gg[1], x1, gg[0] * x0);
            f1 = sfma(gg[2], x1, gg[1] * x0);
        }
        if constexpr (MET::SCALED)
            f0 = q * f0, f1 = q * f1, f2 = q * f2;
        P1[x] = f0;
        P2[x] = f1;
        if constexpr (DIM == 3)
            P3[x] = f2;
        P0[x] = met.mass(x, q, P0[x]);
    }
}

// the whole operator on the elements of this workgroup; lds: the images, 4 (2D: 3) nq0 nq1 nq2 scalars
template <typename T, int DIM, int NT, class MET>
__device__ __forceinline__ void helm_generic_body(T *lds, const T *b0, const T *b1, const T *b2, const T *d0, const T *d1,
                                                  const T *d2, MET &met, const T *in, T *out, uint64_t nelmt, int nq0,
                                                  int nq1, int nq2)
{
    const int nm0 = nq0 - 1, nm1 = nq1 - 1, nm2 = DIM == 3 ? nq2 - 1 : 1;
    const int nz  = DIM == 3 ? nq2 : 1;
    const int n01 = nq0 * nq1;
    const int nqt = n01 * nz;        // points per element
    const int nmt = nm0 * nm1 * nm2; // modes per element
    T *P0 = lds, *P1 = lds + nqt, *P2 = lds + 2 * nqt, *P3 = lds + (DIM == 3 ? 3 : 2) * nqt;
    const int tid = threadIdx.x;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        T *dst       = out + e * (uint64_t)nmt;
        met.element(e, nqt);
        for (int x = tid; x < nmt; x += NT)
            P1[x] = src[x];
        __syncthreads();
        if constexpr (DIM == 2)
        {
            // forward 0: w1[q][i] = sum_p in[q][p] * B0[p][i]
            for (int x = tid; x < nm1 * nq0; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                P2[x] = dot_strided(P1 + q * nm0, 1, b0 + i, nq0, nm0);
            }
            __syncthreads();
            // forward 1: u[j][i] = sum_q w1[q][i] * B1[q][j]
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                P0[x] = dot_strided(P2 + i, nq0, b1 + j, nq1, nm1);
            }
            __syncthreads();
            // du_0[j][i] = sum_m D0[i][m] u[j][m];  du_1[j][i] = sum_m D1[j][m] u[m][i]
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                P1[x] = dot_strided(P0 + j * nq0, 1, d0 + i * nq0, 1, nq0);
                P2[x] = dot_strided(P0 + i, nq0, d1 + j * nq1, 1, nq1);
            }
            __syncthreads();
            // fluxes in place, the mass term over u (every thread touches its own points only)
            flux_points<DIM, NT>(met, tid, nq0, nq1, nqt, P0, P1, P2, P3);
            __syncthreads();
            // v = ((lambda w) u + D_0^T f_0) + D_1^T f_1, over the mass term
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                const T t0 = dot_strided(P1 + j * nq0, 1, d0 + i, nq0, nq0);
                const T t1 = dot_strided(P2 + i, nq0, d1 + j, nq1, nq1);
                P0[x]      = (P0[x] + t0) + t1;
            }
            __syncthreads();
            // transposed 1: t1[q'][i] = sum_j v[j][i] * B1[q'][j]
            for (int x = tid; x < nm1 * nq0; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                P1[x] = dot_strided(P0 + i, nq0, b1 + q * nq1, 1, nq1);
            }
            __syncthreads();
            // transposed 0: out[q'][p'] = sum_i t1[q'][i] * B0[p'][i]
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, q = x / nm0;
                dst[x] = dot_strided(P1 + q * nq0, 1, b0 + p * nq0, 1, nq0);
            }
        }
        else
        {
            // forward 0: w1[r][q][i] = sum_p in[r][q][p] * B0[p][i]
            for (int x = tid; x < nq0 * nm1 * nm2; x += NT)
            {
                const int i = x % nq0, rq = x / nq0;
                P0[x] = dot_strided(P1 + rq * nm0, 1, b0 + i, nq0, nm0);
            }
            __syncthreads();
            // forward 1: w2[r][j][i] = sum_q w1[r][q][i] * B1[q][j]
            for (int x = tid; x < n01 * nm2; x += NT)
            {
                const int i = x % nq0, rj = x / nq0, j = rj % nq1, r = rj / nq1;
                P1[x] = dot_strided(P0 + r * nm1 * nq0 + i, nq0, b1 + j, nq1, nm1);
            }
            __syncthreads();
            // forward 2: u[k][j][i] = sum_r w2[r][j][i] * B2[r][k]
            for (int x = tid; x < nqt; x += NT)
            {
                const int ji = x % n01, k = x / n01;
                P0[x] = dot_strided(P1 + ji, n01, b2 + k, nq2, nm2);
            }
            __syncthreads();
            // du_0 = D0 u along i, du_1 = D1 u along j, du_2 = D2 u along k
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                P1[x] = dot_strided(P0 + kj * nq0, 1, d0 + i * nq0, 1, nq0);
                P2[x] = dot_strided(P0 + k * n01 + i, nq0, d1 + j * nq1, 1, nq1);
                P3[x] = dot_strided(P0 + j * nq0 + i, n01, d2 + k * nq2, 1, nq2);
            }
            __syncthreads();
            // fluxes in place, the mass term over u (every thread touches its own points only)
            flux_points<DIM, NT>(met, tid, nq0, nq1, nqt, P0, P1, P2, P3);
            __syncthreads();
            // v = (((lambda w) u + D_0^T f_0) + D_1^T f_1) + D_2^T f_2, over the mass term
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                const T t0 = dot_strided(P1 + kj * nq0, 1, d0 + i, nq0, nq0);
                const T t1 = dot_strided(P2 + k * n01 + i, nq0, d1 + j, nq1, nq1);
                const T t2 = dot_strided(P3 + j * nq0 + i, n01, d2 + k, nq2, nq2);
                P0[x]      = ((P0[x] + t0) + t1) + t2;
            }
            __syncthreads();
            // transposed 2: t1[r'][j][i] = sum_k v[k][j][i] * B2[r'][k]
            for (int x = tid; x < n01 * nm2; x += NT)
            {
                const int ji = x % n01, r = x / n01;
                P1[x] = dot_strided(P0 + ji, n01, b2 + r * nq2, 1, nq2);
            }
            __syncthreads();
            // transposed 1: t2[r'][q'][i] = sum_j t1[r'][j][i] * B1[q'][j]
            for (int x = tid; x < nq0 * nm1 * nm2; x += NT)
            {
                const int i = x % nq0, rq = x / nq0, q = rq % nm1, r = rq / nm1;
                P2[x] = dot_strided(P1 + r * n01 + i, nq0, b1 + q * nq1, 1, nq1);
            }
            __syncthreads();
            // transposed 0: out[r'][q'][p'] = sum_i t2[r'][q'][i] * B0[p'][i]
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, rq = x / nm0;
                dst[x] = dot_strided(P2 + rq * nq0, 1, b0 + p * nq0, 1, nq0);
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

// scalars of LDS the extents need: one point image per region
inline unsigned helm_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return dim == 3 ? 4 * nq0 * nq1 * nq2 : 3 * nq0 * nq1;
}

// within the extent bounds AND the images fit the large LDS class (true for every extent within the bounds: 3D 12^3
// needs 6912, 2D 32^2 3072; derived all the same, not assumed)
inline bool helm_extents_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kHelmMax3D : kHelmMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    return helm_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kHelmLargeCap;
}

} // namespace sf
