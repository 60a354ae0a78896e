// physderiv_generic.hip -- BwdTrans fused with the physical-space gradient, out_a = sum_b df_ab D_b B x, for any
// extents: the fallback of the wave kernels of physderiv_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; out_a = sum_b df_ab du_b (b ascending; no df: out_a = du_a).
// Two LDS regions of one point image each, P0 and P1 -- the derivatives go from the image of u to HBM through registers:
//   3D: in (P1) -> w1 (P0) -> w2 (P1) -> u (P0) -> du_0, du_1, du_2 (registers) -> out_0, out_1, out_2 (HBM)
//   2D: in (P1) -> w1 (P1, behind in) -> u (P0) -> du_0, du_1 (registers) -> out_0, out_1 (HBM)
// The forward sweeps are those of helm_generic_body (helmholtz_generic.h), restated here because that body runs on to
// the transposed half; the bounds and the LDS classes are shared with it.  Every buffer is read and written with scalar
// accesses: scalar alignment is enough.  No workspace and static LDS only: every launch is a single kernel node that
// needs no function attribute, capture-safe from the first call.  `df` is not dereferenced when has_df is false.
// Latency-bound (a barrier per sweep, one element per workgroup), not a roofline target.  Extents up to 12 per direction
// in 3D and 32 in 2D; beyond, SF_ENOTBUILT.
#include "helmholtz_generic.h"

namespace sf
{

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void physderiv_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ df, bool has_df, const T *__restrict__ in,
    T *__restrict__ out0, T *__restrict__ out1, T *__restrict__ out2, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
    const int nm0 = nq0 - 1, nm1 = nq1 - 1, nm2 = DIM == 3 ? nq2 - 1 : 1;
    const int nz  = DIM == 3 ? nq2 : 1;
    const int n01 = nq0 * nq1;
    const int nqt = n01 * nz;        // points per element
    const int nmt = nm0 * nm1 * nm2; // modes per element
    T *P0 = lds, *P1 = lds + nqt;
    const int tid = threadIdx.x;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        const T *dfe = has_df ? df + e * (uint64_t)(DIM * DIM * nqt) : nullptr;
        T *o0 = out0 + e * (uint64_t)nqt, *o1 = out1 + e * (uint64_t)nqt;
        for (int x = tid; x < nmt; x += NT)
            P1[x] = src[x];
        __syncthreads();
        if constexpr (DIM == 2)
        {
            // forward 0: w1[q][i] = sum_p in[q][p] * B0[p][i], behind the modes in P1 (nmt + nm1 nq0 <= nqt + nq0 nq1)
            T *W1 = P1 + nmt;
            for (int x = tid; x < nm1 * nq0; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                W1[x] = dot_strided(P1 + q * nm0, 1, b0 + i, nq0, nm0);
            }
            __syncthreads();
            // forward 1: u[j][i] = sum_q w1[q][i] * B1[q][j]
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                P0[x] = dot_strided(W1 + i, nq0, b1 + j, nq1, nm1);
            }
            __syncthreads();
            // du_0[j][i] = sum_m D0[i][m] u[j][m];  du_1[j][i] = sum_m D1[j][m] u[m][i];  out_a = sum_b df_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                const T x0 = dot_strided(P0 + j * nq0, 1, d0 + i * nq0, 1, nq0);
                const T x1 = dot_strided(P0 + i, nq0, d1 + j * nq1, 1, nq1);
                if (has_df)
                {
                    o0[x] = sfma(dfe[1 * nqt + x], x1, dfe[0 * nqt + x] * x0);
                    o1[x] = sfma(dfe[3 * nqt + x], x1, dfe[2 * nqt + x] * x0);
                }
                else
                {
                    o0[x] = x0;
                    o1[x] = x1;
                }
            }
        }
        else
        {
            T *o2 = out2 + e * (uint64_t)nqt;
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
            // du_0 = D0 u along i, du_1 = D1 u along j, du_2 = D2 u along k;  out_a = sum_b df_ab du_b
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                const T x0 = dot_strided(P0 + kj * nq0, 1, d0 + i * nq0, 1, nq0);
                const T x1 = dot_strided(P0 + k * n01 + i, nq0, d1 + j * nq1, 1, nq1);
                const T x2 = dot_strided(P0 + j * nq0 + i, n01, d2 + k * nq2, 1, nq2);
                if (has_df)
                {
                    o0[x] = sfma(dfe[2 * nqt + x], x2, sfma(dfe[1 * nqt + x], x1, dfe[0 * nqt + x] * x0));
                    o1[x] = sfma(dfe[5 * nqt + x], x2, sfma(dfe[4 * nqt + x], x1, dfe[3 * nqt + x] * x0));
                    o2[x] = sfma(dfe[8 * nqt + x], x2, sfma(dfe[7 * nqt + x], x1, dfe[6 * nqt + x] * x0));
                }
                else
                {
                    o0[x] = x0;
                    o1[x] = x1;
                    o2[x] = x2;
                }
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

template <int DIM, typename T>
int launch_physderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x, hipStream_t s)
{
    if (!physderiv_generic_built(DIM, nq[0], nq[1], nq[2]))
        return SF_ENOTBUILT;
    if (a.nelmt == 0)
        return SF_OK;
    // The classes of the Helmholtz fallback by extents (64 threads up to 8^3 / 26^2).  This kernel needs 2 nqt scalars in
    // 3D and fewer than 3 nqt in 2D (nqt + nmt + nm1 nq0), where helm_need() is 4 nqt and 3 nqt: the small class keeps
    // its size, the large one holds 2 * 12^3 = 3456 >= 3 * 32^2.
    return launch_lds_class(helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                            physderiv_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                            physderiv_generic_kernel<T, DIM, kHelmLargeCap / 2, 256>, a.nelmt, s, a.b0, a.b1, basis2(a),
                            x.d0, x.d1, x.d2, x.df, x.df != nullptr, a.in, x.out0, x.out1, x.out2, a.nelmt, (int)nq[0],
                            (int)nq[1], (int)nq[2]);
}
template int launch_physderiv_generic<3, double>(const unsigned (&)[3], const HexArgs &, const PhysDerivArgsT<double> &,
                                                 hipStream_t);
template int launch_physderiv_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &,
                                                const PhysDerivArgsT<float> &, hipStream_t);
template int launch_physderiv_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const PhysDerivArgsT<double> &,
                                                 hipStream_t);
template int launch_physderiv_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &,
                                                const PhysDerivArgsT<float> &, hipStream_t);

bool physderiv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return helm_extents_built(dim, nq0, nq1, nq2);
}

} // namespace sf
