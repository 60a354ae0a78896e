// helmholtz_generic.hip -- the fused Helmholtz operator B^T [lambda diag(w) + sum_ab D_a^T diag(G_ab) D_b] B for any
// extents: the fallback of the wave kernels of helmholtz_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS, one thread per output value
// of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of operations of the
// wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; f_a = sum_b G_ab du_b (b ascending);
// v = ((lambda w) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]; transposed k -> r', j -> q', i -> p'.
// Four (2D: three) LDS regions of one point image each, P0 .. P3:
//   3D: in (P1) -> w1 (P0) -> w2 (P1) -> u (P0) -> du_0, du_1, du_2 (P1, P2, P3) -> f_0, f_1, f_2 in place and
//       (lambda w) u over u (P0) -> v over it (P0) -> t1 (P1) -> t2 (P2) -> out (HBM)
//   2D: in (P1) -> w1 (P2) -> u (P0) -> du_0, du_1 (P1, P2) -> f_0, f_1 in place, (lambda w) u (P0) -> v (P0) -> t1 (P1)
//       -> out (HBM)
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `w` is not
// dereferenced when has_w is false.  Latency-bound (a barrier per sweep, one element per workgroup), not a roofline
// target.  Extents up to 12 per direction in 3D (four images of 12^3 doubles: 55 296 bytes of the 64 KB of static LDS)
// and 32 in 2D; beyond, SF_ENOTBUILT.
#include "any_extent.h"

namespace sf
{

constexpr unsigned kHelmMax3D = 12, kHelmMax2D = 32;
constexpr int kHelmSmallCap = 2048, kHelmLargeCap = 4 * 12 * 12 * 12; // scalars; 2D 32^2 needs 3 * 1024

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void helmholtz_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ g, const T *__restrict__ w, T lam,
    bool has_w, const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
    const int nm0 = nq0 - 1, nm1 = nq1 - 1, nm2 = DIM == 3 ? nq2 - 1 : 1;
    const int nz  = DIM == 3 ? nq2 : 1;
    const int n01 = nq0 * nq1;
    const int nqt = n01 * nz;        // points per element
    const int nmt = nm0 * nm1 * nm2; // modes per element
    constexpr int NCOMP = DIM == 3 ? 6 : 3;
    T *P0 = lds, *P1 = lds + nqt, *P2 = lds + 2 * nqt, *P3 = lds + (DIM == 3 ? 3 : 2) * nqt;
    const int tid = threadIdx.x;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nmt;
        const T *ge  = g + e * (uint64_t)(NCOMP * nqt);
        const T *wt  = has_w ? w + e * (uint64_t)nqt : nullptr;
        T *dst       = out + e * (uint64_t)nmt;
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
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = P1[x], x1 = P2[x];
                const T g00 = ge[x], g01 = ge[nqt + x], g11 = ge[2 * nqt + x];
                P1[x] = sfma(g01, x1, g00 * x0);
                P2[x] = sfma(g11, x1, g01 * x0);
                P0[x] = has_w ? (lam * wt[x]) * P0[x] : T(0);
            }
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
            for (int x = tid; x < nqt; x += NT)
            {
                const T x0 = P1[x], x1 = P2[x], x2 = P3[x];
                const T g00 = ge[x], g01 = ge[nqt + x], g02 = ge[2 * nqt + x];
                const T g11 = ge[3 * nqt + x], g12 = ge[4 * nqt + x], g22 = ge[5 * nqt + x];
                P1[x] = sfma(g02, x2, sfma(g01, x1, g00 * x0));
                P2[x] = sfma(g12, x2, sfma(g11, x1, g01 * x0));
                P3[x] = sfma(g22, x2, sfma(g12, x1, g02 * x0));
                P0[x] = has_w ? (lam * wt[x]) * P0[x] : T(0);
            }
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
static unsigned helm_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return dim == 3 ? 4 * nq0 * nq1 * nq2 : 3 * nq0 * nq1;
}

template <int DIM, typename T>
int launch_helmholtz_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s)
{
    if (!helmholtz_generic_built(DIM, nq[0], nq[1], nq[2]))
        return SF_ENOTBUILT;
    if (a.nelmt == 0)
        return SF_OK;
    return launch_lds_class(helm_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kHelmSmallCap,
                            helmholtz_generic_kernel<T, DIM, kHelmSmallCap, 64>,
                            helmholtz_generic_kernel<T, DIM, kHelmLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0,
                            x.d1, x.d2, x.g, x.w, x.lam, x.w != nullptr, a.in, a.out, a.nelmt, (int)nq[0], (int)nq[1],
                            (int)nq[2]);
}
template int launch_helmholtz_generic<3, double>(const unsigned (&)[3], const HexArgs &, const HelmArgsT<double> &,
                                                 hipStream_t);
template int launch_helmholtz_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const HelmArgsT<float> &,
                                                hipStream_t);
template int launch_helmholtz_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const HelmArgsT<double> &,
                                                 hipStream_t);
template int launch_helmholtz_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const HelmArgsT<float> &,
                                                hipStream_t);

// within the extent bounds AND the images fit the large LDS class (true for every extent within the bounds: 3D 12^3
// needs 6912, 2D 32^2 3072; derived all the same, not assumed)
bool helmholtz_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kHelmMax3D : kHelmMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    return helm_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kHelmLargeCap;
}

} // namespace sf
