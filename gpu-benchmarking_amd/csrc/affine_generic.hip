// affine_generic.hip -- the fused Helmholtz operator on affine elements, B^T [lambda je_e diag(q) + sum_ab ge_ab D_a^T
// diag(q) D_b] B with q the tensor product of the one-dimensional quadrature weights, for any extents: the fallback of
// the wave kernels of affine_wave.h.
//
// The kernel of helmholtz_generic.hip with the metric planes replaced: one workgroup per element (a grid-stride loop
// over elements), the same images in static LDS (four regions of one point image in 3D, three in 2D), one thread per
// output value of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order of
// operations of the wave kernels: forward p -> i, q -> j, r -> k; du_a = D_a u; q = qw2[k] (qw1[j] qw0[i]) (2D: qw1[j]
// qw0[i]); f_a = q (sum_b ge_ab du_b), b ascending; v = (((lambda je_e) q) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2];
// transposed k -> r', j -> q', i -> p'.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `je` is not
// dereferenced when has_j is false.  Latency-bound, not a roofline target.  Extents up to 12 per direction in 3D and 32
// in 2D; beyond, SF_ENOTBUILT.
#include "any_extent.h"

namespace sf
{

constexpr unsigned kAffMax3D = 12, kAffMax2D = 32;
constexpr int kAffSmallCap = 2048, kAffLargeCap = 4 * 12 * 12 * 12; // scalars; 2D 32^2 needs 3 * 1024

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void affine_generic_kernel(
    const T *__restrict__ b0, const T *__restrict__ b1, const T *__restrict__ b2, const T *__restrict__ d0,
    const T *__restrict__ d1, const T *__restrict__ d2, const T *__restrict__ qw0, const T *__restrict__ qw1,
    const T *__restrict__ qw2, const T *__restrict__ ge, const T *__restrict__ je, T lam, bool has_j,
    const T *__restrict__ in, T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
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
        const T *gc  = ge + e * (uint64_t)NCOMP;
        const T lj   = has_j ? lam * je[e] : T(0);
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
            const T g00 = gc[0], g01 = gc[1], g11 = gc[2];
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                const T q  = qw1[j] * qw0[i];
                const T x0 = P1[x], x1 = P2[x];
                P1[x] = q * sfma(g01, x1, g00 * x0);
                P2[x] = q * sfma(g11, x1, g01 * x0);
                P0[x] = has_j ? (lj * q) * P0[x] : T(0);
            }
            __syncthreads();
            // v = (((lambda je) q) u + D_0^T f_0) + D_1^T f_1, over the mass term
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
            const T g00 = gc[0], g01 = gc[1], g02 = gc[2], g11 = gc[3], g12 = gc[4], g22 = gc[5];
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                const T q  = qw2[k] * (qw1[j] * qw0[i]);
                const T x0 = P1[x], x1 = P2[x], x2 = P3[x];
                P1[x] = q * sfma(g02, x2, sfma(g01, x1, g00 * x0));
                P2[x] = q * sfma(g12, x2, sfma(g11, x1, g01 * x0));
                P3[x] = q * sfma(g22, x2, sfma(g12, x1, g02 * x0));
                P0[x] = has_j ? (lj * q) * P0[x] : T(0);
            }
            __syncthreads();
            // v = ((((lambda je) q) u + D_0^T f_0) + D_1^T f_1) + D_2^T f_2, over the mass term
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
static unsigned affine_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return dim == 3 ? 4 * nq0 * nq1 * nq2 : 3 * nq0 * nq1;
}

template <int DIM, typename T>
int launch_affine_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s)
{
    if (!affine_generic_built(DIM, nq[0], nq[1], nq[2]))
        return SF_ENOTBUILT;
    if (a.nelmt == 0)
        return SF_OK;
    return launch_lds_class(affine_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kAffSmallCap,
                            affine_generic_kernel<T, DIM, kAffSmallCap, 64>,
                            affine_generic_kernel<T, DIM, kAffLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), x.d0, x.d1,
                            x.d2, x.qw0, x.qw1, x.qw2, x.ge, x.je, x.lam, x.je != nullptr, a.in, a.out, a.nelmt,
                            (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_affine_generic<3, double>(const unsigned (&)[3], const HexArgs &, const AffineArgsT<double> &,
                                              hipStream_t);
template int launch_affine_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const AffineArgsT<float> &,
                                             hipStream_t);
template int launch_affine_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const AffineArgsT<double> &,
                                              hipStream_t);
template int launch_affine_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const AffineArgsT<float> &,
                                             hipStream_t);

// within the extent bounds AND the images fit the large LDS class
bool affine_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kAffMax3D : kAffMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    return affine_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kAffLargeCap;
}

} // namespace sf
