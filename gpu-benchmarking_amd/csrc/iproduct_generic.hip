// iproduct_generic.hip -- IProductWRTBase for any extents: the fallback of the wave kernels of iproduct_wave.h.
//
// One workgroup per element (a grid-stride loop over elements), every image in LDS: the element's input (nq0*nq1[*nq2]
// points, staged with scalar-aligned loads, so 8-byte-aligned buffers are fine), the first intermediate next to it, and
// in 3D the second intermediate over the input.  One thread per output value of a sweep; each sum runs in ascending
// index, sweeps i -> p, j -> q, k -> r, the order of the wave kernels.  The bases are read straight from global memory
// (nm*nq values each, cache-resident).  No workspace: every launch is a single kernel node, capture-safe from the first
// call.  Extents up to 16 per direction in 3D and 32 in 2D; beyond, SF_ENOTBUILT.  The sums are written out where
// the fragments frag/ae_*.inc of the other any-extent kernels call dot_strided(): the compiler schedules the two forms
// differently here, and the sweeps run in the other order, so the kernel shares only its launch (any_extent.h).
#include "any_extent.h"

namespace sf
{

// LDS classes in scalars: input image + first intermediate.  3D 16^3: 4096 + 15*16*16 = 7936; 2D 32^2: 1024 + 31*32.
constexpr int kIprodSmallCap = 2048, kIprodLargeCap = 7936;
constexpr unsigned kIprodMax3D = 16, kIprodMax2D = 32;

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void iprod_generic_kernel(const T *__restrict__ b0, const T *__restrict__ b1,
                                                           const T *__restrict__ b2, const T *__restrict__ in,
                                                           T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
    const int nm0 = nq0 - 1, nm1 = nq1 - 1;
    const int nz  = DIM == 3 ? nq2 : 1;                 // points along direction 2
    const int nqt = nq0 * nq1 * nz;                     // input values per element
    const int nmt = nm0 * nm1 * (DIM == 3 ? nq2 - 1 : 1); // output values per element
    const int n1  = nm0 * nq1 * nz;                     // first intermediate
    T *img = lds;                                       // input, then (3D) the second intermediate
    T *w1  = lds + nqt;
    const int tid = threadIdx.x;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nqt;
        for (int x = tid; x < nqt; x += NT)
            img[x] = src[x];
        __syncthreads();
        // direction 0: w1[k][j][p] = sum_i in[k][j][i] * B0[p][i]
        for (int x = tid; x < n1; x += NT)
        {
            const int p = x % nm0, kj = x / nm0;
            const T *u = img + kj * nq0, *b = b0 + p * nq0;
            T a = u[0] * b[0];
            for (int i = 1; i < nq0; ++i)
                a = sfma(u[i], b[i], a);
            w1[x] = a;
        }
        __syncthreads();
        T *dst = out + e * (uint64_t)nmt;
        if constexpr (DIM == 2)
        {
            // direction 1: out[q][p] = sum_j w1[j][p] * B1[q][j]
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, q = x / nm0;
                const T *b = b1 + q * nq1;
                T a = w1[p] * b[0];
                for (int j = 1; j < nq1; ++j)
                    a = sfma(w1[j * nm0 + p], b[j], a);
                dst[x] = a;
            }
        }
        else
        {
            // direction 1: w2[k][q][p] = sum_j w1[k][j][p] * B1[q][j]  (over the input image)
            const int n2 = nm0 * nm1 * nq2;
            for (int x = tid; x < n2; x += NT)
            {
                const int p = x % nm0, kq = x / nm0, q = kq % nm1, k = kq / nm1;
                const T *u = w1 + k * nq1 * nm0 + p, *b = b1 + q * nq1;
                T a = u[0] * b[0];
                for (int j = 1; j < nq1; ++j)
                    a = sfma(u[j * nm0], b[j], a);
                img[x] = a;
            }
            __syncthreads();
            // direction 2: out[r][q][p] = sum_k w2[k][q][p] * B2[r][k]
            const int nqp = nm0 * nm1;
            for (int x = tid; x < nmt; x += NT)
            {
                const int qp = x % nqp, r = x / nqp;
                const T *u = img + qp, *b = b2 + r * nq2;
                T a = u[0] * b[0];
                for (int k = 1; k < nq2; ++k)
                    a = sfma(u[k * nqp], b[k], a);
                dst[x] = a;
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

template <int DIM, typename T> int launch_iprod_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, hipStream_t s)
{
    const unsigned nz   = DIM == 3 ? nq[2] : 1;
    const unsigned need = nq[0] * nq[1] * nz + (nq[0] - 1) * nq[1] * nz;
    return launch_any_extent(iprod_generic_built(DIM, nq[0], nq[1], nq[2]), need <= (unsigned)kIprodSmallCap,
                             iprod_generic_kernel<T, DIM, kIprodSmallCap, 64>,
                             iprod_generic_kernel<T, DIM, kIprodLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), a.in,
                             a.out, a.nelmt, (int)nq[0], (int)nq[1], (int)nq[2]);
}
template int launch_iprod_generic<3, double>(const unsigned (&)[3], const HexArgs &, hipStream_t);
template int launch_iprod_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, hipStream_t);
template int launch_iprod_generic<2, double>(const unsigned (&)[3], const QuadArgs &, hipStream_t);
template int launch_iprod_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, hipStream_t);

bool iprod_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kIprodMax3D : kIprodMax2D;
    return nq0 <= mx && nq1 <= mx && (dim != 3 || nq2 <= mx);
}

} // namespace sf
