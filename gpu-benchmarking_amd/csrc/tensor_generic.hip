// tensor_generic.hip -- the tensor-product apply of sf_tensor_* for any extents: the fallback of the wave kernels of
// bwdtrans_aniso.h (hex_tensor_wave_kernel / quad_tensor_wave_kernel).
//
// One workgroup per element (a grid-stride loop over elements), every image in static LDS: the element's input
// (ni0*ni1[*ni2] scalars, staged with scalar loads, so buffers aligned only to the scalar are fine), the first
// intermediate behind it, and in 3D the second intermediate over the input.  One thread per output value of a sweep;
// direction 0, then 1, then 2, each sum in ascending summed index, the first term a multiplication and the rest FMAs: the
// order of the wave kernels, so the two routes give the same bits.  The matrices are read straight from global memory
// (cache-resident), row-major ni x no (trans 0) or no x ni (trans 1).  Scalar accesses to every buffer.  No workspace:
// every launch is a single kernel node, capture-safe from the first call.  Extents from 1 up to 16 per direction in 3D
// and 32 in 2D, input and output independently; beyond, SF_ENOTBUILT.  Latency-bound, not a roofline target.
#include "any_extent.h"

namespace sf
{

// LDS classes in scalars: max(input, second intermediate) + first intermediate.  3D 16 -> 16: 4096 + 4096; 2D 32 -> 32:
// 1024 + 1024.
constexpr int kTensorSmallCap = 2048, kTensorLargeCap = 8192;
constexpr unsigned kTensorMax3D = 16, kTensorMax2D = 32;

struct TensorExtents
{
    int ni0, ni1, ni2, no0, no1, no2; // 2D: ni2 = no2 = 1
};

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void tensor_generic_kernel(const T *__restrict__ m0, const T *__restrict__ m1,
                                                            const T *__restrict__ m2, const T *__restrict__ in,
                                                            T *__restrict__ out, uint64_t nelmt, TensorExtents x, int trans)
{
    __shared__ T lds[CAP];
    const int ni0 = x.ni0, ni1 = x.ni1, ni2 = DIM == 3 ? x.ni2 : 1, no0 = x.no0, no1 = x.no1, no2 = DIM == 3 ? x.no2 : 1;
    const int nin  = ni0 * ni1 * ni2;                 // input values per element
    const int nout = no0 * no1 * no2;                 // output values per element
    const int n1   = no0 * ni1 * ni2;                 // first intermediate  w1[r][q][i]
    const int n2   = DIM == 3 ? no0 * no1 * ni2 : 0;  // second intermediate w2[r][j][i], over the input
    T *img = lds;
    T *w1  = lds + (nin > n2 ? nin : n2);
    // M_d(a, b) = m_d[a*ms_d + b*mo_d]: the summed index a strides by ms, the output index b by mo
    const int ms0 = trans ? 1 : no0, mo0 = trans ? ni0 : 1;
    const int ms1 = trans ? 1 : no1, mo1 = trans ? ni1 : 1;
    const int ms2 = trans ? 1 : no2, mo2 = trans ? ni2 : 1;
    const int tid = threadIdx.x;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        const T *src = in + e * (uint64_t)nin;
        for (int t = tid; t < nin; t += NT)
            img[t] = src[t];
        __syncthreads();
        // direction 0: w1[r][q][i] = sum_p in[r][q][p] * M0(p, i)
        for (int t = tid; t < n1; t += NT)
        {
            const int i = t % no0, rq = t / no0;
            w1[t] = dot_strided(img + rq * ni0, 1, m0 + i * mo0, ms0, ni0);
        }
        __syncthreads();
        T *dst = out + e * (uint64_t)nout;
        if constexpr (DIM == 2)
        {
            // direction 1: out[j][i] = sum_q w1[q][i] * M1(q, j)
            for (int t = tid; t < nout; t += NT)
            {
                const int i = t % no0, j = t / no0;
                dst[t] = dot_strided(w1 + i, no0, m1 + j * mo1, ms1, ni1);
            }
        }
        else
        {
            // direction 1: w2[r][j][i] = sum_q w1[r][q][i] * M1(q, j)  (over the input image)
            for (int t = tid; t < n2; t += NT)
            {
                const int i = t % no0, rj = t / no0, j = rj % no1, r = rj / no1;
                img[t] = dot_strided(w1 + r * ni1 * no0 + i, no0, m1 + j * mo1, ms1, ni1);
            }
            __syncthreads();
            // direction 2: out[k][j][i] = sum_r w2[r][j][i] * M2(r, k)
            const int nji = no0 * no1;
            for (int t = tid; t < nout; t += NT)
            {
                const int ji = t % nji, k = t / nji;
                dst[t] = dot_strided(img + ji, nji, m2 + k * mo2, ms2, ni2);
            }
        }
        __syncthreads(); // the next element overwrites the images
    }
}

// scalars of LDS a shape needs
static unsigned tensor_generic_need(int dim, const unsigned (&ni)[3], const unsigned (&no)[3])
{
    const unsigned i2 = dim == 3 ? ni[2] : 1;
    const unsigned nin = ni[0] * ni[1] * i2, n1 = no[0] * ni[1] * i2, n2 = dim == 3 ? no[0] * no[1] * i2 : 0;
    return (nin > n2 ? nin : n2) + n1;
}

template <int DIM, typename T>
int launch_tensor_generic(const unsigned (&ni)[3], const unsigned (&no)[3], int trans, const ArgsT<DIM, T> &a, hipStream_t s)
{
    const TensorExtents x = {(int)ni[0], (int)ni[1], DIM == 3 ? (int)ni[2] : 1,
                             (int)no[0], (int)no[1], DIM == 3 ? (int)no[2] : 1};
    return launch_any_extent(tensor_generic_built(DIM, ni, no),
                             tensor_generic_need(DIM, ni, no) <= (unsigned)kTensorSmallCap,
                             tensor_generic_kernel<T, DIM, kTensorSmallCap, 64>,
                             tensor_generic_kernel<T, DIM, kTensorLargeCap, 256>, a.nelmt, s, a.b0, a.b1, basis2(a), a.in,
                             a.out, a.nelmt, x, trans);
}
template int launch_tensor_generic<3, double>(const unsigned (&)[3], const unsigned (&)[3], int, const HexArgs &,
                                              hipStream_t);
template int launch_tensor_generic<3, float>(const unsigned (&)[3], const unsigned (&)[3], int, const HexArgsT<float> &,
                                             hipStream_t);
template int launch_tensor_generic<2, double>(const unsigned (&)[3], const unsigned (&)[3], int, const QuadArgs &,
                                              hipStream_t);
template int launch_tensor_generic<2, float>(const unsigned (&)[3], const unsigned (&)[3], int, const QuadArgsT<float> &,
                                             hipStream_t);

bool tensor_generic_built(int dim, const unsigned (&ni)[3], const unsigned (&no)[3])
{
    const unsigned mx = dim == 3 ? kTensorMax3D : kTensorMax2D;
    for (int d = 0; d < dim; ++d)
        if (ni[d] < 1 || no[d] < 1 || ni[d] > mx || no[d] > mx)
            return false;
    return tensor_generic_need(dim, ni, no) <= (unsigned)kTensorLargeCap;
}

} // namespace sf
