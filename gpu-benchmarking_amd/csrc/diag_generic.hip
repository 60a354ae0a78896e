// diag_generic.hip -- the diagonal of the fused Helmholtz operator for any extents: the fallback of the wave kernels of
// diag_wave.h, and the kernel of sf_diag_tables_* that forms the tables both read.
//
//   diag_e[r][q][p] = sum_kji lambda w_e[k][j][i] T0^0[p][i] T1^0[q][j] T2^0[r][k]
//                   + sum_c f_c sum_kji g_e[c][k][j][i] T0^{s0}[p][i] T1^{s1}[q][j] T2^{s2}[r][k]
//
// T_d^t the three tables of direction d (tab_d[t][p][i]: B o B, E o B, E o E), s_d = [d == a] + [d == b] and f_c = 1
// (a == b) or 2 for the plane c = (a, b).  One workgroup per element (a grid-stride loop over elements), static LDS, one
// thread per output value of a sweep, each sum in ascending index, the first product a multiply and then FMAs.  The order
// of operations is that of the wave kernels (diag_wave.h states it in full): every term is swept k -> r with its
// direction-2 table straight from HBM into ONE image t1[r][j][i] at a time (off-diagonal planes doubled, which is exact;
// the lambda w image added to the G_22 image), each image is swept j -> q with its direction-1 table and added, in the
// order of the planes, to the image of its direction-0 table, B^{s0}[r][q][i]; the three are swept i -> p and added in the
// order s0 = 0, 1, 2.  2D: the same without k -- the first sweep j -> q writes the three images keyed by s0.
// LDS: t1 and the three B images, nm2 nq1 nq0 + 3 nm2 nm1 nq0 scalars (12^3: 5940; 2D: 3 nm1 nq0, 32^2: 2976).
// The transposed sweeps of frag/ae_transposed_*.inc do not fit (a table per image, sums of sweeps): they are written out.
// Every buffer is read and written with scalar accesses: scalar alignment is enough.  No workspace and static LDS only:
// every launch is a single kernel node that needs no function attribute, capture-safe from the first call.  `w` is not
// dereferenced when has_w is false.  Latency-bound, not a roofline target.  Extents up to 12 per direction in 3D and 32
// in 2D (the bounds of helmholtz_generic.hip); beyond, SF_ENOTBUILT.
#include "any_extent.h"

namespace sf
{

constexpr unsigned kDiagMax3D = 12, kDiagMax2D = 32;
constexpr int kDiagSmallCap = 2048, kDiagLargeCap = 6144; // scalars

inline unsigned diag_need(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    return dim == 3 ? (nq2 - 1) * nq1 * nq0 + 3 * (nq2 - 1) * (nq1 - 1) * nq0 : 3 * (nq1 - 1) * nq0;
}

// a = sum_{m < n} (lam * w[m*ws]) * b[m], ascending m, the first product a multiply
template <typename T> __device__ __forceinline__ T dot_scaled(T lam, const T *w, int ws, const T *b, int n)
{
    T a = (lam * w[0]) * b[0];
    for (int m = 1; m < n; ++m)
        a = sfma(lam * w[m * ws], b[m], a);
    return a;
}

template <typename T, int DIM, int CAP, int NT>
__global__ __launch_bounds__(NT) void diag_generic_kernel(const T *__restrict__ t0, const T *__restrict__ t1,
                                                          const T *__restrict__ t2, const T *__restrict__ g,
                                                          const T *__restrict__ w, T lam, bool has_w,
                                                          T *__restrict__ out, uint64_t nelmt, int nq0, int nq1, int nq2)
{
    __shared__ T lds[CAP];
#include "frag/ae_prologue.inc"
    // table t of direction d: row-major nm_d x nq_d
    const int ts0 = nm0 * nq0, ts1 = nm1 * nq1;
    for (uint64_t e = blockIdx.x; e < nelmt; e += gridDim.x)
    {
        T *dst = out + e * (uint64_t)nmt;
        if constexpr (DIM == 3)
        {
            const int ts2 = nm2 * nq2;
            const T *ge   = g + e * (uint64_t)(6 * nqt);
            const T *we   = has_w ? w + e * (uint64_t)nqt : nullptr;
            T *img        = lds;              // t1[r][j][i] of one term
            T *B          = lds + nm2 * n01;  // B^{s0}[r][q][i], s0 = 0, 1, 2
            const int nb  = nm2 * nm1 * nq0;
            // planes in the order of g: (00, 01, 02, 11, 12, 22); their tables (s2, s1, s0)
            constexpr int S2[6] = {0, 0, 1, 0, 1, 2}, S1[6] = {0, 1, 0, 2, 1, 0}, S0[6] = {2, 1, 1, 0, 0, 0};
            for (int c = 0; c < 6; ++c)
            {
                // k -> r: t1[r][j][i] = sum_k g_c[k][j][i] T2^{s2}[r][k]
                const T *tab = t2 + S2[c] * ts2;
                for (int x = tid; x < n01 * nm2; x += NT)
                {
                    const int ji = x % n01, r = x / n01;
                    T a          = dot_strided(ge + c * nqt + ji, n01, tab + r * nq2, 1, nq2);
                    if (c == 1 || c == 2 || c == 4)
                        a = a + a; // the symmetric pair is stored once
                    if (c == 5 && has_w)
                        a = a + dot_scaled(lam, we + ji, n01, t2 + r * nq2, nq2);
                    img[x] = a;
                }
                __syncthreads();
                // j -> q, added to the image of the direction-0 table
                const T *tb = t1 + S1[c] * ts1;
                T *Bs       = B + S0[c] * nb;
                const bool first = c == 0 || c == 1 || c == 3;
                for (int x = tid; x < nb; x += NT)
                {
                    const int i = x % nq0, rq = x / nq0, q = rq % nm1, r = rq / nm1;
                    const T a   = dot_strided(img + r * n01 + i, nq0, tb + q * nq1, 1, nq1);
                    Bs[x]       = first ? a : Bs[x] + a;
                }
                __syncthreads();
            }
            // i -> p: the three images, added in the order s0 = 0, 1, 2
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, rq = x / nm0;
                const T a0  = dot_strided(B + rq * nq0, 1, t0 + p * nq0, 1, nq0);
                const T a1  = dot_strided(B + nb + rq * nq0, 1, t0 + ts0 + p * nq0, 1, nq0);
                const T a2  = dot_strided(B + 2 * nb + rq * nq0, 1, t0 + 2 * ts0 + p * nq0, 1, nq0);
                dst[x]      = (a0 + a1) + a2;
            }
            __syncthreads(); // the images are rewritten by the next element
        }
        else
        {
            const T *ge  = g + e * (uint64_t)(3 * nqt);
            const T *we  = has_w ? w + e * (uint64_t)nqt : nullptr;
            T *B         = lds; // B^{s0}[q][i]
            const int nb = nm1 * nq0;
            // j -> q: planes (00, 01, 11) with the direction-1 tables 0, 1, 2, into the images s0 = 2, 1, 0
            for (int x = tid; x < nb; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                B[2 * nb + x] = dot_strided(ge + i, nq0, t1 + q * nq1, 1, nq1);
                const T a1    = dot_strided(ge + nqt + i, nq0, t1 + ts1 + q * nq1, 1, nq1);
                B[nb + x]     = a1 + a1;
                T a0          = dot_strided(ge + 2 * nqt + i, nq0, t1 + 2 * ts1 + q * nq1, 1, nq1);
                if (has_w)
                    a0 = a0 + dot_scaled(lam, we + i, nq0, t1 + q * nq1, nq1);
                B[x] = a0;
            }
            __syncthreads();
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, q = x / nm0;
                const T a0  = dot_strided(B + q * nq0, 1, t0 + p * nq0, 1, nq0);
                const T a1  = dot_strided(B + nb + q * nq0, 1, t0 + ts0 + p * nq0, 1, nq0);
                const T a2  = dot_strided(B + 2 * nb + q * nq0, 1, t0 + 2 * ts0 + p * nq0, 1, nq0);
                dst[x]      = (a0 + a1) + a2;
            }
            __syncthreads();
        }
    }
}

template <int DIM, typename T>
int launch_diag_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s)
{
    return launch_any_extent(diag_generic_built(DIM, nq[0], nq[1], nq[2]),
                             diag_need(DIM, nq[0], nq[1], nq[2]) <= (unsigned)kDiagSmallCap,
                             diag_generic_kernel<T, DIM, kDiagSmallCap, 64>, diag_generic_kernel<T, DIM, kDiagLargeCap, 256>,
                             a.nelmt, s, a.b0, a.b1, basis2(a), x.g, x.w, x.lam, x.w != nullptr, a.out, a.nelmt, (int)nq[0],
                             (int)nq[1], (int)nq[2]);
}
template int launch_diag_generic<3, double>(const unsigned (&)[3], const HexArgs &, const DiagArgsT<double> &, hipStream_t);
template int launch_diag_generic<3, float>(const unsigned (&)[3], const HexArgsT<float> &, const DiagArgsT<float> &,
                                           hipStream_t);
template int launch_diag_generic<2, double>(const unsigned (&)[3], const QuadArgs &, const DiagArgsT<double> &, hipStream_t);
template int launch_diag_generic<2, float>(const unsigned (&)[3], const QuadArgsT<float> &, const DiagArgsT<float> &,
                                           hipStream_t);

// within the extent bounds AND the images fit the large LDS class (derived, not assumed)
bool diag_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2)
{
    const unsigned mx = dim == 3 ? kDiagMax3D : kDiagMax2D;
    if (nq0 < 2 || nq1 < 2 || (dim == 3 && nq2 < 2) || nq0 > mx || nq1 > mx || (dim == 3 && nq2 > mx))
        return false;
    return diag_need(dim, nq0, nq1, dim == 3 ? nq2 : 0) <= (unsigned)kDiagLargeCap;
}

// ---- sf_diag_tables_*: the three tables of one direction ---------------------------------------------------------------
// One thread per (p, i): E = sum_m deriv[i*nq + m] basis[p*nq + m], ascending m, the first product a multiply, then FMAs;
// the tables are single products.
template <typename T>
__global__ __launch_bounds__(256) void diag_tables_kernel(const T *__restrict__ basis, const T *__restrict__ deriv,
                                                          T *__restrict__ tab, unsigned nq)
{
    const unsigned n = (nq - 1) * nq;
    const unsigned x = blockIdx.x * 256u + threadIdx.x;
    if (x >= n)
        return;
    const unsigned p = x / nq, i = x - p * nq;
    const T E        = dot_strided(deriv + (size_t)i * nq, 1, basis + (size_t)p * nq, 1, (int)nq);
    const T b        = basis[x];
    tab[x]                 = b * b;
    tab[(size_t)n + x]     = E * b;
    tab[2 * (size_t)n + x] = E * E;
}

template <typename T> int launch_diag_tables(unsigned nq, const T *basis, const T *deriv, T *tab, hipStream_t s)
{
    const unsigned n = (nq - 1) * nq;
    diag_tables_kernel<T><<<(n + 255) / 256, 256, 0, s>>>(basis, deriv, tab, nq);
    return launch_rc();
}
template int launch_diag_tables<double>(unsigned, const double *, const double *, double *, hipStream_t);
template int launch_diag_tables<float>(unsigned, const float *, const float *, float *, hipStream_t);

} // namespace sf
