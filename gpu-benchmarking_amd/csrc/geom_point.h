// geom_point.h -- the geometric factors of ONE quadrature point from its Jacobian, the text that the wave kernels of
// geom_wave.h, the any-extent kernel and the affine kernel of geom_generic.hip share, so that every route rounds alike.
//
//   J[a][b] = d x_a / d xi_b   ->   df[a*d + b] = d xi_b / d x_a,  det J,  w = |det J| q,  G_ab = w sum_x df[x*d+a] df[x*d+b]
//
// Order of operations (steps 3-7 of sf_geom_* in include/sumfact.h; every sum in ascending index, the first product a
// multiply, then FMAs -- every FMA is named, nothing is left to contraction):
//   3. 3D: cof[a][b] = fma(J[a+1][b+1], J[a+2][b+2], -(J[a+1][b+2] * J[a+2][b+1])), indices mod 3
//      2D: cof = (J11, -J10, -J01, J00) in the order of c
//   4. det = J[0][0] * cof[0][0], then fma(J[0][b], cof[0][b], det) for b = 1 [, 2]
//   5. r = 1 / det (a correctly rounded division), df[a*d + b] = cof[a][b] * r
//   6. w = |det| * q            (q: the product of the quadrature weights, formed by the caller; SCALED false: w = |det|)
//   7. G_ab = w * (sum_x df[x*d + a] * df[x*d + b]), x ascending, (a, b) in the order 00, 01, 02, 11, 12, 22 / 00, 01, 11
// det == 0 gives inf / NaN at this point; nothing is refused.
#pragma once

namespace sf
{

__device__ __forceinline__ double geom_fma(double a, double b, double c)
{
    return __builtin_fma(a, b, c);
}
__device__ __forceinline__ float geom_fma(float a, float b, float c)
{
    return __builtin_fmaf(a, b, c);
}
__device__ __forceinline__ double geom_abs(double a)
{
    return __builtin_fabs(a);
}
__device__ __forceinline__ float geom_abs(float a)
{
    return __builtin_fabsf(a);
}

// which outputs a kernel instantiation can write
constexpr int kGeomDf = 1, kGeomW = 2, kGeomG = 4, kGeomDet = 8, kGeomAll = 15;

template <int DIM, typename T> struct GeomPoint
{
    T df[DIM * DIM], g[DIM * (DIM + 1) / 2], w, det;
};

// MASK: what the caller will read of p -- the rest may hold anything and its arithmetic is not generated
template <int DIM, int MASK, bool SCALED, typename T>
__device__ __forceinline__ void geom_point(const T (&J)[DIM][DIM], T q, GeomPoint<DIM, T> &p)
{
    T cof[DIM][DIM];
    if constexpr (DIM == 3)
    {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b)
            {
                const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
                cof[a][b] = geom_fma(J[a1][b1], J[a2][b2], -(J[a1][b2] * J[a2][b1]));
            }
    }
    else
    {
        cof[0][0] = J[1][1];
        cof[0][1] = -J[1][0];
        cof[1][0] = -J[0][1];
        cof[1][1] = J[0][0];
    }
    T det = J[0][0] * cof[0][0];
#pragma unroll
    for (int b = 1; b < DIM; ++b)
        det = geom_fma(J[0][b], cof[0][b], det);
    p.det = det;
    if constexpr ((MASK & (kGeomDf | kGeomG)) != 0)
    {
        const T r = T(1) / det;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b)
                p.df[a * DIM + b] = cof[a][b] * r;
    }
    if constexpr ((MASK & (kGeomW | kGeomG)) != 0)
        p.w = SCALED ? geom_abs(det) * q : geom_abs(det);
    if constexpr ((MASK & kGeomG) != 0)
    {
        int c = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = a; b < DIM; ++b, ++c)
            {
                T sum = p.df[a] * p.df[b];
#pragma unroll
                for (int x = 1; x < DIM; ++x)
                    sum = geom_fma(p.df[x * DIM + a], p.df[x * DIM + b], sum);
                p.g[c] = p.w * sum;
            }
    }
}

} // namespace sf
