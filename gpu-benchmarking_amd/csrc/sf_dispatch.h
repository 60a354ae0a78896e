// sf_dispatch.h -- internal launch / helper entry points shared between the C ABI (capi.hip) and the
// translation units that define them (bwdtrans_hex.hip, bwdtrans_quad.hip, bwdtrans_generic.hip, bwdtrans_rt.hip,
// aux_kernels.hip, rtc.hip and those of the fused operators).  Every function returns SF_OK, a negative SF_E* code or a
// positive hipError_t.
#pragma once

#include "sf_common.h"

#include <mutex>
#include <type_traits>

namespace sf
{
template <int DIM, typename T> using ArgsT = typename std::conditional<DIM == 3, HexArgsT<T>, QuadArgsT<T>>::type;
// what the launch just enqueued answered
inline int launch_rc()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SF_OK : (int)e;
}
// BwdTrans, one set of entry points for both dimensions and both scalar types, each specialised in the translation unit
// that holds its kernels (bwdtrans_hex.hip <3, T>, bwdtrans_quad.hip <2, T>, bwdtrans_generic.hip all four).  The order
// tables of one kernel family, T = double only (SF_ENOTBUILT off the table): the wave kernel (3D nq 2..11, 2D 2..24 and
// 32), the 16x16x4 matrix-core kernel (3D 4..16, 2D 11..32), the 4x4x4_4b matrix-core kernel (3D 12..16, 2D 8..32).
template <int DIM, typename T> int launch_bwd_wave(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s);
template <int DIM, typename T> int launch_bwd_mfma(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s);
template <int DIM, typename T> int launch_bwd_mfma4(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s);
// the 3D 4x4x4_4b kernel with its output path named: the element assembled in LDS and streamed out flat, or (direct) the
// sweep-3 accumulators stored as they are; launch_bwd_mfma4<3, double> picks per order (sf_bwdtrans_hex_f64_mfma4)
int launch_hex_mfma4_path(bool direct, unsigned nq, const HexArgs &a, hipStream_t s);
// what SF_VARIANT_AUTO runs for an isotropic order on 16-byte-aligned in / out: the measured best kernel of the order,
// then whatever else is built for it (SF_ENOTBUILT: nothing is); double and float
template <int DIM, typename T> int launch_bwd_iso_auto(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s);
// the any-extent kernels and the reference's decompositions (SF_VARIANT_GENERIC / THREAD / BLOCK_LDS / BLOCK_GLB; nq[2]
// is 0 in 2D); double and float
template <int DIM, typename T>
int launch_bwd_generic(int variant, const unsigned (&nq)[3], const ArgsT<DIM, T> &a, hipStream_t s);
int launch_hex_wave3(unsigned nq0, unsigned nq1, unsigned nq2, const HexArgs &a, hipStream_t s);
int launch_hex_rt(unsigned nq0, unsigned nq1, unsigned nq2, const HexArgs &a, hipStream_t s);
int sumsq_async(const double *x, size_t n, double *result_dev, hipStream_t s);
int sumsq_blocking(const double *x, size_t n, double *result_host, hipStream_t s);
int fill_sincos(double *in, size_t nelmt, size_t nm_tot, hipStream_t s);
int fill_basis(double *b, size_t nm, size_t nq, hipStream_t s);
int fill_random(double *x, size_t n, uint64_t seed, uint64_t first, hipStream_t s);
int fill_l2norm(double *x, size_t n, hipStream_t s);
int stream_copy(const double *src, double *dst, size_t n, hipStream_t s);
int vector_add(double *x, const double *y, size_t n, hipStream_t s);
int fill_vecadd(double *x, double *y, size_t n, hipStream_t s);
int matvec(unsigned M, unsigned N, const double *A, const double *x, double *y, hipStream_t s);
int fill_matvec(double *A, double *x, unsigned M, unsigned N, hipStream_t s);
int release_workspaces();
// internal scratch buffer of (current device, stream, kind), at least `bytes` long; kinds: 0 reductions, 1 BwdTrans
// intermediates, 2 the gather-scatter setup.  Hold scratch_mutex() from the acquire to the end of the enqueue sequence that uses the buffer.
int scratch_acquire(hipStream_t s, int kind, size_t bytes, void **out);
std::recursive_mutex &scratch_mutex();
// 8-byte batch counter for one launch of a persistent kernel on `s` (zero it with a one-thread kernel in front of the
// launch: wave_launch.h counter_reset_kernel).  Counters live in one buffer per device that is allocated at first use and
// freed only by sf_shutdown().  Eager launches on a stream share that stream's counter (their work is ordered); a launch
// enqueued while `s` is capturing gets a counter of its own (the graph may replay on any stream).  SF_ENOMEM: none to be
// had -- fall back.  Hold counter_mutex() (of the current device) from the acquire to the launch of the kernel that draws
// from the counter: two host threads on one stream may not interleave their resets and kernels.
int counter_acquire(hipStream_t s, unsigned long long **out);
std::mutex &counter_mutex();
int release_counters();
int set_launch_hint(unsigned threads, unsigned elblocks);
int launch_hex_interleaved(unsigned nq0, unsigned nq1, unsigned nq2, const HexArgs &a, hipStream_t s);
int launch_interleave64(const double *src, double *dst, size_t nelmt, size_t n, int inverse,
                        hipStream_t s);
// run-time specialisation (rtc.hip): sf_specialise / sf_specialisation_state / the launch of a ready module (SF_ENOTBUILT
// unless one of the shape is ready on the current device) / the calling thread's last compile log / sf_shutdown's part
int rtc_specialise(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes);
int rtc_state(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, uint64_t *launches);
int launch_specialised(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, const void *b0,
                       const void *b1, const void *b2, const void *in, void *out, uint64_t nelmt, hipStream_t s);
const char *rtc_last_log();
int rtc_release();
// IProductWRTBase, the fused mass operator and the fused Helmholtz operator have one pair of entry points each, for both
// dimensions and both scalar types: the wave kernels of an isotropic order (SF_ENOTBUILT off their table) and the
// any-extent kernels (nq[2] is 0 in 2D; SF_ENOTBUILT beyond their bounds).  Each is defined for <3, T> and <2, T> in the
// translation unit that holds the kernels of T.
// IProductWRTBase (iproduct.hip: the wave kernels, 3D nq 2..11, 2D 2..16; iproduct_generic.hip: any extents up to 16 per
// direction in 3D and 32 in 2D)
template <int DIM, typename T> int launch_iprod_wave(unsigned nq, const ArgsT<DIM, T> &a, hipStream_t s);
template <int DIM, typename T> int launch_iprod_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, hipStream_t s);
bool iprod_wave_built(int dim, unsigned nq);
bool iprod_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// The tensor-product apply with independent input / output extents, out = (M2 (x) M1 (x) M0) in (tensor.hip,
// tensor_quad.hip and their _f32 twins: the wave kernels of the table in tensor_launch.h; tensor_generic.hip: any extents
// from 1 up to 16 per direction in 3D and 32 in 2D; rtc.hip: a wave kernel compiled at run time for one shape).  ni[2] and
// no[2] are 1 in 2D; a.b0 .. a.b2 are the matrices, row-major ni x no (trans 0) or no x ni (trans 1); a.wsp is not used.
template <int DIM, typename T>
int launch_tensor_wave(const unsigned (&ni)[3], const unsigned (&no)[3], int trans, const ArgsT<DIM, T> &a, hipStream_t s);
template <int DIM, typename T>
int launch_tensor_generic(const unsigned (&ni)[3], const unsigned (&no)[3], int trans, const ArgsT<DIM, T> &a,
                          hipStream_t s);
bool tensor_wave_built(int dim, const unsigned (&ni)[3], const unsigned (&no)[3]);
bool tensor_generic_built(int dim, const unsigned (&ni)[3], const unsigned (&no)[3]);
int rtc_specialise_tensor(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes);
int rtc_tensor_state(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes,
                     uint64_t *launches);
int launch_tensor_specialised(int dim, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, int scalar_bytes,
                              const void *m0, const void *m1, const void *m2, const void *in, void *out, uint64_t nelmt,
                              hipStream_t s);
// The fused mass operator B^T diag(w) B (mass.hip / mass_f32.hip: the wave kernels of mass_wave.h, 3D nq 2..11, 2D 2..16;
// mass_generic.hip: any extents up to 16 per direction in 3D and 32 in 2D).  `w`: one weight per quadrature point per
// element; a.wsp is not used.
template <int DIM, typename T>
int launch_mass_wave(unsigned nq, const ArgsT<DIM, T> &a, const T *w, hipStream_t s);
template <int DIM, typename T>
int launch_mass_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const T *w, hipStream_t s);
bool mass_wave_built(int dim, unsigned nq);
bool mass_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// The fused Helmholtz operator B^T [lambda diag(w) + sum_ab D_a^T diag(G_ab) D_b] B (helmholtz.hip / helmholtz_f32.hip:
// the wave kernels of helmholtz_wave.h, 3D nq 2..8, 2D 2..16; helmholtz_generic.hip: any extents up to 12 per direction
// in 3D and 32 in 2D).  What the operator takes beyond the BwdTrans arguments: the derivative matrices, the metric
// planes, the mass weight (null: lambda == 0, never read) and lambda in the scalar type.
template <typename T> struct HelmArgsT
{
    const T *d0, *d1, *d2, *g, *w;
    T lam;
};
template <int DIM, typename T>
int launch_helmholtz_wave(unsigned nq, const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_helmholtz_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const HelmArgsT<T> &x, hipStream_t s);
bool helmholtz_wave_built(int dim, unsigned nq);
bool helmholtz_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// The fused Helmholtz operator on affine elements, G_ab,e = ge[e][ab] (x) qw, w_e = je[e] (x) qw (affine.hip /
// affine_f32.hip: the wave kernels of affine_wave.h, the Helmholtz table; affine_generic.hip: any extents up to 12 per
// direction in 3D and 32 in 2D).  What the operator takes beyond the BwdTrans arguments: the derivative matrices, the
// one-dimensional quadrature weights, the constants of every element (je null: lambda == 0, never read) and lambda in
// the scalar type.
template <typename T> struct AffineArgsT
{
    const T *d0, *d1, *d2, *qw0, *qw1, *qw2, *ge, *je;
    T lam;
};
template <int DIM, typename T>
int launch_affine_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_affine_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineArgsT<T> &x, hipStream_t s);
bool affine_wave_built(int dim, unsigned nq);
bool affine_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// BwdTrans fused with the physical-space gradient, out_a = sum_b df_ab D_b B x (physderiv.hip / physderiv_f32.hip: the
// wave kernels of physderiv_wave.h, the Helmholtz table; physderiv_generic.hip: any extents up to 12 per direction in 3D
// and 32 in 2D).  What the operator takes beyond the BwdTrans arguments: the derivative matrices, the d*d planes of the
// inverse Jacobian (null: never read, the reference-space derivatives) and its d outputs -- `out` of the BwdTrans
// arguments is not used.
template <typename T> struct PhysDerivArgsT
{
    const T *d0, *d1, *d2, *df;
    T *out0, *out1, *out2;
};
template <int DIM, typename T>
int launch_physderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_physderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const PhysDerivArgsT<T> &x, hipStream_t s);
bool physderiv_wave_built(int dim, unsigned nq);
bool physderiv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// IProductWRTDerivBase, out = sum_b B^T D_b^T (w sum_a df_ab in_a), the transpose of the gradient above (iprodderiv.hip /
// iprodderiv_f32.hip: the wave kernels of iprodderiv_wave.h, the Helmholtz table; iprodderiv_generic.hip: any extents up
// to 12 per direction in 3D and 32 in 2D).  What the operator takes beyond the BwdTrans arguments: the derivative
// matrices, the d*d planes of the inverse Jacobian (null: never read), the weight plane (null: never read) and its d
// inputs -- `in` of the BwdTrans arguments is not used.  The wave launcher carries one switch (df); the weight picks one
// of two argument structs.
template <typename T> struct IprodDerivArgsT
{
    const T *d0, *d1, *d2, *df, *w;
    const T *in0, *in1, *in2;
};
template <typename T> struct IprodDerivWArgsT : IprodDerivArgsT<T> // w is not null
{
};
template <int DIM, typename T>
int launch_iprodderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const IprodDerivArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_iprodderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const IprodDerivArgsT<T> &x, hipStream_t s);
bool iprodderiv_wave_built(int dim, unsigned nq);
bool iprodderiv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// The gradient and the weak divergence on affine elements, df_ab = dfe[e][a*d + b] at every point and w_e = je[e] (x) qw
// (affine_deriv.hip / affine_deriv_f32.hip: the wave kernels of affine_deriv_wave.h, the Helmholtz table;
// affine_deriv_generic.hip: any extents up to 12 per direction in 3D and 32 in 2D).  The gradient takes what
// sf_physderiv_* takes with the d*d constants of every element in the place of the planes (required); the weak divergence
// what sf_iprodderiv_* takes with dfe, the one-dimensional quadrature weights and je (null: no weight, je and qw_d never
// read).  One pair of `built` answers serves both operators.
template <typename T> struct AffinePhysDerivArgsT
{
    const T *d0, *d1, *d2, *dfe;
    T *out0, *out1, *out2;
};
template <typename T> struct AffineIprodDerivArgsT
{
    const T *d0, *d1, *d2, *qw0, *qw1, *qw2, *dfe, *je;
    const T *in0, *in1, *in2;
};
template <int DIM, typename T>
int launch_affine_physderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffinePhysDerivArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_affine_physderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffinePhysDerivArgsT<T> &x,
                                    hipStream_t s);
template <int DIM, typename T>
int launch_affine_iprodderiv_wave(unsigned nq, const ArgsT<DIM, T> &a, const AffineIprodDerivArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_affine_iprodderiv_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const AffineIprodDerivArgsT<T> &x,
                                     hipStream_t s);
bool affine_deriv_wave_built(int dim, unsigned nq);
bool affine_deriv_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// The diagonal of the fused Helmholtz operator, diag(B^T [lambda diag(w) + sum_ab D_a^T diag(G_ab) D_b] B) (diag.hip /
// diag_f32.hip: the wave kernels of diag_wave.h, the Helmholtz table; diag_generic.hip: any extents up to 12 per direction
// in 3D and 32 in 2D, and the kernel that forms the tables).  There is no input array: b0 .. b2 of the BwdTrans arguments
// are the table triples tab_d[t][p][i] of sf_diag_tables_*, `in` is not used.  Beyond them: the metric planes, the mass
// weight (null: lambda == 0, never read) and lambda in the scalar type.
template <typename T> struct DiagArgsT
{
    const T *g, *w;
    T lam;
};
template <int DIM, typename T>
int launch_diag_wave(unsigned nq, const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s);
template <int DIM, typename T>
int launch_diag_generic(const unsigned (&nq)[3], const ArgsT<DIM, T> &a, const DiagArgsT<T> &x, hipStream_t s);
bool diag_wave_built(int dim, unsigned nq);
bool diag_generic_built(int dim, unsigned nq0, unsigned nq1, unsigned nq2);
// tab[t][p][i], t = 0, 1, 2: B o B, E o B, E o E with E[p][i] = sum_m deriv[i*nq + m] basis[p*nq + m]; one kernel
template <typename T> int launch_diag_tables(unsigned nq, const T *basis, const T *deriv, T *tab, hipStream_t s);
// Gather-scatter (gs.hip): the setup that inverts a local-to-global map into rows / perm (blocking; integer atomics, a
// three-kernel scan, scratch kind 2) and the three apply launches, one kernel each; sign null: all +1.
int gs_setup(size_t nlocal, size_t nglobal, const int32_t *l2g, int32_t *rows, int32_t *perm, hipStream_t s);
template <typename T>
int launch_global_to_local(size_t nlocal, const int32_t *l2g, const T *sign, const T *global, T *local, hipStream_t s);
template <typename T>
int launch_assemble(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, const T *local, T *global,
                    hipStream_t s);
template <typename T>
int launch_gs(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, T *local, hipStream_t s);
int sumsq_f32_blocking(const float *x, size_t n, double *result_host, hipStream_t s);
int fill_sincos_f32(float *in, size_t nelmt, size_t nm_tot, hipStream_t s);
int fill_basis_f32(float *b, size_t nm, size_t nq, hipStream_t s);
int fill_random_f32(float *x, size_t n, uint64_t seed, uint64_t first, hipStream_t s);
} // namespace sf
