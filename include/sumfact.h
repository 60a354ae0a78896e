/*
 * include/sumfact.h -- C ABI of libsumfact.so, the MI355X (gfx950) drop-in for the BwdTrans
 * sum-factorisation hot path of CFD-Xing/gpu-benchmarking.
 *
 * The reference has no FFI: its "interface" for this path is the kernel call a maintainer makes from
 * run_test<T> (benchmark05/benchmark05.cc:1322-1328, benchmark04/benchmark04.cc:1001-1004): raw
 * device pointers + unsigned extents, caller owns every buffer, the kernel allocates nothing.  Each
 * entry point below replaces one such call site (cited per function).  INTEGRATION.md shows the
 * exact edit in the reference's run_test.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - layouts are the reference's: in[e][r][q][p] (p fastest), out[e][k][j][i] (i fastest),
 *     basis[p*nq + i] row-major nm x nq, nm = nq - 1;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream, as in the reference);
 *     launches are asynchronous, like a <<<>>> launch; the caller synchronises.  One call may enqueue SEVERAL kernels on
 *     `stream` (a 3D nq = 7 / 8 batch above 1 048 576 elements goes out as launches of 524 288 elements each: elements are
 *     independent and the pieces re-align the chip's eight XCDs, +2 % from 2.5 M elements); results do not depend on it;
 *   - element counts are size_t (the reference's 32-bit `unsigned` overflows at
 *     nelmt*nq^3 > 2^32, i.e. above 8 388 608 elements at nq = 8);
 *   - return value: 0 on success, a positive hipError_t, or a negative SF_E* code.  The reference
 *     reports no errors at all; nothing here aborts the process;
 *   - thread / stream safety: every entry point may be called concurrently from several host threads and on several
 *     streams of a device (sf_set_launch_hint is per calling thread).  Several host threads may launch on the SAME
 *     stream (the null stream included): what one call enqueues around the library's internal memory (scratch, batch
 *     counter, the copy of a reduction's result) stays one unit on the stream, never interleaved with that of another
 *     thread's call.  The library's internal device memory:
 *     (i) reduction partials of sf_sumsq_* and the intermediates of the any-extent fallback (at most 1 GiB, the grid
 *     is cut down to fit) live in a scratch buffer per (device, stream; per thread for hipStreamPerThread), allocated
 *     on the first call that needs it on that stream -- that FIRST call may not be inside a stream capture;
 *     (ii) the batch counters of the persistent 2D kernels (AUTO 2D nq 25..32) live in one 512 KiB buffer per device
 *     that is allocated once and freed only by sf_shutdown(): BwdTrans launches are capture-safe from the first call
 *     (kernel nodes only -- a kernel zeroes the counter; inside a capture that precedes the buffer's allocation the
 *     same kernel runs with a fixed share per wave instead), and a captured graph stays replayable until sf_shutdown().
 */
#ifndef SUMFACT_H
#define SUMFACT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_VERSION 100

enum
{
    SF_OK        = 0,
    SF_EINVAL    = -1, /* nq < 2, null pointer with nelmt > 0, unknown variant */
    SF_EALIGN    = -2, /* in/out not 8-byte aligned */
    SF_ENOTBUILT = -3, /* requested variant has no instantiation for this nq */
    SF_ENOMEM    = -4, /* internal workspace allocation failed */
    SF_ECOMPILE  = -5  /* run-time specialisation unavailable: hiprtc missing, compile failed, or it would spill */
};

/* Kernel strategies (benchmark columns / tuning).  SF_VARIANT_AUTO picks the fastest measured: 3D isotropic nq 2..11
 * WAVE, 12 / 14 / 16 MFMA4, 13 / 15 MFMA; 2D isotropic nq 2..20 WAVE, 21..31 MFMA4, 32 MFMA; 3D anisotropic extents: WAVE where the shape
 * is one of the compile-time triples of csrc/bwdtrans_rt.hip, else WAVE_RT up to nq = 8 per direction (also taken for
 * isotropic shapes in buffers that are only 8-byte aligned); anything else (2D anisotropic, any higher order) GENERIC,
 * which runs every extent: LDS-resident while one element's images fit the
 * 160 KiB of LDS, then through a bounded internal scratch (one intermediate pair per workgroup; first use on a
 * stream allocates, so it is not stream-capture safe; SF_ENOMEM if that allocation fails). */
enum
{
    SF_VARIANT_AUTO       = 0,
    SF_VARIANT_WAVE       = 1, /* flagship: one wavefront per chunk of elements (3D nq 2..11, 2D nq 2..24, 32) */
    SF_VARIANT_THREAD     = 2, /* one thread per element, fused nest  (cf. benchmark05.cc:15-102)  */
    SF_VARIANT_BLOCK_LDS  = 3, /* one workgroup per element, 3 sweeps in LDS (cf. :291-429)       */
    SF_VARIANT_BLOCK_GLB  = 4, /* one workgroup per element, global workspace (cf. :203-289)       */
    SF_VARIANT_GENERIC    = 5, /* runtime-nq fallback (anisotropic nq0 != nq1 != nq2)              */
    SF_VARIANT_MFMA       = 6, /* v_mfma_f64_16x16x4 chained GEMMs: 2D quad nq 11..32, 3D hex nq 4..16 */
    SF_VARIANT_MFMA4      = 7, /* v_mfma_f64_4x4x4_4b chained products (tile granularity 4): 2D quad nq 8..32, 3D hex nq 12..16 */
    SF_VARIANT_WAVE_RT    = 8, /* one wavefront per chunk with RUN-TIME extents: 3D, any extents up to 16 per direction */
    SF_NUM_VARIANTS       = 9
};

int sf_version(void);
const char *sf_error_string(int rc);
const char *sf_variant_name(int variant);

/*
 * 3D hex BwdTrans: out[e][k][j][i] = sum_r sum_q sum_p in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k].
 * Replaces BwdTransHexKernel_QP<<<blocks, dim3(...), smem>>>(nm0,nm1,nm2,nmTot,nq0,nq1,nq2,nelmt,
 * d_basis0,d_basis1,d_basis2,d_in,d_out)  -- benchmark05/benchmark05.cc:1322-1328 (and the other
 * five launches :1265, :1283, :1300, :1342, :1362, which compute the same result).
 */
int sf_bwdtrans_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                        const double *basis0, const double *basis1, const double *basis2,
                        const double *in, double *out, void *stream);

/* Same, with an explicit strategy; wsp (may be NULL) is only used by SF_VARIANT_BLOCK_GLB and
 * SF_VARIANT_THREAD and must then hold nelmt*(nq0*nm1*nm2 + nq0*nq1*nm2) doubles (benchmark05.cc:1243-1244). */
int sf_bwdtrans_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2,
                                size_t nelmt, const double *basis0, const double *basis1,
                                const double *basis2, const double *in, double *wsp, double *out,
                                void *stream);

/* For tests and tuning: the SF_VARIANT_MFMA4 kernel of the isotropic order nq with its output path named.  direct == 0
 * assembles the element in LDS and streams it out flat; direct != 0 stores the accumulators of the third sweep as they
 * are.  SF_VARIANT_AUTO and SF_VARIANT_MFMA4 keep choosing the path per order (direct at nq = 16 only).  For the same
 * arguments it answers what sf_bwdtrans_hex_f64_variant(SF_VARIANT_MFMA4, nq, nq, nq, ..., wsp = NULL, ...) answers: the
 * same validation, SF_EALIGN unless in / out are 16-byte aligned, SF_ENOTBUILT (before any HIP call) outside nq 12..16. */
int sf_bwdtrans_hex_f64_mfma4(int direct, unsigned nq, size_t nelmt, const double *basis0,
                              const double *basis1, const double *basis2, const double *in,
                              double *out, void *stream);

/*
 * 2D quad BwdTrans: out[e][j][i] = sum_q sum_p in[e][q][p] B0[p][i] B1[q][j].
 * Replaces BwdTransQuadKernel_QP_1D<<<blocks, threads, smem>>>(nm0,nm1,nmTot,nq0,nq1,nelmt,
 * d_basis0,d_basis1,d_in,d_out) -- benchmark04/benchmark04.cc:1001-1004 (and :912, :930, :947,
 * :966, :983).
 */
int sf_bwdtrans_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                         const double *basis1, const double *in, double *out, void *stream);

int sf_bwdtrans_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                                 const double *basis0, const double *basis1, const double *in,
                                 double *wsp, double *out, void *stream);

/*
 * sum_i x[i]^2 -> *result_host (blocking: synchronises `stream`).  Deterministic (fixed-shape
 * two-pass tree).  Replaces thrust::transform_reduce(d_out, d_out + n, x*x, 0, plus)
 * -- benchmark05/benchmark05.cc:1273-1276 -- and bm01's l2norm kernels
 * (benchmark01/benchmark01.cc:245-253).
 */
int sf_sumsq_f64(const double *x, size_t n, double *result_host, void *stream);

/* Same reduction, result left on the device (result_dev[0]); asynchronous. */
int sf_sumsq_f64_async(const double *x, size_t n, double *result_dev, void *stream);

/*
 * Device-side initialisers (the reference fills on the host and copies:
 * benchmark05/benchmark05.cc:1195-1258).
 *   sincos : in[e*nm_tot + f] = sin(f + 1)                      (:1206-1207)
 *   basis  : basis[x] = cos(x), x < nm*nq                        (:1220)
 *   random : x[i] = U[-1,1) from splitmix64(seed, first_idx + i) (not in the reference; identical
 *            to oracle_fill_random so host and device arrays agree bit for bit)
 *   l2norm : x[i] = i%13 + (0.2 + 1e-5*(i%100191))              (benchmark01/benchmark01.cc:178)
 * sin/cos run on the device's libm: values may differ from glibc's in the last ulp.
 */
int sf_fill_sincos_f64(double *in, size_t nelmt, size_t nm_tot, void *stream);
int sf_fill_basis_f64(double *basis, size_t nm, size_t nq, void *stream);
int sf_fill_random_f64(double *x, size_t n, uint64_t seed, uint64_t first_idx, void *stream);
int sf_fill_l2norm_f64(double *x, size_t n, void *stream);

/*
 * HBM calibrators (benchmark02/benchmark02.cc:16-58 is the reference's analogue):
 * dst[i] = src[i] with 16-byte lanes, n doubles.  Used to report the *measured* stream rate next
 * to the 8 TB/s datasheet roofline.
 */
int sf_stream_copy_f64(const double *src, double *dst, size_t n, void *stream);

/*
 * Wave-64 interleaved element layout: data[(e/64)][f][e%64], padded to whole groups of
 * 64 elements.  One thread per element with fully coalesced accesses: the decomposition of the
 * reference's BwdTransHexKernel_Coa (benchmark05/benchmark05.cc:104-201, launch :1283-1286) for a
 * 64-wide wavefront and without its output-index bug (:193-194).  Sizes in doubles, G = ceil(nelmt/64)*64:
 *   in_il G*nm0*nm1*nm2, out_il G*nq0*nq1*nq2, wsp_il G*(nm1*nm2 + nm2).
 * sf_interleave64_f64 converts element-major [e][n] -> interleaved (inverse = 0) or back (inverse = 1).
 */
int sf_bwdtrans_hex_f64_interleaved(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                    const double *basis0, const double *basis1, const double *basis2,
                                    const double *in_il, double *wsp_il, double *out_il, void *stream);
int sf_interleave64_f64(const double *src, double *dst, size_t nelmt, size_t n, int inverse,
                        void *stream);

/*
 * fp32: the reference's kernels are templates on T but only T = double is ever
 * instantiated (benchmark05/benchmark05.cc:15, 1439); these are the T = float instantiations of the
 * same kernels (float4 lanes).  sumsq accumulates in double.  Same layouts and error codes.
 */
int sf_bwdtrans_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                        const float *basis1, const float *basis2, const float *in, float *out,
                        void *stream);
int sf_bwdtrans_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                         const float *basis1, const float *in, float *out, void *stream);
int sf_sumsq_f32(const float *x, size_t n, double *result_host, void *stream);
int sf_fill_sincos_f32(float *in, size_t nelmt, size_t nm_tot, void *stream);
int sf_fill_basis_f32(float *basis, size_t nm, size_t nq, void *stream);
int sf_fill_random_f32(float *x, size_t n, uint64_t seed, uint64_t first_idx, void *stream);

/*
 * IProductWRTBase, the inner product with respect to the basis: the exact transpose of BwdTrans.
 *   3D: out[e][r][q][p] = sum_k sum_j sum_i in[e][k][j][i] B0[p][i] B1[q][j] B2[r][k]
 *   2D: out[e][q][p]    = sum_j sum_i       in[e][j][i]    B0[p][i] B1[q][j]
 * `in` holds nq0*nq1[*nq2] values per element at the quadrature points (i fastest), `out` nm0*nm1[*nm2] modes per
 * element (p fastest).  The bases are the BwdTrans bases, unchanged: basis[p*nq + i], row-major nm x nq.  Sweeps i -> p,
 * j -> q, k -> r, each sum in ascending index.  Quadrature weights of tensor-product form fold into the bases
 * (B_d'[p][i] = B_d[p][i] * w_d[i]), so the kernels carry no weight array.  BwdTrans -> pointwise weight ->
 * IProductWRTBase is a mass operator: sf_mass_* below runs that chain as ONE kernel (and sf_helmholtz_* the
 * Helmholtz operator; chain the three calls yourself only for what neither covers); this is also the gradient of BwdTrans with respect to
 * its input.
 * Variants: SF_VARIANT_AUTO (the wave kernel for the isotropic orders of its table -- 3D nq 2..11, 2D nq 2..16 -- when
 * in / out are 16-byte aligned, else GENERIC), SF_VARIANT_WAVE (SF_ENOTBUILT off that table, SF_EALIGN unless 16-byte
 * aligned), SF_VARIANT_GENERIC (one workgroup per element, any extents up to 16 per direction in 3D and 32 in 2D);
 * any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  Validation as sf_bwdtrans_*, before any
 * HIP call.  No internal workspace: every call is capture-safe from the first one.
 */
int sf_iproduct_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                        const double *basis0, const double *basis1, const double *basis2,
                        const double *in, double *out, void *stream);
int sf_iproduct_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                const double *basis0, const double *basis1, const double *basis2,
                                const double *in, double *out, void *stream);
int sf_iproduct_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                         const double *basis1, const double *in, double *out, void *stream);
int sf_iproduct_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                                 const double *basis0, const double *basis1, const double *in,
                                 double *out, void *stream);
/* T = float (AUTO route; in / out / bases 4-byte aligned) */
int sf_iproduct_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                        const float *basis1, const float *basis2, const float *in, float *out,
                        void *stream);
int sf_iproduct_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                         const float *basis1, const float *in, float *out, void *stream);

/*
 * The fused mass operator y_e = B^T diag(w_e) B x_e: BwdTrans, a pointwise weight and IProductWRTBase in one kernel.
 *   3D: out[e][r'][q'][p'] = sum_kji B0[p'][i] B1[q'][j] B2[r'][k] * w[e][k][j][i] * (sum_rqp in[e][r][q][p] B0[p][i] B1[q][j] B2[r][k])
 *   2D: out[e][q'][p']     = sum_ji  B0[p'][i] B1[q'][j]           * w[e][j][i]    * (sum_qp  in[e][q][p]    B0[p][i] B1[q][j])
 * `in` and `out` hold nm0*nm1[*nm2] modes per element (p fastest, the BwdTrans input layout); `w` holds nq0*nq1[*nq2]
 * values per element (i fastest, the BwdTrans output layout): one weight per quadrature point per element -- Jacobian
 * determinant times quadrature weights -- so deformed elements are covered.  The bases are the BwdTrans bases,
 * unchanged.  The quadrature-space image never reaches HBM: per element the call moves 2 nm^d + nq^d scalars where the
 * three-call chain moves 2 nm^d + 5 nq^d.
 * Sweep order (it defines the rounding; every sum in ascending index): forward p -> i, q -> j, r -> k as BwdTrans, one
 * multiply by w per point, then the transposed sweeps in REVERSE order, k -> r', j -> q', i -> p' (IProductWRTBase
 * on its own sweeps i, j, k: the fused result and the three-call chain agree to rounding, not bit for bit).
 * Routes: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq 2..11, 2D nq 2..16,
 * the IProductWRTBase table) when in / out are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off
 * that table and SF_EALIGN unless in / out are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per element, latency-
 * bound) takes any extents up to 16 per direction in 3D and 32 in 2D -- 3D nq 12..16 and 2D nq 17..32 have no fused
 * matrix-core kernel yet and take it; any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  `w`
 * and the bases need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, w, in or out: SF_EINVAL; (4) any of them not scalar-aligned:
 * SF_EALIGN; (5) `out` overlapping `in` or `w`, compared as byte ranges of their full sizes: SF_EINVAL; (6) extents
 * beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * The operator is NOT in-place safe and overlap is refused, not undefined: the kernels read 16-byte words that straddle
 * the neighbouring element, which another wave may already have overwritten.  `in` may overlap `w`: both are only read.
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_mass_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                    const double *basis0, const double *basis1, const double *basis2,
                    const double *w, const double *in, double *out, void *stream);
int sf_mass_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                            const double *basis0, const double *basis1, const double *basis2,
                            const double *w, const double *in, double *out, void *stream);
int sf_mass_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                     const double *basis1, const double *w, const double *in, double *out, void *stream);
int sf_mass_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                             const double *basis0, const double *basis1, const double *w,
                             const double *in, double *out, void *stream);
/* T = float (AUTO route; w / in / out / bases 4-byte aligned) */
int sf_mass_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                    const float *basis1, const float *basis2, const float *w, const float *in,
                    float *out, void *stream);
int sf_mass_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                     const float *basis1, const float *w, const float *in, float *out, void *stream);

/*
 * The fused Helmholtz operator, what a Poisson / Helmholtz / implicit-diffusion solve applies every Krylov iteration:
 *   y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e
 * BwdTrans, the collocation derivatives, the per-point metric contraction, the transposed derivatives and
 * IProductWRTBase in ONE kernel; lambda == 0 is the stiffness (Laplacian) operator, g == 0 and lambda == 1 the mass
 * operator of sf_mass_*.  Per element the call moves 2 nm^d + (1 + d(d+1)/2) nq^d scalars; no quadrature-space image
 * reaches HBM.
 * Layout: `in` and `out` hold nm0*nm1[*nm2] modes per element (p fastest, the BwdTrans input layout).  basis_d: the
 * BwdTrans bases, unchanged.  deriv_d: row-major nq_d x nq_d, deriv_d[i*nq_d + m] = l'_m(xi_i), the derivative of the
 * m-th Lagrange polynomial of the quadrature points at point i, so (D_d u)[i] = sum_m deriv_d[i*nq_d + m] u[m].
 * w[e][k][j][i]: one mass weight per point, as in sf_mass_*.  g[e][c][k][j][i]: the symmetric metric tensor per point
 * (Jacobian determinant x quadrature weight x grad xi_a . grad xi_b) as component planes per element, each plane laid
 * out like w.  Component order: 3D c = 0..5 for (a,b) = (00, 01, 02, 11, 12, 22), 2D c = 0..2 for (00, 01, 11);
 * G_ba = G_ab is not stored.  g may be indefinite; the operator is symmetric for any g.
 * If lambda == 0, `w` may be NULL: it is then never read (nor validated), and the operator moves one plane less.
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs):
 *   1. forward sweeps p -> i, q -> j, r -> k, as BwdTrans:                  u
 *   2. du_a = D_a u for each direction a
 *   3. f_a = sum_b G_ab du_b, b ascending
 *   4. v = ((lambda w) u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]            (lambda == 0: the first term is 0)
 *   5. transposed sweeps k -> r', j -> q', i -> p', as sf_mass_*
 * lambda is a double in every entry point; the f32 entry points round it to float once, before the launch.
 * Routes: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq 2..8, 2D nq 2..16)
 * when in / out are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off that table and SF_EALIGN
 * unless in / out are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per element, latency-bound) takes any extents
 * up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 are NOT in the wave table and take it, as do all anisotropic
 * shapes; any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  g, w, the bases and the derivative
 * matrices need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, g, in or out, a null w with lambda != 0, or a lambda that
 * is not finite: SF_EINVAL; (4) any of them (w only if lambda != 0) not scalar-aligned: SF_EALIGN; (5) `out` overlapping
 * `in`, `g` or (if lambda != 0) `w`, compared as byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the
 * fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe, for the reason given under sf_mass_*; the inputs may overlap each other (all are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_helmholtz_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                         const double *basis0, const double *basis1, const double *basis2,
                         const double *deriv0, const double *deriv1, const double *deriv2,
                         const double *g, const double *w, double lambda,
                         const double *in, double *out, void *stream);
int sf_helmholtz_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                 const double *basis0, const double *basis1, const double *basis2,
                                 const double *deriv0, const double *deriv1, const double *deriv2,
                                 const double *g, const double *w, double lambda,
                                 const double *in, double *out, void *stream);
int sf_helmholtz_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0, const double *basis1,
                          const double *deriv0, const double *deriv1, const double *g, const double *w,
                          double lambda, const double *in, double *out, void *stream);
int sf_helmholtz_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                  const double *basis1, const double *deriv0, const double *deriv1,
                                  const double *g, const double *w, double lambda, const double *in,
                                  double *out, void *stream);
/* T = float (AUTO route; g / w / in / out / bases / derivative matrices 4-byte aligned; lambda stays a double) */
int sf_helmholtz_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                         const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                         const float *deriv2, const float *g, const float *w, double lambda, const float *in,
                         float *out, void *stream);
int sf_helmholtz_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                          const float *deriv0, const float *deriv1, const float *g, const float *w,
                          double lambda, const float *in, float *out, void *stream);

/*
 * The fused Helmholtz operator on AFFINE elements (parallelepipeds, parallelograms: a constant Jacobian J_e), where the
 * metric of sf_helmholtz_* factorises into constants of the element times quadrature weights that all elements share:
 *   G_ab,e[k][j][i] = ge[e][ab] * qw2[k] qw1[j] qw0[i]        w_e[k][j][i] = je[e] * qw2[k] qw1[j] qw0[i]
 *   y_e = B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B x_e
 * The same operator in one kernel, without the metric stream: per element the call moves 2 nm^d + d(d+1)/2 + 1 scalars
 * where sf_helmholtz_* moves 2 nm^d + (1 + d(d+1)/2) nq^d, and the caller stores d(d+1)/2 + 1 scalars per element
 * instead of (1 + d(d+1)/2) nq^d.
 * Layout: basis_d, deriv_d, `in` and `out` exactly as in sf_helmholtz_*.  qw_d: the nq_d one-dimensional quadrature
 * weights of direction d.  ge[e][c]: the constant symmetric tensor |det J_e| J_e^-1 J_e^-T of the element, d(d+1)/2
 * scalars per element, c in the order of the planes of g: 3D c = 0..5 for (a,b) = (00, 01, 02, 11, 12, 22), 2D c = 0..2
 * for (00, 01, 11).  ge may be indefinite; the operator is symmetric for any ge.  je[e]: |det J_e|, one scalar per
 * element.  If lambda == 0, `je` may be NULL: it is then never read (nor validated).
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike):
 *   1. forward sweeps p -> i, q -> j, r -> k, as BwdTrans:                  u
 *   2. du_a = D_a u for each direction a
 *   3. q = qw2[k] * (qw1[j] * qw0[i])  (2D: q = qw1[j] * qw0[i]);   f_a = q * (sum_b ge_ab du_b), b ascending
 *   4. v = (((lambda je_e) * q) * u + D_0^T f_0) + D_1^T f_1 [+ D_2^T f_2]  (lambda == 0: the first term is 0)
 *   5. transposed sweeps k -> r', j -> q', i -> p', as sf_mass_*
 * lambda is a double in every entry point; it is rounded to the scalar type once, before the launch, and lambda je_e
 * is formed in the scalar type.
 * Routes, as sf_helmholtz_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when in / out are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off that
 * table and SF_EALIGN unless in / out are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per element, latency-
 * bound) takes any extents up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 and all anisotropic shapes take it;
 * any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  ge, je, the quadrature weights, the bases
 * and the derivative matrices need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, qw, ge, in or out, a null je with lambda != 0, or a lambda
 * that is not finite: SF_EINVAL; (4) any of them (je only if lambda != 0) not scalar-aligned: SF_EALIGN;
 * (5) `out` overlapping `in`, `ge` or (if lambda != 0) `je`, compared as byte ranges of their full sizes: SF_EINVAL;
 * (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe, for the reason given under sf_mass_*; the inputs may overlap each other (all are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_affine_helmholtz_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                const double *basis0, const double *basis1, const double *basis2,
                                const double *deriv0, const double *deriv1, const double *deriv2,
                                const double *qw0, const double *qw1, const double *qw2,
                                const double *ge, const double *je, double lambda,
                                const double *in, double *out, void *stream);
int sf_affine_helmholtz_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                        const double *basis0, const double *basis1, const double *basis2,
                                        const double *deriv0, const double *deriv1, const double *deriv2,
                                        const double *qw0, const double *qw1, const double *qw2,
                                        const double *ge, const double *je, double lambda,
                                        const double *in, double *out, void *stream);
int sf_affine_helmholtz_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                 const double *basis1, const double *deriv0, const double *deriv1,
                                 const double *qw0, const double *qw1, const double *ge, const double *je,
                                 double lambda, const double *in, double *out, void *stream);
int sf_affine_helmholtz_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                                         const double *basis0, const double *basis1, const double *deriv0,
                                         const double *deriv1, const double *qw0, const double *qw1,
                                         const double *ge, const double *je, double lambda, const double *in,
                                         double *out, void *stream);
/* T = float (AUTO route; every array 4-byte aligned; lambda stays a double) */
int sf_affine_helmholtz_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                                const float *basis1, const float *basis2, const float *deriv0,
                                const float *deriv1, const float *deriv2, const float *qw0, const float *qw1,
                                const float *qw2, const float *ge, const float *je, double lambda,
                                const float *in, float *out, void *stream);
int sf_affine_helmholtz_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                                 const float *basis1, const float *deriv0, const float *deriv1,
                                 const float *qw0, const float *qw1, const float *ge, const float *je,
                                 double lambda, const float *in, float *out, void *stream);

/*
 * BwdTrans fused with the physical-space gradient (PhysDeriv), what an explicit advection or diffusion step, a pointwise
 * flux or an error norm needs at the quadrature points:
 *   u = B x_e,   du_b = D_b u,   out_a[e][k][j][i] = sum_b df[e][a*d + b][k][j][i] * du_b[e][k][j][i],   a = 0 .. d-1
 * BwdTrans, the d collocation derivatives and the d x d product with the inverse Jacobian in ONE kernel.  Per element
 * the call moves nm^d + (d*d + d) nq^d scalars (nm^d + d nq^d without df); no intermediate point image reaches HBM.
 * Layout: basis_d, deriv_d (deriv_d[i*nq_d + m] = l'_m(xi_i)) and `in` (nm0*nm1[*nm2] modes per element) exactly as in
 * sf_helmholtz_*.  df[e][c][k][j][i]: the inverse Jacobian per point as d*d component planes per element, component
 * order c = a*d + b for d xi_b / d x_a (row a: the physical direction of out_a; column b: the reference direction of
 * du_b), each plane laid out like the output of BwdTrans.  df is NOT symmetric: all d*d planes are stored, 9 in 3D and
 * 4 in 2D.  out_a: d separate caller-owned arrays of nq0*nq1[*nq2] points per element in the BwdTrans output layout
 * (i fastest); each can go straight into sf_iproduct_* or sf_mass_*.
 * If df is NULL it is never read (nor validated): the call returns the reference-space derivatives out_a = du_a, with
 * no multiplication by one, and moves d*d planes less.
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike):
 *   1. forward sweeps p -> i, q -> j, r -> k, as BwdTrans:                  u
 *   2. du_a = D_a u for each direction a
 *   3. out_a = sum_b df_ab du_b, b ascending                                (df NULL: out_a = du_a)
 * Routes, as sf_helmholtz_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when `in` and every out_a are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT
 * off that table and SF_EALIGN unless `in` and every out_a are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per
 * element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 and all
 * anisotropic shapes take it; any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  df, the bases
 * and the derivative matrices need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, in or out_a: SF_EINVAL (df may be null); (4) any of them
 * (df only if it is not null) not scalar-aligned: SF_EALIGN; (5) any out_a overlapping `in`, `df` or another out_b,
 * compared as byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an
 * unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe: an output that overlaps an input or another output is refused, not undefined; the inputs may overlap
 * each other (all are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_physderiv_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                         const double *basis0, const double *basis1, const double *basis2,
                         const double *deriv0, const double *deriv1, const double *deriv2,
                         const double *df, const double *in,
                         double *out0, double *out1, double *out2, void *stream);
int sf_physderiv_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                 const double *basis0, const double *basis1, const double *basis2,
                                 const double *deriv0, const double *deriv1, const double *deriv2,
                                 const double *df, const double *in,
                                 double *out0, double *out1, double *out2, void *stream);
int sf_physderiv_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0, const double *basis1,
                          const double *deriv0, const double *deriv1, const double *df, const double *in,
                          double *out0, double *out1, void *stream);
int sf_physderiv_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                  const double *basis1, const double *deriv0, const double *deriv1,
                                  const double *df, const double *in, double *out0, double *out1,
                                  void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_physderiv_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                         const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                         const float *deriv2, const float *df, const float *in, float *out0, float *out1,
                         float *out2, void *stream);
int sf_physderiv_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                          const float *deriv0, const float *deriv1, const float *df, const float *in,
                          float *out0, float *out1, void *stream);

/*
 * benchmark02: x[i] += y[i]  -- replaces add_vector<T,vl><<<>>>
 * (benchmark02/benchmark02.cc:16-58); 24 bytes of HBM traffic per element (:255), so its GB/s is the
 * measured stream rate used as the second roofline denominator.  fill: data1/data2 of :84-85.
 */
int sf_vector_add_f64(double *x, const double *y, size_t n, void *stream);
int sf_fill_vecadd_f64(double *x, double *y, size_t n, void *stream);

/*
 * benchmark03: y = A x, A row-major m x n -- replaces compute_matvec<T,vl><<<>>>
 * (benchmark03/benchmark03.cc:80-104).  fill: A[i*n+j] = sin(i*n+j+1), x[j] = j (:160-167).
 */
int sf_matvec_f64(unsigned m, unsigned n, const double *A, const double *x, double *y, void *stream);
int sf_fill_matvec_f64(double *A, double *x, unsigned m, unsigned n, void *stream);

/*
 * The reference drivers' `threads` / `elblocks` arguments (benchmark05/benchmark05.cc:1428-1429): block
 * size of the thread-per-element / flat-tid kernels and elements per workgroup (`blocks = nelmt/elblocks`,
 * :1188).  They shape only the reference-style decompositions (SF_VARIANT_THREAD / BLOCK_LDS / BLOCK_GLB);
 * the wave and matrix-core kernels choose their own launch shapes.  0 = automatic (default).  The hint belongs to the
 * CALLING host thread: it shapes that thread's later launches only.
 */
int sf_set_launch_hint(unsigned threads, unsigned elblocks);

/* Number of compute units / device name of the current device (for logs). */
int sf_device_info(int *num_cu, int *wave_size, char *name, size_t name_len);

/*
 * Run-time specialisation.  The flagship wave-per-chunk kernels are compiled ahead of time for a table of shapes (3D
 * isotropic, 33 anisotropic triples, 2D isotropic); sf_specialise() compiles the same kernel for any other extents
 * with hiprtc (loaded with dlopen on first use; never linked), once per process, and loads it once per device.
 * SF_VARIANT_AUTO of sf_bwdtrans_{hex,quad}_f64 and sf_bwdtrans_{hex,quad}_f32 then launches a READY specialisation
 * for a shape the compiled tables miss when in / out are 16-byte aligned (order: table, specialisation, the fallbacks
 * above).  AUTO never compiles on its own; the other variants are unaffected.  sf_shutdown() unloads every module.
 */

/* Compile (once per process) and load (once per device) the wave-per-chunk kernel specialised for these extents on
 * the current device.  dim 2 ignores nq2; scalar_bytes 8 (fp64) or 4 (fp32).  3D extents 2..16, 2D 2..24.
 * Not inside a stream capture.  Shapes already in a compiled table also specialise (for comparison); AUTO keeps
 * preferring the table for those.  SF_ECOMPILE: hiprtc missing, compile failed, the device is not gfx950 (xnack-),
 * one wave's LDS would exceed 64 KiB, or the kernel spills; the failure is remembered for the device. */
int sf_specialise(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes);

/* State on the current device: 0 none, 1 ready, SF_ECOMPILE failed; *launches (may be NULL) counts launches of it. */
int sf_specialisation_state(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, uint64_t *launches);

/* Launch only the specialised kernel: SF_ENOTBUILT if it is not ready, SF_EALIGN unless in/out are 16-byte aligned. */
int sf_bwdtrans_specialised(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, size_t nelmt,
                            const void *basis0, const void *basis1, const void *basis2, const void *in, void *out,
                            void *stream);

/* The calling thread's last sf_specialise() log: one line with the shape, device, target, the process's compile
 * number and its seconds, the instantiation, then the compiler's log (resource-usage remarks included).  "" before
 * the first call; valid until the thread's next sf_specialise(). */
const char *sf_last_specialise_log(void);

/* Free internal workspaces of the current device and unload every specialisation (optional; called at exit otherwise
 * never). */
int sf_shutdown(void);

/*
 * IProductWRTDerivBase, the weak divergence sum_a int d phi / d x_a f_a: what every explicit advection, diffusion or DG
 * volume term ends in, and the exact transpose of sf_physderiv_*.  With f_a = in_a[e][k][j][i], a = 0 .. d-1:
 *   g_b[e][k][j][i] = w[e][k][j][i] * sum_a df[e][a*d + b][k][j][i] * in_a[e][k][j][i]            (per point; b = 0 .. d-1)
 *   out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p]
 * The d x d product with the inverse Jacobian, the weight, the d transposed collocation derivatives and IProductWRTBase
 * in ONE kernel.  Per element the call moves (d*d + d + 1) nq^d + nm^d scalars (less d*d nq^d without df, less nq^d
 * without w); no intermediate point image reaches HBM.
 * Layout: basis_d and deriv_d exactly as in sf_physderiv_*.  in_a: d separate caller-owned arrays of nq0*nq1[*nq2]
 * points per element in the BwdTrans output layout (i fastest) -- exactly what sf_physderiv_* writes.  df: the d*d planes
 * of sf_physderiv_*, the same array in the same component order c = a*d + b for d xi_b / d x_a; the sum here runs over
 * the ROW index a (the transpose of the product in sf_physderiv_*).  w: one plane per element, laid out like the w of
 * sf_mass_* (Jacobian times quadrature weight).  out: nm0*nm1[*nm2] modes per element, the layout of sf_iproduct_*'s
 * output.
 * If df is NULL it is never read (nor validated): g_b = w * in_b.  If w is NULL it is never read (nor validated): no
 * multiplication happens.  With both NULL the call is sum_b B^T D_b^T in_b.  With w == NULL the call is bit for bit the
 * algebraic transpose of sf_physderiv_* on the same df.
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike):
 *   1. t_b = sum_a df_ab in_a, a ascending                                  (df NULL: t_b = in_b)
 *   2. g_b = w * t_b                                                        (w NULL: g_b = t_b)
 *   3. v = (D_0^T g_0 + D_1^T g_1) [+ D_2^T g_2]
 *   4. transposed sweeps k -> r, j -> q, i -> p, as sf_iproduct_* / sf_mass_*
 * Routes, as sf_physderiv_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when `out` is 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off that table and
 * SF_EALIGN unless `out` is 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per element, latency-bound) takes any
 * extents up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 and all anisotropic shapes take it; any other variant
 * SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  Only `out` needs 16-byte alignment for the wave route (it is
 * flushed as the 16-byte stream); every in_a, df, w, the bases and the derivative matrices are read one scalar per lane
 * and need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, in_a or out: SF_EINVAL (df and w may be null); (4) any of
 * them (df, w only if not null) not scalar-aligned: SF_EALIGN; (5) `out` overlapping any in_a, `df` or `w`, compared as
 * byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported
 * variant: SF_ENOTBUILT.
 * NOT in-place safe: an output that overlaps an input is refused, not undefined; the inputs may overlap each other (all
 * are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_iprodderiv_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                          const double *basis0, const double *basis1, const double *basis2,
                          const double *deriv0, const double *deriv1, const double *deriv2,
                          const double *df, const double *w,
                          const double *in0, const double *in1, const double *in2, double *out, void *stream);
int sf_iprodderiv_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                  const double *basis0, const double *basis1, const double *basis2,
                                  const double *deriv0, const double *deriv1, const double *deriv2,
                                  const double *df, const double *w,
                                  const double *in0, const double *in1, const double *in2, double *out, void *stream);
int sf_iprodderiv_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0, const double *basis1,
                           const double *deriv0, const double *deriv1, const double *df, const double *w,
                           const double *in0, const double *in1, double *out, void *stream);
int sf_iprodderiv_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                   const double *basis1, const double *deriv0, const double *deriv1,
                                   const double *df, const double *w, const double *in0, const double *in1,
                                   double *out, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_iprodderiv_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                          const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                          const float *deriv2, const float *df, const float *w, const float *in0,
                          const float *in1, const float *in2, float *out, void *stream);
int sf_iprodderiv_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                           const float *deriv0, const float *deriv1, const float *df, const float *w,
                           const float *in0, const float *in1, float *out, void *stream);

/*
 * sf_physderiv_* on AFFINE elements (parallelepipeds, parallelograms: a constant Jacobian per element): sf_aff_physderiv_*
 * (the prefix sf_affine_ names the Helmholtz family of sf_affine_helmholtz_* alone; these two families take sf_aff_).
 *   u = B x_e,   du_b = D_b u,   out_a[e][k][j][i] = sum_b dfe[e][a*d + b] * du_b[e][k][j][i],   a = 0 .. d-1
 * The inverse Jacobian is d*d constants per element where sf_physderiv_* streams d*d planes: per element the call moves
 * nm^d + d nq^d + d*d scalars, and the caller stores d*d scalars per element where it stored d*d nq^d.
 * Layout: basis_d, deriv_d, `in` and out_a exactly as in sf_physderiv_*.  dfe[e][c]: d*d scalars per element, component
 * order c = a*d + b for d xi_b / d x_a -- the order of the planes of df; NOT symmetric.  dfe is required: the
 * reference-space derivatives are sf_physderiv_* with df == NULL.
 * Summation order: steps 1-3 of sf_physderiv_* with df_ab replaced by the element's constant (b ascending, the first
 * product a multiply, then FMAs).  On a route the result is therefore BIT FOR BIT that of sf_physderiv_* on the same
 * route with planes filled with the constants, in fp64 and in fp32.
 * Routes, as sf_physderiv_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when `in` and every out_a are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT
 * off that table and SF_EALIGN unless `in` and every out_a are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per
 * element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 and all
 * anisotropic shapes take it; any other variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  dfe, the bases
 * and the derivative matrices need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, dfe, in or out_a: SF_EINVAL; (4) any of them not
 * scalar-aligned: SF_EALIGN; (5) any out_a overlapping `in`, `dfe` or another out_b, compared as byte ranges of their
 * full sizes: SF_EINVAL; (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant:
 * SF_ENOTBUILT.
 * NOT in-place safe: an output that overlaps an input or another output is refused, not undefined; the inputs may overlap
 * each other (all are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_aff_physderiv_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                const double *basis0, const double *basis1, const double *basis2,
                                const double *deriv0, const double *deriv1, const double *deriv2,
                                const double *dfe, const double *in,
                                double *out0, double *out1, double *out2, void *stream);
int sf_aff_physderiv_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                        const double *basis0, const double *basis1, const double *basis2,
                                        const double *deriv0, const double *deriv1, const double *deriv2,
                                        const double *dfe, const double *in,
                                        double *out0, double *out1, double *out2, void *stream);
int sf_aff_physderiv_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                 const double *basis1, const double *deriv0, const double *deriv1,
                                 const double *dfe, const double *in, double *out0, double *out1, void *stream);
int sf_aff_physderiv_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                                         const double *basis0, const double *basis1, const double *deriv0,
                                         const double *deriv1, const double *dfe, const double *in,
                                         double *out0, double *out1, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_aff_physderiv_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                                const float *basis1, const float *basis2, const float *deriv0,
                                const float *deriv1, const float *deriv2, const float *dfe, const float *in,
                                float *out0, float *out1, float *out2, void *stream);
int sf_aff_physderiv_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                                 const float *basis1, const float *deriv0, const float *deriv1,
                                 const float *dfe, const float *in, float *out0, float *out1, void *stream);

/*
 * sf_iprodderiv_* on AFFINE elements, the weak divergence with a constant Jacobian per element and the exact transpose
 * of sf_aff_physderiv_*.  With f_a = in_a[e][k][j][i], a = 0 .. d-1:
 *   t_b = sum_a dfe[e][a*d + b] * f_a                                   (per point; b = 0 .. d-1, a ascending)
 *   q   = qw2[k] * (qw1[j] * qw0[i])                                    (2D: qw1[j] * qw0[i])
 *   g_b = (je[e] * q) * t_b
 *   out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p]
 * Per element the call moves d nq^d + nm^d + d*d + 1 scalars where sf_iprodderiv_* moves (d*d + d + 1) nq^d + nm^d.
 * Layout: basis_d, deriv_d, in_a and out exactly as in sf_iprodderiv_*.  qw_d: the nq_d one-dimensional quadrature
 * weights of direction d, as in sf_affine_helmholtz_*.  dfe[e][c]: the d*d constants of sf_aff_physderiv_*, the
 * same array in the same order c = a*d + b; the sum here runs over the ROW index a.  je[e]: one scalar per element
 * (|det J_e|), as in sf_affine_helmholtz_*.  dfe is required.
 * If je is NULL no weight is applied at all: je and every qw_d are then never read (nor validated), and the call is bit
 * for bit the algebraic transpose of sf_aff_physderiv_* on the same dfe.  With je given, the result is BIT FOR BIT
 * that of sf_iprodderiv_* on the same route with df planes filled with the constants and the weight plane expanded in
 * the working precision with exactly the association above, w = je * (qw2 * (qw1 * qw0)).
 * Summation order: steps 1-4 of sf_iprodderiv_* with df_ab replaced by the element's constant and w by (je_e q).
 * Routes, as sf_iprodderiv_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when `out` is 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off that table and
 * SF_EALIGN unless `out` is 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per element, latency-bound) takes any
 * extents up to 12 per direction in 3D and 32 in 2D -- 3D nq 9..11 and all anisotropic shapes take it; any other variant
 * SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  Only `out` needs 16-byte alignment for the wave route; every
 * in_a, dfe, je, qw_d, the bases and the derivative matrices need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, dfe, in_a or out, or -- only when je is not null -- a null
 * qw_d: SF_EINVAL; (4) any of them (je, qw_d only when je is not null) not scalar-aligned: SF_EALIGN; (5) `out`
 * overlapping any in_a, `dfe` or `je`, compared as byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the
 * fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe: an output that overlaps an input is refused, not undefined; the inputs may overlap each other (all
 * are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_aff_iprodderiv_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                 const double *basis0, const double *basis1, const double *basis2,
                                 const double *deriv0, const double *deriv1, const double *deriv2,
                                 const double *qw0, const double *qw1, const double *qw2,
                                 const double *dfe, const double *je,
                                 const double *in0, const double *in1, const double *in2, double *out, void *stream);
int sf_aff_iprodderiv_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                         const double *basis0, const double *basis1, const double *basis2,
                                         const double *deriv0, const double *deriv1, const double *deriv2,
                                         const double *qw0, const double *qw1, const double *qw2,
                                         const double *dfe, const double *je,
                                         const double *in0, const double *in1, const double *in2, double *out,
                                         void *stream);
int sf_aff_iprodderiv_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                  const double *basis1, const double *deriv0, const double *deriv1,
                                  const double *qw0, const double *qw1, const double *dfe, const double *je,
                                  const double *in0, const double *in1, double *out, void *stream);
int sf_aff_iprodderiv_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt,
                                          const double *basis0, const double *basis1, const double *deriv0,
                                          const double *deriv1, const double *qw0, const double *qw1,
                                          const double *dfe, const double *je, const double *in0,
                                          const double *in1, double *out, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_aff_iprodderiv_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                                 const float *basis1, const float *basis2, const float *deriv0,
                                 const float *deriv1, const float *deriv2, const float *qw0, const float *qw1,
                                 const float *qw2, const float *dfe, const float *je, const float *in0,
                                 const float *in1, const float *in2, float *out, void *stream);
int sf_aff_iprodderiv_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0,
                                  const float *basis1, const float *deriv0, const float *deriv1,
                                  const float *qw0, const float *qw1, const float *dfe, const float *je,
                                  const float *in0, const float *in1, float *out, void *stream);

/*
 * The DIAGONAL of the fused Helmholtz operator of sf_helmholtz_*, per element:
 *   diag_e = diag( B^T [ lambda diag(w_e) + sum_a sum_b D_a^T diag(G_ab,e) D_b ] B )
 * what a Jacobi preconditioner, a Chebyshev smoother or a diagonal scaling of a matrix-free Poisson / Helmholtz /
 * implicit-diffusion solve needs next to the operator itself, in ONE kernel: per element the call reads the
 * (1 + d(d+1)/2) nq^d metric scalars of sf_helmholtz_* (one plane fewer with lambda == 0) and writes nm^d modes; applying
 * the operator to nm^d unit vectors costs nm^d launches and nm^d times that traffic.  Two calls:
 *
 * sf_diag_tables_*: the tables of ONE direction, once per order (they depend on the basis and the derivative matrix only).
 *   With E[p][i] = sum_m deriv[i*nq + m] * basis[p*nq + m], the derivative of mode p at point i, the call writes
 *   tab[t][p][i], t = 0, 1, 2:  T^0 = B o B,  T^1 = E o B,  T^2 = E o E  (elementwise products), each row-major nm x nq
 *   like a basis: 3 nm nq scalars, caller-owned.  Rounding: E is an ascending sum over m, the first product a multiply,
 *   then FMAs; every table entry is a single product.  One small kernel, no allocation, capture-safe.  Validation, before
 *   any HIP call: nq < 2 or nq > 1024: SF_EINVAL; a null pointer: SF_EINVAL; a pointer not scalar-aligned: SF_EALIGN;
 *   `tab` overlapping `basis` or `deriv` as byte ranges: SF_EINVAL.
 *
 * sf_diag_helmholtz_*: with tab_d the table triple of direction d,
 *   3D: out[e][r][q][p] = sum_kji lambda w[e][k][j][i] T0^0[p][i] T1^0[q][j] T2^0[r][k]
 *                       + sum_c f_c sum_kji g[e][c][k][j][i] T0^{s0}[p][i] T1^{s1}[q][j] T2^{s2}[r][k]
 *   2D: the same without k and r.  For the plane c = (a, b) of g: s_d = [d == a] + [d == b] is the table of direction d,
 *   f_c = 1 if a == b, else 2 (the symmetric pair is stored once).  Seven terms in 3D, four in 2D.
 * Layout: g and w exactly as in sf_helmholtz_* (g[e][c][k][j][i], component order 3D (00, 01, 02, 11, 12, 22), 2D (00,
 * 01, 11); w[e][k][j][i]); g may be indefinite.  out: nm0*nm1[*nm2] modes per element, p fastest, the layout of the
 * output of sf_iproduct_*.  If lambda == 0, `w` may be NULL: it is then never read (nor validated), and the call moves one
 * plane less.  lambda is a double in every entry point, rounded to the scalar type once, before the launch.
 * Why tables in memory: the kernels take their one-dimensional operands as wave-uniform scalar-register rows straight
 * from global memory; forming B o B or E o B inside a sweep would cost a vector multiply per FMA.
 * Order of operations (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs;
 * each image below is a sum of its own, merges are additions; the wave kernels and the fallback follow it alike):
 *   3D, the planes in the order of g, c = 0 .. 5, contraction order k -> r, j -> q, i -> p:
 *   1. k -> r: A_c[r][j][i] = sum_k g_c[k][j][i] T2^{s2}[r][k]; A_1, A_2, A_4 (the off-diagonal planes) are doubled, which
 *      is exact; if lambda != 0: A_5 = A_5 + sum_k (lambda w[k][j][i]) T2^0[r][k]      -- six images, one merge
 *   2. j -> q: S_c[r][q][i] = sum_j A_c[r][j][i] T1^{s1}[q][j], merged by the direction-0 table in the order of the planes:
 *      B^2 = S_0,  B^1 = S_1 + S_2,  B^0 = (S_3 + S_4) + S_5                           -- three images, three merges
 *   3. i -> p: out[r][q][p] = (sum_i B^0 T0^0[p][i] + sum_i B^1 T0^1[p][i]) + sum_i B^2 T0^2[p][i]       -- two merges
 *   2D, contraction order j -> q, i -> p:
 *   1. j -> q: B^0[q][i] = sum_j g_2 T1^2[q][j] (if lambda != 0: + sum_j (lambda w) T1^0[q][j]),
 *      B^1 = 2 sum_j g_1 T1^1[q][j],  B^2 = sum_j g_0 T1^0[q][j]
 *   2. i -> p: as step 3 above.
 * Routes, through the same dispatch as the other operators: SF_VARIANT_AUTO runs the wave kernel for the isotropic orders
 * of its table (3D nq 2..8, 2D nq 2..16: the table of sf_helmholtz_*, no row left out) when `out` is 16-byte aligned, else
 * GENERIC; SF_VARIANT_WAVE returns SF_ENOTBUILT off that table and SF_EALIGN unless `out` is 16-byte aligned;
 * SF_VARIANT_GENERIC (one workgroup per element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D
 * -- 3D nq 9..12, all anisotropic shapes and an `out` that is only scalar-aligned take it; any other variant SF_ENOTBUILT,
 * extents beyond those bounds SF_ENOTBUILT.  g, w and the tables are read one scalar per lane or as scalar operands and
 * need only scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null table, g or out, a null w with lambda != 0, or a lambda that is not finite:
 * SF_EINVAL; (4) any of them (w only if lambda != 0) not scalar-aligned: SF_EALIGN; (5) `out` overlapping `g`, (if
 * lambda != 0) `w`, or any of the tables, compared as byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the
 * fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.  The inputs may overlap each other (all are
 * only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call, thread-safe as the rest.
 */
int sf_diag_tables_f64(unsigned nq, const double *basis, const double *deriv, double *tab, void *stream);
int sf_diag_tables_f32(unsigned nq, const float *basis, const float *deriv, float *tab, void *stream);
int sf_diag_helmholtz_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                              const double *tab0, const double *tab1, const double *tab2,
                              const double *g, const double *w, double lambda, double *out, void *stream);
int sf_diag_helmholtz_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                      const double *tab0, const double *tab1, const double *tab2,
                                      const double *g, const double *w, double lambda, double *out, void *stream);
int sf_diag_helmholtz_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *tab0, const double *tab1,
                               const double *g, const double *w, double lambda, double *out, void *stream);
int sf_diag_helmholtz_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *tab0,
                                       const double *tab1, const double *g, const double *w, double lambda,
                                       double *out, void *stream);
/* T = float (AUTO route; every array 4-byte aligned; lambda stays a double) */
int sf_diag_helmholtz_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *tab0,
                              const float *tab1, const float *tab2, const float *g, const float *w, double lambda,
                              float *out, void *stream);
int sf_diag_helmholtz_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *tab0, const float *tab1,
                               const float *g, const float *w, double lambda, float *out, void *stream);

/*
 * GEOMETRIC FACTORS from the coordinates of every element: what sf_helmholtz_* / sf_diag_helmholtz_* (g, w),
 * sf_physderiv_* / sf_iprodderiv_* (df, w) and their affine forms (ge, je, dfe) take, computed from the mesh in ONE
 * kernel.  The element is isoparametric: coordinate a of element e is the field x_a[e] of nm0*nm1[*nm2] modal
 * coefficients in the layout of `in` of every other call (p fastest, nm_d = nq_d - 1), expanded in the same bases.
 *   X_a = B x_a,   J[a][b] = D_b X_a = d x_a / d xi_b   at every quadrature point,   a, b = 0 .. d-1
 *   df[e][c][k][j][i],   c = a*d + b for d xi_b / d x_a: the inverse of J, d*d planes -- the df of sf_physderiv_*
 *   detj[e][k][j][i] = det J, with its sign: a negative value marks an inverted element (w hides the sign)
 *   w[e][k][j][i] = |det J| * q,   q = qw2[k] * (qw1[j] * qw0[i])   (2D: qw1[j] * qw0[i]) -- the w of sf_helmholtz_*
 *   g[e][c][k][j][i],   c = 00, 01, 02, 11, 12, 22 (2D: 00, 01, 11):   G_ab = w * sum_x df[x*d + a] * df[x*d + b]
 *                                                                       -- the g of sf_helmholtz_*
 * Per element the call moves d nm^d + (d*d + d(d+1)/2 + 2) nq^d scalars when every output is asked for; no intermediate
 * point image reaches HBM.
 * Layout: basis_d and deriv_d exactly as in sf_helmholtz_*; qw_d the nq_d one-dimensional quadrature weights of
 * direction d, as in sf_affine_helmholtz_*; x_a: d separate caller-owned arrays.  Every output plane is laid out like
 * the output of BwdTrans (i fastest) and goes into its consumer with no copy.
 * Any output may be NULL: it is then neither written nor validated, and its arithmetic may be left out.  All four
 * NULL: SF_EINVAL.  qw_d may be NULL when w and g are both NULL (they are then never read, nor validated).
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike):
 *   1. forward sweeps p -> i, q -> j, r -> k of x_a, as BwdTrans:           X_a
 *   2. J[a][b] = D_b X_a
 *   3. 3D: cof[a][b] = fma(J[a+1][b+1], J[a+2][b+2], -(J[a+1][b+2] * J[a+2][b+1])), indices mod 3
 *      2D: cof = (J11, -J10, -J01, J00) in the order of c
 *   4. det = J[0][0] * cof[0][0], then det = fma(J[0][b], cof[0][b], det) for b = 1 [, 2]
 *   5. r = 1 / det (a correctly rounded division),   df[a*d + b] = cof[a][b] * r
 *   6. q as above,   w = |det| * q
 *   7. G_ab = w * (sum_x df[x*d + a] * df[x*d + b]), x ascending
 * A point with det == 0 gives inf / NaN at that point only: nothing is refused on the device, no neighbour is touched.
 * Routes, as sf_physderiv_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when every x_a and every output that is not NULL are 16-byte aligned, else GENERIC;
 * SF_VARIANT_WAVE returns SF_ENOTBUILT off that table and SF_EALIGN unless they are 16-byte aligned; SF_VARIANT_GENERIC
 * (one workgroup per element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D; any other
 * variant SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  The bases, the derivative matrices and qw_d need only
 * scalar alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv or x_a, all four outputs null, or a null qw_d while w or g
 * is asked for: SF_EINVAL; (4) any of them (an output, qw_d: only if it is looked at) not scalar-aligned: SF_EALIGN;
 * (5) any output overlapping any x_a or another output, compared as byte ranges of their full sizes: SF_EINVAL;
 * (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe: an output that overlaps a coordinate array or another output is refused, not undefined; the inputs
 * may overlap each other (all are only read).
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_geom_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                    const double *basis0, const double *basis1, const double *basis2,
                    const double *deriv0, const double *deriv1, const double *deriv2,
                    const double *qw0, const double *qw1, const double *qw2,
                    const double *x0, const double *x1, const double *x2,
                    double *df, double *w, double *g, double *detj, void *stream);
int sf_geom_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                            const double *basis0, const double *basis1, const double *basis2,
                            const double *deriv0, const double *deriv1, const double *deriv2,
                            const double *qw0, const double *qw1, const double *qw2,
                            const double *x0, const double *x1, const double *x2,
                            double *df, double *w, double *g, double *detj, void *stream);
int sf_geom_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0, const double *basis1,
                     const double *deriv0, const double *deriv1, const double *qw0, const double *qw1,
                     const double *x0, const double *x1, double *df, double *w, double *g, double *detj,
                     void *stream);
int sf_geom_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                             const double *basis1, const double *deriv0, const double *deriv1, const double *qw0,
                             const double *qw1, const double *x0, const double *x1, double *df, double *w,
                             double *g, double *detj, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_geom_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                    const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                    const float *deriv2, const float *qw0, const float *qw1, const float *qw2, const float *x0,
                    const float *x1, const float *x2, float *df, float *w, float *g, float *detj, void *stream);
int sf_geom_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                     const float *deriv0, const float *deriv1, const float *qw0, const float *qw1,
                     const float *x0, const float *x1, float *df, float *w, float *g, float *detj, void *stream);

/*
 * sf_geom_* for elements the caller knows to be AFFINE (a constant Jacobian): the same formulas at the point
 * (k, j, i) = (0, 0, 0) only, written as the per-element constants that sf_affine_helmholtz_* and sf_aff_physderiv_* /
 * sf_aff_iprodderiv_* take:
 *   dfe[e][c] = df of that point, c = a*d + b;   je[e] = |det J|;   ge[e][c] = je * sum_x dfe[x*d + a] * dfe[x*d + b],
 *   c = 00, 01, 02, 11, 12, 22 (2D: 00, 01, 11)
 * No quadrature weights enter: the affine operators multiply by q themselves.  Steps 1-5 and 7 of sf_geom_* in the same
 * order, so dfe[e][c] and je[e] equal df[e][c][0][0][0] and |detj[e][0][0][0]| of sf_geom_* on the same coordinates BIT
 * FOR BIT.  Whether the element is affine is not checked.
 * Any output may be NULL (neither written nor validated); all three NULL: SF_EINVAL.  One plain small kernel without
 * variants, for any extents the GENERIC route of sf_geom_* takes (beyond: SF_ENOTBUILT); every array needs only scalar
 * alignment.  Validation in the order of sf_geom_* without the variant; an output overlapping any x_a or another output:
 * SF_EINVAL.  No internal workspace and no allocation: a single kernel node, capture-safe from the first call.
 */
int sf_geom_affine_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                           const double *basis0, const double *basis1, const double *basis2,
                           const double *deriv0, const double *deriv1, const double *deriv2,
                           const double *x0, const double *x1, const double *x2,
                           double *dfe, double *ge, double *je, void *stream);
int sf_geom_affine_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                            const double *basis1, const double *deriv0, const double *deriv1, const double *x0,
                            const double *x1, double *dfe, double *ge, double *je, void *stream);
int sf_geom_affine_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                           const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                           const float *deriv2, const float *x0, const float *x1, const float *x2, float *dfe,
                           float *ge, float *je, void *stream);
int sf_geom_affine_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                            const float *deriv0, const float *deriv1, const float *x0, const float *x1,
                            float *dfe, float *ge, float *je, void *stream);

/*
 * THE WEAK ADVECTION TERM (c . grad) u tested against the basis, for nf = 1 or d fields, in ONE kernel: the first-order
 * term of an advection-diffusion or Navier-Stokes step and of an Oseen operator.  For every element e and field a:
 *   u_a      = B in_a[e]                              forward sweeps p -> i, q -> j, r -> k, as BwdTrans
 *   J[a][b]  = D_b u_a                                collocation derivative, b = 0 .. d-1
 *   beta_b   = sum_j c_j[e] * df[e][j*d + b]          per point; j ascending
 *   r_a      = w[e] * (sum_b beta_b * J[a][b])        per point; b ascending, then one multiply by w
 *   out_a[e] = B^T r_a                                transposed sweeps k -> r', j -> q', i -> p', as IProductWRTBase
 * df: the d*d planes of the inverse Jacobian in the layout of sf_physderiv_* / sf_geom_* (c = a*d + b for
 * d xi_b / d x_a); w: the weight plane of sf_mass_* / sf_geom_*; c_j: d planes of the advecting velocity at the
 * quadrature points, each laid out like the output of BwdTrans (from sf_bwdtrans_* of a modal velocity, or from anywhere
 * else); in_a / out_a: nm0*nm1[*nm2] modes per element, nm_d = nq_d - 1, the layout of `in` of every other call.
 * nf = 1 is scalar transport: in1.. / out1.. are ignored, may be NULL and are never written.  nf = d advects a vector
 * field: all d fields share one read of df, w and c.  Any other nf: SF_EINVAL.  All of df, w, c_j are required.
 * Per element the call moves (d*d + d + 1) nq^d + 2 nf nm^d scalars; no point image reaches HBM.
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike, bit for bit): the five lines above, in that order.  beta is formed
 * first on purpose: d*d FMAs per point shared by the fields.  out_a of a call with nf = 1 and in = in_a equals out_a of
 * the call with nf = d bit for bit.
 * Routes, as sf_physderiv_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq
 * 2..8, 2D nq 2..16) when every in_a and out_a (a < nf) are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns
 * SF_ENOTBUILT off that table and SF_EALIGN unless they are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per
 * element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D; any other variant SF_ENOTBUILT,
 * extents beyond those bounds SF_ENOTBUILT.  df, w, c_j, the bases and the derivative matrices need only scalar
 * alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2, a variant outside [0, SF_NUM_VARIANTS) or nf other
 * than 1 or d: SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, df, w, c_j, or in_a / out_a with a < nf:
 * SF_EINVAL; (4) any of them not scalar-aligned: SF_EALIGN; (5) any out_a overlapping anything the call reads or another
 * out_a, compared as byte ranges of their full sizes: SF_EINVAL; (6) extents beyond the fallback's bounds: SF_ENOTBUILT;
 * (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe: an overlapping output is refused, not undefined; the inputs may overlap each other.
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_advect_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf,
                      const double *basis0, const double *basis1, const double *basis2,
                      const double *deriv0, const double *deriv1, const double *deriv2,
                      const double *df, const double *w, const double *c0, const double *c1, const double *c2,
                      const double *in0, const double *in1, const double *in2,
                      double *out0, double *out1, double *out2, void *stream);
int sf_advect_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf,
                              const double *basis0, const double *basis1, const double *basis2,
                              const double *deriv0, const double *deriv1, const double *deriv2,
                              const double *df, const double *w, const double *c0, const double *c1, const double *c2,
                              const double *in0, const double *in1, const double *in2,
                              double *out0, double *out1, double *out2, void *stream);
int sf_advect_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf, const double *basis0,
                       const double *basis1, const double *deriv0, const double *deriv1, const double *df,
                       const double *w, const double *c0, const double *c1, const double *in0, const double *in1,
                       double *out0, double *out1, void *stream);
int sf_advect_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf,
                               const double *basis0, const double *basis1, const double *deriv0, const double *deriv1,
                               const double *df, const double *w, const double *c0, const double *c1,
                               const double *in0, const double *in1, double *out0, double *out1, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_advect_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf, const float *basis0,
                      const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                      const float *deriv2, const float *df, const float *w, const float *c0, const float *c1,
                      const float *c2, const float *in0, const float *in1, const float *in2, float *out0,
                      float *out1, float *out2, void *stream);
int sf_advect_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf, const float *basis0, const float *basis1,
                       const float *deriv0, const float *deriv1, const float *df, const float *w, const float *c0,
                       const float *c1, const float *in0, const float *in1, float *out0, float *out1, void *stream);

/*
 * sf_advect_* on AFFINE elements: the weak advection term with a constant Jacobian per element.  For every element e
 * and field a < nf, nf = 1 or d:
 *   u_a      = B in_a[e]                                forward sweeps, as sf_advect_*
 *   J[a][b]  = D_b u_a
 *   beta_b   = sum_j c_j[e][pt] * dfe[e][j*d + b]       per point; j ascending; first product a multiply, then FMAs
 *   q        = qw2[k] * (qw1[j] * qw0[i])               (2D: qw1[j] * qw0[i])
 *   r_a      = (je[e] * q) * (sum_b beta_b * J[a][b])   b ascending, then one multiply by the weight
 *   out_a[e] = B^T r_a                                  transposed sweeps, as sf_advect_*
 * Per element the call moves d nq^d + 2 nf nm^d + d*d + 1 scalars where sf_advect_* moves (d*d + d + 1) nq^d + 2 nf nm^d.
 * Layout: basis_d, deriv_d, c_j, in_a and out_a exactly as in sf_advect_*.  dfe[e][c]: the d*d constants of
 * sf_aff_physderiv_* / sf_geom_affine_*, the same array in the same order c = a*d + b (not symmetric); required.
 * qw_d: the nq_d one-dimensional quadrature weights of direction d and je[e]: one scalar per element (|det J_e|), both as
 * in sf_aff_iprodderiv_*.  c_j: the d planes of the advecting velocity at the points; required.
 * If je is NULL no weight is applied at all, r_a = sum_b beta_b J[a][b]: je and every qw_d are then never read (nor
 * validated).  nf = 1 is scalar transport: in1.. / out1.. are ignored, may be NULL and are never written.  nf = d shares
 * one read of c, dfe and je over the fields.  Any other nf: SF_EINVAL.
 * Bit contract.  The order of operations is that of sf_advect_* with df_ab replaced by the element's constant and w by
 * je * (qw2 * (qw1 * qw0)) formed in the working precision in exactly that association.  On a route the result is
 * therefore BIT FOR BIT that of sf_advect_* on the same route with df planes filled with the constants and w expanded
 * that way; with je NULL, that of sf_advect_* with w a plane of ones.  This holds in fp64 and fp32.  out_a of a call with
 * nf = 1 and in = in_a equals out_a of the call with nf = d bit for bit.
 * Routes, as sf_advect_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq 2..8,
 * 2D nq 2..16) when every in_a and out_a (a < nf) are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE returns
 * SF_ENOTBUILT off that table and SF_EALIGN unless they are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup per
 * element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D; any other variant SF_ENOTBUILT,
 * extents beyond those bounds SF_ENOTBUILT.  dfe, je, qw_d, c_j, the bases and the derivative matrices need only scalar
 * alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2, a variant outside [0, SF_NUM_VARIANTS) or nf other
 * than 1 or d: SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, dfe, c_j, or in_a / out_a with a < nf, or --
 * only when je is not null -- a null qw_d: SF_EINVAL; (4) any of them (je, qw_d only when je is not null) not
 * scalar-aligned: SF_EALIGN; (5) any out_a overlapping anything the call reads or another out_a, compared as byte ranges
 * of their full sizes: SF_EINVAL; (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant:
 * SF_ENOTBUILT.
 * NOT in-place safe: an overlapping output is refused, not undefined; the inputs may overlap each other.
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_aff_advect_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf, const double *basis0,
                          const double *basis1, const double *basis2, const double *deriv0, const double *deriv1,
                          const double *deriv2, const double *qw0, const double *qw1, const double *qw2,
                          const double *dfe, const double *je, const double *c0, const double *c1, const double *c2,
                          const double *in0, const double *in1, const double *in2, double *out0, double *out1,
                          double *out2, void *stream);
int sf_aff_advect_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf,
                                  const double *basis0, const double *basis1, const double *basis2,
                                  const double *deriv0, const double *deriv1, const double *deriv2, const double *qw0,
                                  const double *qw1, const double *qw2, const double *dfe, const double *je,
                                  const double *c0, const double *c1, const double *c2, const double *in0,
                                  const double *in1, const double *in2, double *out0, double *out1, double *out2,
                                  void *stream);
int sf_aff_advect_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf, const double *basis0,
                           const double *basis1, const double *deriv0, const double *deriv1, const double *qw0,
                           const double *qw1, const double *dfe, const double *je, const double *c0, const double *c1,
                           const double *in0, const double *in1, double *out0, double *out1, void *stream);
int sf_aff_advect_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf,
                                   const double *basis0, const double *basis1, const double *deriv0,
                                   const double *deriv1, const double *qw0, const double *qw1, const double *dfe,
                                   const double *je, const double *c0, const double *c1, const double *in0,
                                   const double *in1, double *out0, double *out1, void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_aff_advect_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, unsigned nf, const float *basis0,
                          const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                          const float *deriv2, const float *qw0, const float *qw1, const float *qw2, const float *dfe,
                          const float *je, const float *c0, const float *c1, const float *c2, const float *in0,
                          const float *in1, const float *in2, float *out0, float *out1, float *out2, void *stream);
int sf_aff_advect_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, unsigned nf, const float *basis0,
                           const float *basis1, const float *deriv0, const float *deriv1, const float *qw0,
                           const float *qw1, const float *dfe, const float *je, const float *c0, const float *c1,
                           const float *in0, const float *in1, float *out0, float *out1, void *stream);

/*
 * GRADIENT, DIVERGENCE AND CURL OF A VECTOR FIELD at the quadrature points, in ONE kernel: the velocity-gradient tensor
 * behind a strain rate, an eddy viscosity or a Q-criterion, the divergence residual and the vorticity of an
 * incompressible-flow step.  For every element e and field a = 0 .. d-1:
 *   u_a        = B in_a[e]                              forward sweeps p -> i, q -> j, r -> k, as BwdTrans
 *   J[a][b]    = D_b u_a                                collocation derivative, b = 0 .. d-1
 *   grad[a][j] = sum_b df[e][j*d + b] * J[a][b]         per point; b ascending; this is d u_a / d x_j, step 3 of
 *                                                       sf_physderiv_* applied to field a
 *   div        = (grad[0][0] + grad[1][1]) [+ grad[2][2]]      plain additions of the rounded entries
 *   3D: curl0 = grad[2][1] - grad[1][2],   curl1 = grad[0][2] - grad[2][0],   curl2 = grad[1][0] - grad[0][1]
 *   2D: curl0 = grad[1][0] - grad[0][1]                        plain subtractions of the rounded entries
 * Layout: basis_d, deriv_d, in_a (d separate caller-owned arrays of nm0*nm1[*nm2] modes per element) and df (required;
 * the d*d planes, c = a*d + b for d xi_b / d x_a) exactly as in sf_advect_* / sf_physderiv_*.  grad[e][c][k][j][i]: d*d
 * planes per element in the layout of df, c = a*d + j.  div, curl0 and -- in 3D -- curl1, curl2: separate caller-owned
 * arrays of one plane per element in the layout of the output of BwdTrans, so that each goes straight into
 * sf_iproduct_*, sf_mass_* or, as c_j, into sf_advect_*.
 * Any of grad, div and the curl may be NULL: it is then neither written nor validated.  All NULL: SF_EINVAL.  In 3D
 * curl0, curl1, curl2 are all NULL or all not NULL; anything else: SF_EINVAL.
 * Per element the call moves d nm^d + d*d nq^d + n_out nq^d scalars, n_out the number of planes asked for (at most
 * d*d + 1 + d(d-1)/2); no intermediate point image reaches HBM.  d calls of sf_physderiv_* read df d times.
 * Summation order (it defines the rounding; every sum in ascending index, the first product a multiply, then FMAs; the
 * wave kernels and the fallback follow it alike): the lines above, in that order.  Plane a*d + j of grad therefore
 * equals output j of sf_physderiv_* on in_a on the same route BIT FOR BIT, div and curl equal the sums and differences
 * of those planes formed in the order written above, and in float64 the wave kernels and the fallback agree bit for
 * bit.  The reference-space form (no df) is not offered.
 * Routes, as sf_geom_*: SF_VARIANT_AUTO runs the fused wave kernel for the isotropic orders of its table (3D nq 2..8,
 * 2D nq 2..16) when every in_a and every output that is not NULL are 16-byte aligned, else GENERIC; SF_VARIANT_WAVE
 * returns SF_ENOTBUILT off that table and SF_EALIGN unless they are 16-byte aligned; SF_VARIANT_GENERIC (one workgroup
 * per element, latency-bound) takes any extents up to 12 per direction in 3D and 32 in 2D; any other variant
 * SF_ENOTBUILT, extents beyond those bounds SF_ENOTBUILT.  df, the bases and the derivative matrices need only scalar
 * alignment on every route.
 * Validation, before any HIP call, in this order: (1) an extent < 2 or a variant outside [0, SF_NUM_VARIANTS):
 * SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null basis, deriv, df or in_a, every output null, or -- in 3D -- only some of
 * curl0..2 null: SF_EINVAL; (4) any of them (an output: only if it is not null) not scalar-aligned: SF_EALIGN; (5) any
 * output overlapping anything the call reads or another output, compared as byte ranges of their full sizes: SF_EINVAL;
 * (6) extents beyond the fallback's bounds: SF_ENOTBUILT; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe: an overlapping output is refused, not undefined; the inputs may overlap each other.
 * No internal workspace and no allocation: every call is a single kernel node, capture-safe from the process's first
 * call.
 */
int sf_vecgrad_hex_f64(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                       const double *basis0, const double *basis1, const double *basis2,
                       const double *deriv0, const double *deriv1, const double *deriv2,
                       const double *df, const double *in0, const double *in1, const double *in2,
                       double *grad, double *div, double *curl0, double *curl1, double *curl2, void *stream);
int sf_vecgrad_hex_f64_variant(int variant, unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                               const double *basis0, const double *basis1, const double *basis2,
                               const double *deriv0, const double *deriv1, const double *deriv2,
                               const double *df, const double *in0, const double *in1, const double *in2,
                               double *grad, double *div, double *curl0, double *curl1, double *curl2, void *stream);
int sf_vecgrad_quad_f64(unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0, const double *basis1,
                        const double *deriv0, const double *deriv1, const double *df, const double *in0,
                        const double *in1, double *grad, double *div, double *curl0, void *stream);
int sf_vecgrad_quad_f64_variant(int variant, unsigned nq0, unsigned nq1, size_t nelmt, const double *basis0,
                                const double *basis1, const double *deriv0, const double *deriv1, const double *df,
                                const double *in0, const double *in1, double *grad, double *div, double *curl0,
                                void *stream);
/* T = float (AUTO route; every array 4-byte aligned) */
int sf_vecgrad_hex_f32(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt, const float *basis0,
                       const float *basis1, const float *basis2, const float *deriv0, const float *deriv1,
                       const float *deriv2, const float *df, const float *in0, const float *in1, const float *in2,
                       float *grad, float *div, float *curl0, float *curl1, float *curl2, void *stream);
int sf_vecgrad_quad_f32(unsigned nq0, unsigned nq1, size_t nelmt, const float *basis0, const float *basis1,
                        const float *deriv0, const float *deriv1, const float *df, const float *in0, const float *in1,
                        float *grad, float *div, float *curl0, void *stream);

/*
 * GATHER-SCATTER between the element-local coefficients the operators above work on and the global degrees of freedom
 * of a continuous-Galerkin space: with Q the nlocal x nglobal matrix of a local-to-global map, global_to_local applies
 * Q, assemble Q^T and gs Q Q^T, so that  A = Q^T blockdiag(H_e) Q  is  global_to_local -> sf_helmholtz_* -> assemble,
 * and the Jacobi diagonal is assemble(sf_diag_helmholtz_*).  Replaces Nektar++'s AssemblyMap::GlobalToLocal, ::Assemble
 * and ::UniversalAssemble round an operator evaluation.  The library numbers nothing: the caller passes the map.
 *
 * The map.  l2g[i], i = 0 .. nlocal-1, is the global degree of freedom of local coefficient i (i = e * nm^d + ..., the
 *   layout of the operators' `in`).  A negative entry: the coefficient belongs to no global degree of freedom (a
 *   constrained / Dirichlet coefficient).  Entries must be < nglobal.
 * The sign.  `sign` may be NULL: all +1.  Otherwise sign[i] is +1 or -1 (Nektar++'s localToGlobalSign), in the scalar
 *   type of the values; products with it are exact.
 * global_to_local:  local[i] = sign[i] * global[l2g[i]];  local[i] = 0 where l2g[i] < 0.  Every local[i] is written.
 * assemble:  global[g] = sum of sign[i] * local[i] over { i : l2g[i] == g }, the terms added in ASCENDING i, starting
 *   from the first term, one rounding per addition; a g with no local coefficient gets 0.  Every one of the nglobal
 *   outputs is written (no zeroing beforehand).  No float atomics: the result is bitwise reproducible.
 * gs:  local[i] <- sign[i] * sum_j sign[j] * local[j] over { j : l2g[j] == l2g[i] }, the sum in the order of assemble, in
 *   place.  Coefficients with l2g[i] < 0 are left untouched, and so are those alone on their global degree of freedom
 *   (sign^2 = 1).  The lists are disjoint, which is what makes the update in place safe.
 *
 * sf_gs_setup inverts the map once: it writes `rows` (nglobal words) and `perm` (nlocal words), caller-owned, the
 *   inverted index that assemble and gs walk -- CSR by global degree of freedom, the local indices of a row ascending.
 *   The content is opaque but deterministic: two calls on one map write the same bytes.  It is BLOCKING (it synchronises
 *   `stream`, like sf_sumsq_f64), takes the stream's internal scratch (not stream-capture safe) and returns SF_EINVAL if
 *   any l2g[i] >= nglobal; nothing is then written out of range and rows / perm are unusable.  A row is summed by one
 *   lane: rows far longer than a finite-element mesh produces (a few dozen entries) are correct but slow, in the setup
 *   and in assemble / gs.
 * The three apply calls are asynchronous, stateless, allocate nothing, are thread-safe and capture-safe (one kernel node
 *   each).  local, global and sign may not overlap each other, nor the index arrays.
 * Limits and validation, before any HIP call, in this order: (1) nlocal or nglobal > 2^31 - 1: SF_EINVAL; (2) a count of
 *   zero (setup: either; global_to_local: nlocal; assemble, gs: nglobal): SF_OK, nothing launched, nothing written;
 *   (3) a null pointer (sign excepted): SF_EINVAL; (4) a pointer not aligned to its own scalar (4 bytes for the int32_t
 *   arrays and float, 8 for double): SF_EALIGN.  Anything scalar-aligned works, at the same speed: the kernels access
 *   one scalar per lane, consecutive lanes on consecutive scalars.
 */
int sf_gs_setup(size_t nlocal, size_t nglobal, const int32_t *l2g, int32_t *rows, int32_t *perm, void *stream);
int sf_global_to_local_f64(size_t nlocal, const int32_t *l2g, const double *sign, const double *global, double *local,
                           void *stream);
int sf_global_to_local_f32(size_t nlocal, const int32_t *l2g, const float *sign, const float *global, float *local,
                           void *stream);
int sf_assemble_f64(size_t nglobal, const int32_t *rows, const int32_t *perm, const double *sign, const double *local,
                    double *global, void *stream);
int sf_assemble_f32(size_t nglobal, const int32_t *rows, const int32_t *perm, const float *sign, const float *local,
                    float *global, void *stream);
int sf_gs_f64(size_t nglobal, const int32_t *rows, const int32_t *perm, const double *sign, double *local, void *stream);
int sf_gs_f32(size_t nglobal, const int32_t *rows, const int32_t *perm, const float *sign, float *local, void *stream);

/*
 * TENSOR-PRODUCT APPLY with independent input and output extents: one small matrix per direction applied to every
 * element, the input length ni_d and the output length no_d of a direction named separately.  What interpolation between
 * point sets (n -> n), dealiasing and over-integration (n -> ceil(3n/2) and back), p-multigrid prolongation and
 * restriction (nc -> nf and its transpose), and BwdTrans / IProductWRTBase with a quadrature order chosen independently
 * of the polynomial order have in common.  Every other operator of this header keeps nm = nq - 1.
 *   3D: out[e][k][j][i] = sum_r sum_q sum_p in[e][r][q][p] * M0(p,i) * M1(q,j) * M2(r,k)
 *   2D: out[e][j][i]    = sum_q sum_p       in[e][q][p]    * M0(p,i) * M1(q,j)
 *   trans = 0:  M_d(a,b) = m_d[a*no_d + b]   (row-major ni_d x no_d, the layout of a BwdTrans basis)
 *   trans = 1:  M_d(a,b) = m_d[b*ni_d + a]   (row-major no_d x ni_d: the same array an IProductWRTBase reads)
 * `in` holds ni0*ni1[*ni2] scalars per element, fastest index first; `out` holds no0*no1[*no2].  One `trans` serves
 * every direction.  With A the operator of (ni, no, trans = 0, m), its transpose A^T is (no, ni, trans = 1, m): the same
 * arrays.
 * Order of operations (it defines the rounding and is the same in every kernel of the family): direction 0, then 1, then
 * 2; every sum in ascending summed index; the first term a multiplication, the rest FMAs.  Hence, by value: with
 * ni = nq - 1, no = nq, trans = 0 the result equals sf_bwdtrans_*; with ni = nq, no = nq - 1, trans = 1 it equals
 * sf_iproduct_*; and every route below gives the same bits.
 * Routes.  SF_VARIANT_AUTO with 16-byte-aligned in / out: (1) the compiled table of wave kernels -- isotropic pairs, every
 * direction the same, both trans: 3D n -> n for n 2..8, n -> ceil(3n/2) and ceil(3n/2) -> n for n 2..6; 2D n -> n for
 * n 2..16, the 3/2 pairs for n 2..10; (2) a specialisation the caller made ready with sf_specialise_tensor(); (3) the
 * any-extent kernel.  in / out aligned only to the scalar take the any-extent kernel.  SF_VARIANT_WAVE runs the table
 * only: SF_ENOTBUILT off it, SF_EALIGN unless in / out are 16-byte aligned.  SF_VARIANT_GENERIC (one workgroup per
 * element, latency-bound) takes extents from 1 up to 16 per direction in 3D and 32 in 2D, input and output independently;
 * beyond, SF_ENOTBUILT on every route.  Any other variant: SF_ENOTBUILT.  The launch configurations of the table are a
 * first choice (one rule for every shape), not tuned ones; a pair whose kernel needed scratch under that rule would get
 * smaller chunks or leave the table -- no kernel ships with scratch.  The matrices need only scalar alignment.
 * Validation, before any HIP call, in this order: (1) an extent of 0, trans other than 0 / 1 or a variant outside
 * [0, SF_NUM_VARIANTS): SF_EINVAL; (2) nelmt == 0: SF_OK; (3) a null matrix, in or out: SF_EINVAL; (4) any of them not
 * scalar-aligned: SF_EALIGN; (5) extents beyond the any-extent kernel's bounds: SF_ENOTBUILT; (6) `out` overlapping `in`,
 * compared as byte ranges of their full sizes: SF_EINVAL; (7) an unsupported variant: SF_ENOTBUILT.
 * NOT in-place safe (overlap is refused, not undefined).  No workspace, no allocation: every call is a single kernel
 * node, capture-safe from the process's first call.
 */
int sf_tensor_hex_f64(unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1, unsigned no2, int trans,
                      size_t nelmt, const double *m0, const double *m1, const double *m2, const double *in, double *out,
                      void *stream);
int sf_tensor_hex_f64_variant(int variant, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1,
                              unsigned no2, int trans, size_t nelmt, const double *m0, const double *m1, const double *m2,
                              const double *in, double *out, void *stream);
int sf_tensor_quad_f64(unsigned ni0, unsigned ni1, unsigned no0, unsigned no1, int trans, size_t nelmt, const double *m0,
                       const double *m1, const double *in, double *out, void *stream);
int sf_tensor_quad_f64_variant(int variant, unsigned ni0, unsigned ni1, unsigned no0, unsigned no1, int trans, size_t nelmt,
                               const double *m0, const double *m1, const double *in, double *out, void *stream);
/* T = float: the same routes and variants (m / in / out 4-byte aligned) */
int sf_tensor_hex_f32(unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1, unsigned no2, int trans,
                      size_t nelmt, const float *m0, const float *m1, const float *m2, const float *in, float *out,
                      void *stream);
int sf_tensor_hex_f32_variant(int variant, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1,
                              unsigned no2, int trans, size_t nelmt, const float *m0, const float *m1, const float *m2,
                              const float *in, float *out, void *stream);
int sf_tensor_quad_f32(unsigned ni0, unsigned ni1, unsigned no0, unsigned no1, int trans, size_t nelmt, const float *m0,
                       const float *m1, const float *in, float *out, void *stream);
int sf_tensor_quad_f32_variant(int variant, unsigned ni0, unsigned ni1, unsigned no0, unsigned no1, int trans, size_t nelmt,
                               const float *m0, const float *m1, const float *in, float *out, void *stream);
/* Compile (once per process) and load (once per device) the wave kernel of one tensor shape, as sf_specialise() does for
 * BwdTrans and under keys of its own: dim 2 or 3 (dim 2 ignores ni2 / no2), every extent 1..16 in 3D and 1..24 in 2D,
 * trans 0 / 1, scalar_bytes 8 or 4; anything else SF_EINVAL.  SF_OK: ready, AUTO calls of sf_tensor_* on that shape with
 * 16-byte-aligned in / out launch it (and count the launch) unless the compiled table holds the shape.  SF_ECOMPILE: the
 * shape is refused -- one wave's LDS slab would exceed 64 KiB, the kernel would need scratch, hiprtc is missing, or a
 * stream capture is under way on the device (nothing is compiled then) -- and AUTO keeps the any-extent kernel.  Never
 * called behind a launch.  The log is sf_last_specialise_log(); sf_shutdown() unloads the modules.
 * sf_tensor_specialisation_state: 0 none, 1 ready, SF_ECOMPILE refused; *launches (may be NULL) the launches so far. */
int sf_specialise_tensor(int dim, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1, unsigned no2,
                         int trans, int scalar_bytes);
int sf_tensor_specialisation_state(int dim, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1,
                                   unsigned no2, int trans, int scalar_bytes, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* SUMFACT_H */
