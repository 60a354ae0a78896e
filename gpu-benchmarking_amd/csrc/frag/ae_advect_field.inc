// frag/ae_advect_field.inc -- one field of an any-extent advection kernel, the body of its loop over the fields a: forward
// sweeps, r_a = [weight] (sum_b beta_b D_b u_a) with beta_b = sum_j c_j df[j*d + b] at every point, transposed sweeps.
//   3D: in_a (B) -> w1 (A) -> w2 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> t2 (B) -> out_a (HBM)
//   2D: in_a (A) -> w1 (B) -> u_a (A) -> r_a (B) -> t1 (A) -> out_a (HBM)
// Expects: everything frag/ae_forward_*, ae_deriv_* and ae_transposed_* expect but src, dst and P0; DIM; A, B, two
//          regions of nqt scalars; x0 .. x2, out0 .. out2; e, a; ce0, ce1, ce2, the planes of c of the element.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_ADV_DF(c)                 entry c = j*d + b of the inverse Jacobian at the point x
//   AE_ADV_VALUE(r, i, j, k)     the statement that stores the point's value into B[x], of its sum r and its indices
//                                (k = 0 in 2D)
// After: out_a of the element is written; the regions are dead, behind a barrier.
            const T *src = (a == 0 ? x0 : (a == 1 ? x1 : x2)) + e * (uint64_t)nmt;
            T *dst       = (a == 0 ? out0 : (a == 1 ? out1 : out2)) + e * (uint64_t)nmt;
            const T *P0  = A; // the point image of u_a
            if constexpr (DIM == 2)
            {
#define AE_MODES A
#define AE_W1 B
#define AE_POINTS A
#define AE_POINT_VALUE(s) s
#include "ae_forward_2d.inc"
                for (int x = tid; x < nqt; x += NT)
                {
                    T J0, J1;
#define AE_DU0 J0
#define AE_DU1 J1
#include "ae_deriv_2d.inc"
                    const T v0 = ce0[x], v1 = ce1[x];
                    const T be0 = sfma(v1, AE_ADV_DF(2), v0 * AE_ADV_DF(0));
                    const T be1 = sfma(v1, AE_ADV_DF(3), v0 * AE_ADV_DF(1));
                    AE_ADV_VALUE(sfma(be1, J1, be0 * J0), i, j, 0)
                }
                __syncthreads();
#define AE_POINTS B
#define AE_T1 A
#include "ae_transposed_2d.inc"
            }
            else
            {
#define AE_MODES B
#define AE_W1 A
#define AE_W2 B
#define AE_POINTS A
#define AE_POINT_VALUE(s) s
#include "ae_forward_3d.inc"
                for (int x = tid; x < nqt; x += NT)
                {
                    T J0, J1, J2;
#define AE_DU0 J0
#define AE_DU1 J1
#define AE_DU2 J2
#include "ae_deriv_3d.inc"
                    const T v0 = ce0[x], v1 = ce1[x], v2 = ce2[x];
                    const T be0 = sfma(v2, AE_ADV_DF(6), sfma(v1, AE_ADV_DF(3), v0 * AE_ADV_DF(0)));
                    const T be1 = sfma(v2, AE_ADV_DF(7), sfma(v1, AE_ADV_DF(4), v0 * AE_ADV_DF(1)));
                    const T be2 = sfma(v2, AE_ADV_DF(8), sfma(v1, AE_ADV_DF(5), v0 * AE_ADV_DF(2)));
                    AE_ADV_VALUE(sfma(be2, J2, sfma(be1, J1, be0 * J0)), i, j, k)
                }
                __syncthreads();
#define AE_POINTS B
#define AE_T1 A
#define AE_T2 B
#include "ae_transposed_3d.inc"
            }
            __syncthreads(); // the next field, or the next element, overwrites the images
#undef AE_ADV_DF
#undef AE_ADV_VALUE
