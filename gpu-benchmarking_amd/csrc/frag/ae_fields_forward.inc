// frag/ae_fields_forward.inc -- the d fields of an any-extent element forward into point images that stay: field a into
// R(a), its sweeps in the regions behind its image (geom_generic.hip, vecgrad_generic.hip).
//   3D, field a: modes (R(a+1)) -> w1 (Ra) -> w2 (R(a+1)) -> u_a (Ra)
//   2D, field a: modes (R(a+1)) -> w1 (behind the modes, fewer than 2 nqt scalars in all) -> u_a (Ra)
// Expects: everything frag/ae_forward_{2d,3d}.inc expect but src; DIM; R0 .. R3, four regions of nqt scalars; x0, x1 (3D:
//          x2), the modes of the fields; e, the element.
// After: R0 .. R(d-1) hold the point images of the fields, behind a barrier.
        if constexpr (DIM == 2)
        {
            (void)R3;
            {
                const T *src = x0 + e * (uint64_t)nmt;
                T *W1        = R1 + nmt;
#define AE_MODES R1
#define AE_W1 W1
#define AE_POINTS R0
#define AE_POINT_VALUE(s) s
#include "ae_forward_2d.inc"
            }
            {
                const T *src = x1 + e * (uint64_t)nmt;
                T *W1        = R2 + nmt;
#define AE_MODES R2
#define AE_W1 W1
#define AE_POINTS R1
#define AE_POINT_VALUE(s) s
#include "ae_forward_2d.inc"
            }
        }
        else
        {
            {
                const T *src = x0 + e * (uint64_t)nmt;
#define AE_MODES R1
#define AE_W1 R0
#define AE_W2 R1
#define AE_POINTS R0
#define AE_POINT_VALUE(s) s
#include "ae_forward_3d.inc"
            }
            {
                const T *src = x1 + e * (uint64_t)nmt;
#define AE_MODES R2
#define AE_W1 R1
#define AE_W2 R2
#define AE_POINTS R1
#define AE_POINT_VALUE(s) s
#include "ae_forward_3d.inc"
            }
            {
                const T *src = x2 + e * (uint64_t)nmt;
#define AE_MODES R3
#define AE_W1 R2
#define AE_W2 R3
#define AE_POINTS R2
#define AE_POINT_VALUE(s) s
#include "ae_forward_3d.inc"
            }
        }
