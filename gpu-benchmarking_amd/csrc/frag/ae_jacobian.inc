// frag/ae_jacobian.inc -- J[a][b] = D_b u_a of one point of an any-extent element behind frag/ae_fields_forward.inc, inside
// the kernel's loop over its points x: frag/ae_deriv_{2d,3d}.inc once per field.
// Expects: everything frag/ae_deriv_{2d,3d}.inc expect but P0; DIM; R0 .. R(d-1), the point images of the fields;
//          J[DIM][DIM].
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_POINT_WITH(i, j, k)   statements that take the indices of the point (k = 0 in 2D), e.g. its quadrature weight;
//                            may be empty
            if constexpr (DIM == 2)
            {
                {
                    const T *P0 = R0;
#define AE_DU0 J[0][0]
#define AE_DU1 J[0][1]
#include "ae_deriv_2d.inc"
                    AE_POINT_WITH(i, j, 0)
                }
                {
                    const T *P0 = R1;
#define AE_DU0 J[1][0]
#define AE_DU1 J[1][1]
#include "ae_deriv_2d.inc"
                }
            }
            else
            {
                {
                    const T *P0 = R0;
#define AE_DU0 J[0][0]
#define AE_DU1 J[0][1]
#define AE_DU2 J[0][2]
#include "ae_deriv_3d.inc"
                    AE_POINT_WITH(i, j, k)
                }
                {
                    const T *P0 = R1;
#define AE_DU0 J[1][0]
#define AE_DU1 J[1][1]
#define AE_DU2 J[1][2]
#include "ae_deriv_3d.inc"
                }
                {
                    const T *P0 = R2;
#define AE_DU0 J[2][0]
#define AE_DU1 J[2][1]
#define AE_DU2 J[2][2]
#include "ae_deriv_3d.inc"
                }
            }
#undef AE_POINT_WITH
