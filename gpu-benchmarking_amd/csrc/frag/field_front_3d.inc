// frag/field_front_3d.inc -- the front of a hex wave kernel over one field (advect, affine_advect with NF = 1): the front
// of the gradient kernels, physderiv_wave.h, with the kernel's own requests right after the chunk is staged.
// Expects: everything chunk_stage, chunk_fetch_next, forward0, forward1_3d and point_values_3d expect but imgU, imgD, u
//          and dreg; dk.
// Parameters, defined by the kernel just before the #include and undefined here:
//   FRONT_PRIME   the statements behind chunk_stage: the ring primed, the constants of the chunk's elements loaded
// Slab before: dead.  After: d u / d xi_1 and d u / d xi_0 in the first two images, fenced; dk[0] = d u / d xi_2 over k;
// st holds the modes of the wave's next chunk.
            T *imgU = slab;          // u, then du / d xi_1
            T *imgD = slab + G::IMG; // du / d xi_0
#include "chunk_stage.inc"
            FRONT_PRIME
#include "chunk_fetch_next.inc"
#include "forward0.inc"
#include "forward1_3d.inc"
            {
                T u[NPASS][NQ];
                T(&dreg)[NPASS][NQ] = dk[0];
#include "point_values_3d.inc"
            }
#undef FRONT_PRIME
