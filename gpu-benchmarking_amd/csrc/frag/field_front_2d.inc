// frag/field_front_2d.inc -- the front of a quad wave kernel over one field, as frag/field_front_3d.inc.
// Expects: everything chunk_stage, chunk_fetch_next, forward0 and point_values_2d expect but imgU, u and dreg; dk.
// Parameters, defined by the kernel just before the #include and undefined here:
//   FRONT_PRIME   the statements behind chunk_stage
// Slab before: dead.  After: d u / d xi_0 in the first image, fenced; dk[0] = d u / d xi_1 over j; st holds the modes of
// the wave's next chunk.
            T *imgU = slab; // u, then du / d xi_0
#include "chunk_stage.inc"
            FRONT_PRIME
#include "chunk_fetch_next.inc"
#include "forward0.inc"
            {
                T u[NPASS][NQ];
                T(&dreg)[NPASS][NQ] = dk[0];
#include "point_values_2d.inc"
            }
#undef FRONT_PRIME
