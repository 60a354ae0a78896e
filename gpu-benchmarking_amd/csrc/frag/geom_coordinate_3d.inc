// frag/geom_coordinate_3d.inc -- one unit of work of the hex geometric-factor kernel: coordinate GEOM_A of chunk c through
// the front of the gradient kernels.  Included once per coordinate (a loop over the coordinates is not reliably unrolled,
// and the register pencils dk would then live in scratch).
// Expects: everything chunk_stage, forward0, forward1_3d and point_values_3d expect but `in`, imgU and imgD; x0, x1, x2;
//          kept; st, AL; it, n, c; dk[3][NPASS][NQ].
// Parameters, defined by the kernel just before the #include and undefined here:
//   GEOM_A       the coordinate, 0 .. 2
//   GEOM_X       its modes, x0 .. x2
//   GEOM_NEXT    the modes of the next coordinate (GEOM_A < 2 only)
// Slab before: dead.  After: d X_a / d xi_1 and d X_a / d xi_0 in the two images of the coordinate (kept; the last
// coordinate: slab), fenced; dk[GEOM_A] = d X_a / d xi_2 over k; st holds the next unit's modes.
        {
            const T *in = GEOM_X;
            T *imgU     = GEOM_A == 2 ? slab : kept + (2 * GEOM_A) * G::IMG;              // X_a, then d X_a / d xi_1
            T *imgD     = GEOM_A == 2 ? slab + G::IMG : kept + (2 * GEOM_A + 1) * G::IMG; // d X_a / d xi_0
#include "chunk_stage.inc"
            // the next unit's modes: the next coordinate of this chunk, or x_0 of the wave's next chunk
#if GEOM_A < 2
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, GEOM_NEXT, c, nelmt, lane);
#else
            if (n + 1 < it.count)
                chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, x0, c + it.step, nelmt, lane);
#endif
#include "forward0.inc"
#include "forward1_3d.inc"
            {
                T u[NPASS][NQ], dreg[NPASS][NQ];
#include "point_values_3d.inc"
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
#pragma unroll
                    for (int k = 0; k < NQ; ++k)
                        dk[GEOM_A][s][k] = dreg[s][k];
            }
        }
#undef GEOM_A
#undef GEOM_X
#undef GEOM_NEXT
