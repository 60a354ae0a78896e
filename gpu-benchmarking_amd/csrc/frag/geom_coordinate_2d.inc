// frag/geom_coordinate_2d.inc -- one unit of work of the quad geometric-factor kernel: coordinate GEOM_A of chunk c through
// the front of the gradient kernels.  Included once per coordinate, as frag/geom_coordinate_3d.inc.
// Expects: everything chunk_stage, forward0 and point_values_2d expect but `in` and imgU; x0, x1; kept; st, AL; it, n, c;
//          dk[2][NPASS][NQ].
// Parameters, defined by the kernel just before the #include and undefined here:
//   GEOM_A       the coordinate, 0 or 1
//   GEOM_X       its modes, x0 or x1
// Slab before: dead.  After: d X_a / d xi_0 in the image of the coordinate (kept; the last coordinate: slab), fenced;
// dk[GEOM_A] = d X_a / d xi_1 over j; st holds the next unit's modes.
        {
            const T *in = GEOM_X;
            T *imgU     = GEOM_A == 1 ? slab : kept; // X_a, then d X_a / d xi_0
#include "chunk_stage.inc"
            // the next unit's modes: x_1 of this chunk, or x_0 of the wave's next chunk
#if GEOM_A < 1
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, x1, c, nelmt, lane);
#else
            if (n + 1 < it.count)
                chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, x0, c + it.step, nelmt, lane);
#endif
#include "forward0.inc"
            {
                T u[NPASS][NQ], dreg[NPASS][NQ];
#include "point_values_2d.inc"
#pragma unroll
                for (int s = 0; s < NPASS; ++s)
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        dk[GEOM_A][s][j] = dreg[s][j];
            }
        }
#undef GEOM_A
#undef GEOM_X
