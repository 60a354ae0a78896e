// frag/fields_front_3d.inc -- the front of a hex wave kernel over d fields: frag/geom_coordinate_3d.inc once per field
// (x0, x1, x2), with the kernel's own requests in front of the last field's unit, in flight under its sweeps.
// Expects: everything frag/geom_coordinate_3d.inc expects.
// Parameters, defined by the kernel just before the #include and undefined here:
//   FRONT_PRIME   the statements in front of the last field's unit: the ring primed, the constants of the chunk's
//                 elements loaded; may be empty
// Slab before: dead.  After: the six images of d u_a / d xi_1 and d u_a / d xi_0 (fields 0 and 1: kept; field 2: slab),
// fenced; dk[a] = d u_a / d xi_2 over k; st holds x0 of the wave's next chunk.
#define GEOM_A 0
#define GEOM_X x0
#define GEOM_NEXT x1
#include "geom_coordinate_3d.inc"
#define GEOM_A 1
#define GEOM_X x1
#define GEOM_NEXT x2
#include "geom_coordinate_3d.inc"
        FRONT_PRIME
#define GEOM_A 2
#define GEOM_X x2
#define GEOM_NEXT x0
#include "geom_coordinate_3d.inc"
#undef FRONT_PRIME
