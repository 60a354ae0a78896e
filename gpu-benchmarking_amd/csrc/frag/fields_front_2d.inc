// frag/fields_front_2d.inc -- the front of a quad wave kernel over d fields: frag/geom_coordinate_2d.inc once per field
// (x0, x1), as frag/fields_front_3d.inc.
// Expects: everything frag/geom_coordinate_2d.inc expects.
// Parameters, defined by the kernel just before the #include and undefined here:
//   FRONT_PRIME   the statements in front of the last field's unit; may be empty
// Slab before: dead.  After: the two images of d u_a / d xi_0 (field 0: kept; field 1: slab), fenced; dk[a] = d u_a / d xi_1
// over j; st holds x0 of the wave's next chunk.
#define GEOM_A 0
#define GEOM_X x0
#include "geom_coordinate_2d.inc"
        FRONT_PRIME
#define GEOM_A 1
#define GEOM_X x1
#include "geom_coordinate_2d.inc"
#undef FRONT_PRIME
