// frag/advect_field_back.inc -- the back of one field of the advection kernels: the transposed sweeps of the mass kernel out
// of the register pencil dk[ADV_A] into ADV_OUT.  Included once per field (a loop over the fields is not reliably
// unrolled, as frag/geom_coordinate_3d.inc says).  The shared fragments take `u` and `out` from the scope; this one gives
// them those names for the field at hand, which is all it adds to them.
// Expects: everything transposed_last_{2d,3d}, transposed1_3d and transposed0 expect but u, acc and out; dk.
// Parameters, defined by the kernel just before the #include and undefined here:
//   ADV_DIM      2 or 3
//   ADV_A        the field, 0 .. d-1
//   ADV_OUT      its modes, out0 .. out2
// Slab before: dead, its readers fenced.  After: dead -- out_a of the chunk has been flushed, fenced.
        {
            T *out = ADV_OUT;
            {
                T(&u)[NPASS][NQ] = dk[ADV_A];
                T acc[NPASS][NM];
#if ADV_DIM == 3
#include "transposed_last_3d.inc"
#else
#include "transposed_last_2d.inc"
#endif
            }
#if ADV_DIM == 3
#include "transposed1_3d.inc"
#endif
#include "transposed0.inc"
        }
#undef ADV_DIM
#undef ADV_A
#undef ADV_OUT
