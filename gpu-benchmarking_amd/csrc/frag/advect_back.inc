// frag/advect_back.inc -- the back of the advection kernels over all their fields: frag/advect_field_back.inc for field 0
// and, with NF = d, for the fields 1 .. d-1.
// Expects: everything frag/advect_field_back.inc expects; NF; out0, out1 (3D: out2).
// Parameters, defined by the kernel just before the #include and undefined here:
//   ADV_BACK_DIM   2 or 3
// Slab before: dead, its readers fenced.  After: dead -- out_a of the chunk has been flushed for every field, fenced.
#define ADV_DIM ADV_BACK_DIM
#define ADV_A 0
#define ADV_OUT out0
#include "advect_field_back.inc"
        if constexpr (NF == ADV_BACK_DIM)
        {
#define ADV_DIM ADV_BACK_DIM
#define ADV_A 1
#define ADV_OUT out1
#include "advect_field_back.inc"
#if ADV_BACK_DIM == 3
#define ADV_DIM 3
#define ADV_A 2
#define ADV_OUT out2
#include "advect_field_back.inc"
#endif
        }
#undef ADV_BACK_DIM
