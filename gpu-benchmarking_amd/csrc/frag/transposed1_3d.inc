// frag/transposed1_3d.inc -- second transposed sweep of a hex, j -> q': lane (e,r',i) owns a j-pencil.  An instance of
// frag/sweep.inc, with (e,r') in the place of its e.
// Expects: M (MassGeom of the order: SwT1); T, BMODE; b1 (nm x nq); slab, lane.
// Slab before: t2[(e,r',i)][j] (frag/transposed_last_3d.inc).  After: t1[(e,r',q')][i], pencil stride NQP, fenced.
        // ---- transposed 1: t1[(e,r',q')][i] = sum_j t2[(e,r',i)][j] * B1[q'][j] --------------------
#define SWEEP M::SwT1
#define SWEEP_CONTRACT contract_dot
#define SWEEP_BASIS b1
#include "sweep.inc"
