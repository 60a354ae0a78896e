// frag/forward1_3d.inc -- second forward sweep of a hex, q -> j: lane (e,i,r) owns a q-pencil.  An instance of
// frag/sweep.inc.
// Expects: F; T, BMODE; b1 (row-major nm x nq); slab, lane.
// Slab before: w1[(e,i,r)][q] (frag/forward0.inc).  After: w2[(e,j,i)][r], pencil stride F::NMP, fenced -- the
// r-pencils of the point columns, which the last forward sweep takes into registers.
        // ---- forward 1: w2[(e,j,i)][r] = sum_q w1[(e,i,r)][q] * B1[q][j] ---------------------------
#define SWEEP F::Sw1
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b1
#include "sweep.inc"
