// frag/forward0.inc -- first forward sweep of a hex or quad, p -> i: lane (e,r,q) (quad: (e,q)) owns a p-pencil of the
// input.  An instance of frag/sweep.inc.
// Expects: F (WaveGeom of the order); T, BMODE; b0 (row-major nm x nq); slab, lane.
// Slab before: the input image in[(e,r,q)][p], pencil stride F::IN_STRIDE.  After: w1[(e,i,r)][q] (quad: w1[(e,i)][q]),
// pencil stride F::NMP, fenced.
        // ---- forward 0: w1[(e,i,r)][q] = sum_p in[(e,r,q)][p] * B0[p][i]   (quad: without r) --------
#define SWEEP F::Sw0
#define SWEEP_CONTRACT contract
#define SWEEP_BASIS b0
#include "sweep.inc"
