// frag/sweep.inc -- one sweep of a wave kernel, "lane owns a pencil": read the pencils, contract them, scatter the
// results so that the next sweep's pencils are contiguous.  Every forward, IProduct and transposed sweep that stores in
// the form of Sweep (bwdtrans_wave.h) is this text.
// Expects: T, BMODE; slab, lane.
// Parameters, defined by the kernel just before the #include and undefined here (SWEEP by frag/sweep_store.inc):
//   SWEEP            a Sweep: lane t = (e, a, b) owns a pencil of NIN values at stride SIN, value o of its NOUT results
//                    goes to slab[((e*NOUT + o)*A + a)*SOUT + b]
//   SWEEP_CONTRACT   contract (the basis is row-major NIN x NOUT) or contract_dot (NOUT x NIN)
//   SWEEP_BASIS      the basis of the direction
// Slab before: SWEEP::NP pencils of stride SWEEP::SIN.  After: the image described above, fenced.
        {
            T u[SWEEP::PASS][SWEEP::NIN], acc[SWEEP::PASS][SWEEP::NOUT];
            read_pencils<SWEEP::NIN, SWEEP::PASS, SWEEP::NP, SWEEP::SIN>(u, slab, lane);
            SWEEP_CONTRACT<SWEEP::NIN, SWEEP::NOUT, SWEEP::PASS, BMODE>(u, acc, SWEEP_BASIS);
#include "sweep_store.inc"
        }
#undef SWEEP_CONTRACT
#undef SWEEP_BASIS
