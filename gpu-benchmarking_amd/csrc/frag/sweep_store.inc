// frag/sweep_store.inc -- the scatter half of frag/sweep.inc, behind a contraction the kernel writes itself.
// Expects: T; slab, lane; acc[SWEEP::PASS][SWEEP::NOUT], the results of the lane's pencils.
// Parameter, defined by the kernel just before the #include and undefined here:
//   SWEEP   a Sweep (bwdtrans_wave.h): result o of pencil t = (e, a, b) goes to slab[((e*NOUT + o)*A + a)*SOUT + b]
// Slab before: whatever the pencils were read from; its readers must be done (the fragment fences before it stores).
// After: the image described above, fenced.  Lanes of a partial last pass store nothing.
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < SWEEP::PASS; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= SWEEP::NP || t < SWEEP::NP)
                {
                    // A == 1: a is the constant 0, not ab / B (the compiler does not know that ab < B)
                    const int e = t / (SWEEP::A * SWEEP::B), ab = t - e * (SWEEP::A * SWEEP::B);
                    const int a = SWEEP::A == 1 ? 0 : ab / SWEEP::B, b = ab - a * SWEEP::B;
                    T *dst = slab + (e * SWEEP::NOUT * SWEEP::A + a) * SWEEP::SOUT + b;
#pragma unroll
                    for (int o = 0; o < SWEEP::NOUT; ++o)
                        dst[o * SWEEP::A * SWEEP::SOUT] = acc[s][o];
                }
            }
            wave_lds_fence();
#undef SWEEP
