// frag/forward0_2d.inc -- first forward sweep of a quad, p -> i: lane (e,q) owns a p-pencil of the input.
// Expects: F (WaveGeom of the order); T, NM, NQ, NMP, BMODE; b0 (row-major nm x nq); slab, lane.
// Slab before: the input image in[(e,q)][p], pencil stride F::IN_STRIDE.  After: w1[(e,i)][q], pencil stride NMP,
// fenced.
        // ---- forward 0: w1[(e,i)][q] = sum_p in[(e,q)][p] * B0[p][i] -------------------------------
        {
            T u[F::PASS0][NM], acc[F::PASS0][NQ];
            read_pencils<NM, F::PASS0, F::P0, F::IN_STRIDE>(u, slab, lane);
            contract<NM, NQ, F::PASS0, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < F::PASS0; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= F::P0 || t < F::P0)
                {
                    const int e = t / NM, q = t - e * NM;
                    T *dst = slab + e * NQ * NMP + q;
#pragma unroll
                    for (int i = 0; i < NQ; ++i)
                        dst[i * NMP] = acc[s][i];
                }
            }
            wave_lds_fence();
        }
