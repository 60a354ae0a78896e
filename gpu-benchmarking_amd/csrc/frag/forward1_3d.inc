// frag/forward1_3d.inc -- second forward sweep of a hex, q -> j: lane (e,i,r) owns a q-pencil.
// Expects: F; T, NM, NQ, NQ2, NMP, BMODE; b1 (row-major nm x nq); slab, lane.
// Slab before: w1[(e,i,r)][q] (frag/forward0_3d.inc).  After: w2[(e,j,i)][r], pencil stride NMP, fenced -- the
// r-pencils of the point columns, which the last forward sweep takes into registers.
        // ---- forward 1: w2[(e,j,i)][r] = sum_q w1[(e,i,r)][q] * B1[q][j] ---------------------------
        {
            T u[F::PASS1][NM], acc[F::PASS1][NQ];
            read_pencils<NM, F::PASS1, F::P1, NMP>(u, slab, lane);
            contract<NM, NQ, F::PASS1, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < F::PASS1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= F::P1 || t < F::P1)
                {
                    const int e = t / (NQ * NM), ir = t - e * (NQ * NM), i = ir / NM, r = ir - i * NM;
                    T *dst = slab + (e * NQ2 + i) * NMP + r;
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        dst[j * NQ * NMP] = acc[s][j];
                }
            }
            wave_lds_fence();
        }
