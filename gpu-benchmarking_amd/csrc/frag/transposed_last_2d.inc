// frag/transposed_last_2d.inc -- first transposed sweep of a quad, j -> q', out of the registers of the column's lane.
// Expects: T, NM, NQ, NQP, NPASS, BMODE; b1 (nm x nq); slab, lane; own; u[NPASS][NQ] = v, the point values to project,
//          over j; acc[NPASS][NM], declared by the kernel.
// Slab before: whatever the kernel kept there; its readers must be done (the sweep fences before it stores).
// After: t1[(e,q')][i], pencil stride NQP, fenced.
            // ---- transposed 1: t1[(e,q')][i] = sum_j v[j] * B1[q'][j] --------------------------------
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ, i = t - e * NQ;
                    T *dst = slab + e * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
