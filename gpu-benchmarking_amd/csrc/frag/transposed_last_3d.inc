// frag/transposed_last_3d.inc -- first transposed sweep of a hex, k -> r', out of the registers of the column's lane.
// Expects: T, NM, NQ, NQ2, NQP, NPASS, BMODE; b2 (nm x nq); slab, lane; own; u[NPASS][NQ] = v, the point values to
//          project, over k; acc[NPASS][NM], declared by the kernel.
// Slab before: whatever the kernel kept there; its readers must be done (the sweep fences before it stores).
// After: t2[(e,r',i)][j], pencil stride NQP, fenced.
            // ---- transposed 2: t2[(e,r',i)][j] = sum_k v[k] * B2[r'][k] ------------------------------
            contract_dot<NQ, NM, NPASS, BMODE>(u, acc, b2);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                const int t = s * kWave + lane;
                if (own[s])
                {
                    const int e = t / NQ2, ji = t - e * NQ2, j = ji / NQ, i = ji - j * NQ;
                    T *dst = slab + (e * NM * NQ + i) * NQP + j;
#pragma unroll
                    for (int r = 0; r < NM; ++r)
                        dst[r * NQ * NQP] = acc[s][r];
                }
            }
            wave_lds_fence();
