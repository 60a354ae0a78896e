// frag/transposed1_3d.inc -- second transposed sweep of a hex, j -> q': lane (e,r',i) owns a j-pencil.
// Expects: M (MassGeom of the order: PASST2, PT2); T, NM, NQ, NQP, BMODE; b1 (nm x nq); slab, lane.
// Slab before: t2[(e,r',i)][j] (frag/transposed_last_3d.inc).  After: t1[(e,r',q')][i], pencil stride NQP, fenced.
        // ---- transposed 1: t1[(e,r',q')][i] = sum_j t2[(e,r',i)][j] * B1[q'][j] --------------------
        {
            T u[M::PASST2][NQ], acc[M::PASST2][NM];
            read_pencils<NQ, M::PASST2, M::PT2, NQP>(u, slab, lane);
            contract_dot<NQ, NM, M::PASST2, BMODE>(u, acc, b1);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < M::PASST2; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= M::PT2 || t < M::PT2)
                {
                    const int er = t / NQ, i = t - er * NQ; // er = e*NM + r'
                    T *dst = slab + er * NM * NQP + i;
#pragma unroll
                    for (int q = 0; q < NM; ++q)
                        dst[q * NQP] = acc[s][q];
                }
            }
            wave_lds_fence();
        }
