// frag/transposed0.inc -- last transposed sweep, i -> p', and the chunk's way out.  One text for hex and quad: lane
// t = (e,r',q') (quad: (e,q')) owns an i-pencil and its row of the output image.
// Expects: M (MassGeom of the order: PASST1, PT1, OUT_DBL, NMT); IO; T, NM, NQ, NQP, BMODE, MEMF; b0 (nm x nq); out, c,
//          evalid; slab, lane.
// Slab before: t1[t][i], pencil stride NQP (frag/transposed1_3d.inc, frag/transposed_last_2d.inc).  After: dead -- the
// output image out[t][p'] has been flushed to HBM, the elements of the chunk that exist only, and fenced: the next
// chunk may write the slab.
        // ---- transposed 0: out[e][r'][q'][p'] = sum_i t1[(e,r',q')][i] * B0[p'][i]   (quad: without r') ----
        {
            T u[M::PASST1][NQ], acc[M::PASST1][NM];
            read_pencils<NQ, M::PASST1, M::PT1, NQP>(u, slab, lane);
            contract_dot<NQ, NM, M::PASST1, BMODE>(u, acc, b0);
            wave_lds_fence();
#pragma unroll
            for (int s = 0; s < M::PASST1; ++s)
            {
                const int t = s * kWave + lane;
                if ((s + 1) * kWave <= M::PT1 || t < M::PT1)
                {
                    T *dst = slab + t * NM;
#pragma unroll
                    for (int p = 0; p < NM; ++p)
                        dst[p] = acc[s][p];
                }
            }
            wave_lds_fence();
            chunk_flush<IO, !(MEMF & 2), (MEMF & 8) != 0>(slab, out + c * (uint64_t)M::OUT_DBL, evalid * M::NMT, lane);
            wave_lds_fence();
        }
