// frag/ae_transposed_3d.inc -- an any-extent hex's way out: the transposed sweeps k -> r', j -> q', i -> p', the last one
// to HBM.
// Expects: T, NT; tid, nq0, nq1, nq2, nm0, nm1, nm2, n01, nmt (frag/ae_prologue.inc); b0, b1, b2 (nm x nq); dst.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_POINTS, AE_T1, AE_T2   LDS images: points (complete, behind a barrier) -> t1 -> t2; neighbours do not overlap
// After: dst is written; no barrier since.
            // transposed 2: t1[r'][j][i] = sum_k v[k][j][i] * B2[r'][k]
            for (int x = tid; x < n01 * nm2; x += NT)
            {
                const int ji = x % n01, r = x / n01;
                AE_T1[x] = dot_strided(AE_POINTS + ji, n01, b2 + r * nq2, 1, nq2);
            }
            __syncthreads();
            // transposed 1: t2[r'][q'][i] = sum_j t1[r'][j][i] * B1[q'][j]
            for (int x = tid; x < nq0 * nm1 * nm2; x += NT)
            {
                const int i = x % nq0, rq = x / nq0, q = rq % nm1, r = rq / nm1;
                AE_T2[x] = dot_strided(AE_T1 + r * n01 + i, nq0, b1 + q * nq1, 1, nq1);
            }
            __syncthreads();
            // transposed 0: out[r'][q'][p'] = sum_i t2[r'][q'][i] * B0[p'][i]
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, rq = x / nm0;
                dst[x] = dot_strided(AE_T2 + rq * nq0, 1, b0 + p * nq0, 1, nq0);
            }
#undef AE_POINTS
#undef AE_T1
#undef AE_T2
