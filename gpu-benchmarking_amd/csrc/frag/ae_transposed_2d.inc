// frag/ae_transposed_2d.inc -- an any-extent quad's way out: the transposed sweeps j -> q', i -> p', the last one to HBM.
// Expects: T, NT; tid, nq0, nq1, nm0, nm1, nmt (frag/ae_prologue.inc); b0, b1 (nm x nq); dst.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_POINTS, AE_T1   LDS images: points (complete, behind a barrier) -> t1, which do not overlap
// After: dst is written; no barrier since.
            // transposed 1: t1[q'][i] = sum_j v[j][i] * B1[q'][j]
            for (int x = tid; x < nm1 * nq0; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                AE_T1[x] = dot_strided(AE_POINTS + i, nq0, b1 + q * nq1, 1, nq1);
            }
            __syncthreads();
            // transposed 0: out[q'][p'] = sum_i t1[q'][i] * B0[p'][i]
            for (int x = tid; x < nmt; x += NT)
            {
                const int p = x % nm0, q = x / nm0;
                dst[x] = dot_strided(AE_T1 + q * nq0, 1, b0 + p * nq0, 1, nq0);
            }
#undef AE_POINTS
#undef AE_T1
