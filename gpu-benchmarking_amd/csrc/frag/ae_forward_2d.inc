// frag/ae_forward_2d.inc -- an any-extent quad's way in: the modes staged from HBM, then the forward sweeps p -> i, q -> j.
// Expects: T, NT; tid, nq0, nq1, nm0, nm1, nqt, nmt (frag/ae_prologue.inc); b0, b1 (nm x nq); src.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_MODES, AE_W1, AE_POINTS   LDS images: modes -> w1 -> points; AE_W1 overlaps neither of the other two
//   AE_POINT_VALUE(s)            what a point stores, of its sum s and its index x
// After: AE_POINTS holds the point image, behind a barrier.
            for (int x = tid; x < nmt; x += NT)
                AE_MODES[x] = src[x];
            __syncthreads();
            // forward 0: w1[q][i] = sum_p in[q][p] * B0[p][i]
            for (int x = tid; x < nm1 * nq0; x += NT)
            {
                const int i = x % nq0, q = x / nq0;
                AE_W1[x] = dot_strided(AE_MODES + q * nm0, 1, b0 + i, nq0, nm0);
            }
            __syncthreads();
            // forward 1: u[j][i] = sum_q w1[q][i] * B1[q][j]
            for (int x = tid; x < nqt; x += NT)
            {
                const int i = x % nq0, j = x / nq0;
                AE_POINTS[x] = AE_POINT_VALUE(dot_strided(AE_W1 + i, nq0, b1 + j, nq1, nm1));
            }
            __syncthreads();
#undef AE_MODES
#undef AE_W1
#undef AE_POINTS
#undef AE_POINT_VALUE
