// frag/ae_forward_3d.inc -- an any-extent hex's way in: the modes staged from HBM, then the forward sweeps p -> i, q -> j,
// r -> k.
// Expects: T, NT; tid, nq0, nq1, nq2, nm0, nm1, nm2, n01, nqt, nmt (frag/ae_prologue.inc); b0, b1, b2 (nm x nq); src.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_MODES, AE_W1, AE_W2, AE_POINTS   LDS images: modes -> w1 -> w2 -> points; neighbours do not overlap
//   AE_POINT_VALUE(s)                   what a point stores, of its sum s and its index x
// After: AE_POINTS holds the point image, behind a barrier.
            for (int x = tid; x < nmt; x += NT)
                AE_MODES[x] = src[x];
            __syncthreads();
            // forward 0: w1[r][q][i] = sum_p in[r][q][p] * B0[p][i]
            for (int x = tid; x < nq0 * nm1 * nm2; x += NT)
            {
                const int i = x % nq0, rq = x / nq0;
                AE_W1[x] = dot_strided(AE_MODES + rq * nm0, 1, b0 + i, nq0, nm0);
            }
            __syncthreads();
            // forward 1: w2[r][j][i] = sum_q w1[r][q][i] * B1[q][j]
            for (int x = tid; x < n01 * nm2; x += NT)
            {
                const int i = x % nq0, rj = x / nq0, j = rj % nq1, r = rj / nq1;
                AE_W2[x] = dot_strided(AE_W1 + r * nm1 * nq0 + i, nq0, b1 + j, nq1, nm1);
            }
            __syncthreads();
            // forward 2: u[k][j][i] = sum_r w2[r][j][i] * B2[r][k]
            for (int x = tid; x < nqt; x += NT)
            {
                const int ji = x % n01, k = x / n01;
                AE_POINTS[x] = AE_POINT_VALUE(dot_strided(AE_W2 + ji, n01, b2 + k, nq2, nm2));
            }
            __syncthreads();
#undef AE_MODES
#undef AE_W1
#undef AE_W2
#undef AE_POINTS
#undef AE_POINT_VALUE
