// frag/ae_deriv_transposed_3d.inc -- the transposed derivatives of one point of an any-extent hex, inside the kernel's
// loop over its points x.
// Expects: T; x, nq0, nq1, nq2, n01; d0, d1, d2 (nq x nq); P1, P2, P3 = the point images of the three terms, complete.
// Declares: i, j, k, kj; t0 = D_0^T P1, t1 = D_1^T P2, t2 = D_2^T P3, of the point.  The kernel sums them.
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                const T t0 = dot_strided(P1 + kj * nq0, 1, d0 + i, nq0, nq0);
                const T t1 = dot_strided(P2 + k * n01 + i, nq0, d1 + j, nq1, nq1);
                const T t2 = dot_strided(P3 + j * nq0 + i, n01, d2 + k, nq2, nq2);
