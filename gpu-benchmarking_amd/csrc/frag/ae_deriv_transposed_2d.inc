// frag/ae_deriv_transposed_2d.inc -- the transposed derivatives of one point of an any-extent quad, inside the kernel's
// loop over its points x.
// Expects: T; x, nq0, nq1; d0, d1 (nq x nq); P1, P2 = the point images of the direction-0 and direction-1 terms, complete.
// Declares: i, j; t0 = D_0^T P1, t1 = D_1^T P2, of the point.  The kernel sums them.
                const int i = x % nq0, j = x / nq0;
                const T t0 = dot_strided(P1 + j * nq0, 1, d0 + i, nq0, nq0);
                const T t1 = dot_strided(P2 + i, nq0, d1 + j, nq1, nq1);
