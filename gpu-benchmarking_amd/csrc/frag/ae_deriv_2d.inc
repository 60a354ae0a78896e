// frag/ae_deriv_2d.inc -- the derivatives of one point of an any-extent quad, inside the kernel's loop over its points x.
// Expects: T; x, nq0, nq1; d0, d1 (nq x nq); P0 = the point image of u, complete.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_DU0, AE_DU1   lvalues that take du_0[j][i] = sum_m D0[i][m] u[j][m] and du_1[j][i] = sum_m D1[j][m] u[m][i], each
//                    assigned before the next is computed: an image of P0's region is no place for them
// Declares: i, j.
                const int i = x % nq0, j = x / nq0;
                AE_DU0 = dot_strided(P0 + j * nq0, 1, d0 + i * nq0, 1, nq0);
                AE_DU1 = dot_strided(P0 + i, nq0, d1 + j * nq1, 1, nq1);
#undef AE_DU0
#undef AE_DU1
