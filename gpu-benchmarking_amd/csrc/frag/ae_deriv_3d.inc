// frag/ae_deriv_3d.inc -- the derivatives of one point of an any-extent hex, inside the kernel's loop over its points x.
// Expects: T; x, nq0, nq1, nq2, n01; d0, d1, d2 (nq x nq); P0 = the point image of u, complete.
// Parameters, defined by the kernel just before the #include and undefined here:
//   AE_DU0, AE_DU1, AE_DU2   lvalues that take D0 u along i, D1 u along j, D2 u along k, of the point, each assigned
//                            before the next is computed: an image of P0's region is no place for them
// Declares: i, j, k, kj.
                const int i = x % nq0, kj = x / nq0, j = kj % nq1, k = kj / nq1;
                AE_DU0 = dot_strided(P0 + kj * nq0, 1, d0 + i * nq0, 1, nq0);
                AE_DU1 = dot_strided(P0 + k * n01 + i, nq0, d1 + j * nq1, 1, nq1);
                AE_DU2 = dot_strided(P0 + j * nq0 + i, n01, d2 + k * nq2, 1, nq2);
#undef AE_DU0
#undef AE_DU1
#undef AE_DU2
