// frag/point_jacobian_2d.inc -- J[a][b] = D_b u_a of point j of column s of a quad, gathered behind frag/fields_front_2d.inc.
// Expects: T; NQP; kept, slab, dk; colo; s, j.
// Declares: o (the point's offset in an image), J.
// Slab: read.
                    const int o     = colo[s] + j * NQP;
                    const T J[2][2] = {{kept[o], dk[0][s][j]}, {slab[o], dk[1][s][j]}};
