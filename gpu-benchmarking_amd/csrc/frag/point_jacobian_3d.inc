// frag/point_jacobian_3d.inc -- J[a][b] = D_b u_a of point k of column s of a hex, gathered behind frag/fields_front_3d.inc.
// Expects: T, G; PL; kept, slab, dk; colo; s, k.
// Declares: o (the point's offset in an image), J.
// Slab: read.
                    const int o     = colo[s] + k * PL;
                    const T J[3][3] = {{kept[G::IMG + o], kept[o], dk[0][s][k]},
                                       {kept[3 * G::IMG + o], kept[2 * G::IMG + o], dk[1][s][k]},
                                       {slab[G::IMG + o], slab[o], dk[2][s][k]}};
