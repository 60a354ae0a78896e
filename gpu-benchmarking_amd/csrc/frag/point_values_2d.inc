// frag/point_values_2d.inc -- last forward sweep of a quad, q -> j, into registers, and the two derivatives of u.
// Expects: T, NM, NQ, NQP, NMP, NP, NPASS, BMODE; b1 (nm x nq), d0, d1 (nq x nq); slab, imgU, lane; the lane roles
//          (frag/lane_roles_2d.inc); u[NPASS][NQ] and dreg[NPASS][NQ], declared by the kernel.
// Slab before: w1[(e,i)][q] (frag/forward0.inc).  After: imgU = du_0 (index (e nq + j) NQP + i), fenced.
// Registers of the column's lane (e,i): u = the point values, dreg = du_1, both over j.
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b1);
            }
            wave_lds_fence(); // the forward image is dead: the point image takes its place
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
                if (own[s])
                {
#pragma unroll
                    for (int j = 0; j < NQ; ++j)
                        imgU[colo[s] + j * NQP] = u[s][j];
                }
            wave_lds_fence();
            // du_1[j] = sum_m D1[j][m] u[m] in registers; du_0 over u in the image
            contract_dot<NQ, NQ, NPASS, BMODE>(u, dreg, d1);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgU, bi, own, d0);
