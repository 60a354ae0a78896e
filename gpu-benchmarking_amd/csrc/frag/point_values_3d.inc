// frag/point_values_3d.inc -- last forward sweep of a hex, r -> k, into registers, and the three derivatives of u.
// Expects: T, NM, NQ, NQP, NMP, NP, NPASS, PL, BMODE; b2 (nm x nq), d0, d1, d2 (nq x nq); slab, imgU, imgD, lane; the
//          lane roles (frag/lane_roles_3d.inc); u[NPASS][NQ] and dreg[NPASS][NQ], declared by the kernel.
// Slab before: w2[(e,j,i)][r] (frag/forward1_3d.inc).  After: imgD = du_0, imgU = du_1 (index ((e nq + k) nq + j) NQP
// + i), fenced.  Registers of the column's lane (e,j,i): u = the point values, dreg = du_2, both over k.
            {
                T m[NPASS][NM];
                read_pencils<NM, NPASS, NP, NMP>(m, slab, lane);
                contract<NM, NQ, NPASS, BMODE>(m, u, b2);
            }
            wave_lds_fence(); // the forward images are dead: the point images take their place
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
                if (own[s])
                {
#pragma unroll
                    for (int k = 0; k < NQ; ++k)
                        imgU[colo[s] + k * PL] = u[s][k];
                }
            wave_lds_fence();
            // du_2[k] = sum_m D2[k][m] u[m] in registers; du_0 into imgD; du_1 over u in imgU
            contract_dot<NQ, NQ, NPASS, BMODE>(u, dreg, d2);
            image_sweep<NQ, NPASS, 1, BMODE, true>(imgU, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, true>(imgU, imgU, bj, own, d1);
