// frag/deriv_transposed_2d.inc -- the transposed derivatives of a quad, right after the walk over j.
// Expects: T, NQ, NPASS, BMODE; d0, d1 (nq x nq); imgU; own, bi (frag/lane_roles_2d.inc); dreg[NPASS][NQ] = the
//          direction-1 term of the column's lane, over j.
// Declares: t1 = D_1^T dreg, over j.
// Slab before: imgU = the direction-0 term, as the walk stored it (not yet fenced).  After: imgU = D_0^T imgU, fenced.
// The kernel then sums its terms per point into u.
            wave_lds_fence();
            T t1[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(dreg, t1, d1);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgU, imgU, bi, own, d0);
