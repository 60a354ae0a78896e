// frag/deriv_transposed_3d.inc -- the transposed derivatives of a hex, right after the walk over k.
// Expects: T, NQ, NQP, NPASS, BMODE; d0, d1, d2 (nq x nq); imgU, imgD; own, bi, bj (frag/lane_roles_3d.inc);
//          dreg[NPASS][NQ] = the direction-2 term of the column's lane, over k.
// Declares: t2 = D_2^T dreg, over k.
// Slab before: imgD = the direction-0 term, imgU = the direction-1 term, as the walk stored them (not yet fenced).
// After: imgD = D_0^T imgD, imgU = D_1^T imgU, fenced.  The kernel then sums its terms per point into u.
            wave_lds_fence();
            // D_2^T in registers (contract(): the summed index is the row of deriv2), D_0^T and D_1^T in place
            T t2[NPASS][NQ];
            contract<NQ, NQ, NPASS, BMODE>(dreg, t2, d2);
            image_sweep<NQ, NPASS, 1, BMODE, false>(imgD, imgD, bi, own, d0);
            image_sweep<NQ, NPASS, NQP, BMODE, false>(imgU, imgU, bj, own, d1);
