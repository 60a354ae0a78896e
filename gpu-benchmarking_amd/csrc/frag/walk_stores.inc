// frag/walk_stores.inc -- what the stores of a walk over the point columns start from.  First lines of the walk's block.
// Expects: EC, NPASS, NQT; c; own, ecol, colp (frag/lane_roles_*.inc); evalid (frag/chunk_head.inc).
// Declares: e0 (the chunk's first element); put[s] (this lane stores: it has a point column and the column's element is
//           in the batch); ooff[s] (the column's offset in a plane of the chunk, one plane per element).
// Slab: untouched.
            const uint64_t e0 = c * (uint64_t)EC;
            bool put[NPASS];
            int ooff[NPASS];
#pragma unroll
            for (int s = 0; s < NPASS; ++s)
            {
                put[s]  = own[s] && ecol[s] < evalid;
                ooff[s] = ecol[s] * NQT + colp[s];
            }
