// frag/ring_offsets.inc -- the column offsets of a ring of point planes, every lane's in bounds: lanes without a point
// column and columns whose element lies beyond the batch take the chunk's last valid element.
// Expects: NPASS; ecol, colp (frag/lane_roles_*.inc); evalid (frag/chunk_head.inc).
// Parameters, defined by the kernel just before the #include and undefined here:
//   RING_OFF   the offset arrays this declares, e.g. doff[NPASS], woff[NPASS]
//   RING_SET   the statements that set them for pass s from e, the clamped element of the column
// Slab: untouched.
        int RING_OFF;
#pragma unroll
        for (int s = 0; s < NPASS; ++s)
        {
            const int e = ecol[s] < evalid ? ecol[s] : evalid - 1;
            RING_SET
        }
#undef RING_OFF
#undef RING_SET
