// frag/wave_chunks.inc -- the wave's share of the chunks.  Follows frag/wave_slab.inc.
// Expects: EC, WPB, KMAP, MEMF; nelmt; wib.
// Declares: nchunk, it.  Leaves the kernel when the wave has no chunk.
// Slab: untouched.
    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const ChunkIter it    = chunk_iter<KMAP, WPB, ((MEMF >> 4) & 0xfff)>(nchunk, wib);
    if (it.count == 0)
        return;
