// frag/wave_one_chunk.inc -- the whole input side of a kernel whose short-lived waves take ONE chunk each: no chunk loop,
// no prefetch.  Follows frag/wave_slab.inc.
// Expects: T; G (a SweepGeom); EC, WPB, XG; in, nelmt; slab, lane, wib.
// Declares: nchunk, c (the wave's chunk; leaves the kernel when the batch has none for it), left, evalid
//           (frag/chunk_head.inc), st.
// Slab after: the input image of chunk c, fenced.
    const uint64_t nchunk = (nelmt + EC - 1) / EC;
    const uint64_t c      = logical_block<XG>() * WPB + wib;
    if (c >= nchunk)
        return;
#include "chunk_head.inc"
    typename G::Vec st[G::NLD];
    chunk_fetch<G, EC, true, false>(st, in, c, nelmt, lane);
    chunk_stage<G, false>(st, slab, lane, G::VEC2 ? 0 : line_offset<T>(in + c * G::IN_DBL));
    wave_lds_fence();
