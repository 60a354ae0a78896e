// frag/chunk_stage.inc -- the staging registers of chunk c go into the slab.
// Expects: IO, AL, st (frag/chunk_fetch_first.inc); T, in, c, slab, lane.
// Slab before: dead (the previous chunk has been flushed or stored).  After: the input image, IO::IN_DBL scalars per chunk (nm^d modes per element; IProductWRTBase: nq^d points),
// fenced; st is free again.  The kernel requests its own streams next, then includes frag/chunk_fetch_next.inc.
        chunk_stage<IO, AL>(st, slab, lane,
                            IO::VEC2 ? (AL ? align_shift(in + c * IO::IN_DBL) : 0) : line_offset<T>(in + c * IO::IN_DBL));
        wave_lds_fence();
