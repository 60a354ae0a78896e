// frag/chunk_fetch_first.inc -- request the wave's first chunk of input, one chunk ahead of the loop.
// Expects: IO (the chunk I/O view of the geometry: a SweepGeom, or MassIo for a fused operator); EC, MEMF; in, nelmt; it, lane.
// Declares: AL, st (the staging registers, consumed by frag/chunk_stage.inc, refilled by frag/chunk_fetch_next.inc).
// Slab: untouched.
    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);
