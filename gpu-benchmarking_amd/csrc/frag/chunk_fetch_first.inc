// frag/chunk_fetch_first.inc -- request the wave's first chunk of modes, one chunk ahead of the loop.
// Expects: IO (MassIo view of the geometry); EC, MEMF; in, nelmt; it, lane.
// Declares: AL, st (the staging registers, consumed by frag/chunk_stage.inc, refilled by frag/chunk_fetch_next.inc).
// Slab: untouched.
    constexpr bool AL = (MEMF & 4) && IO::ALIGN_OK;
    typename IO::Vec st[IO::NLD];
    chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, it.first, nelmt, lane);
