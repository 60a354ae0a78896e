// frag/chunk_fetch_next.inc -- request the wave's next chunk of input: in flight under this chunk's sweeps.
// Expects: IO, AL, st; EC, MEMF; in, nelmt; it, n, c, lane.
// Slab: untouched.
        if (n + 1 < it.count)
            chunk_fetch<IO, EC, !(MEMF & 1), AL>(st, in, c + it.step, nelmt, lane);
