// frag/chunk_head.inc -- first lines of the chunk loop `for (n ...; c += it.step)`: how much of chunk c is in the batch.
// Expects: EC, nelmt, c.
// Declares: left, evalid (1 .. EC elements of this chunk exist; only the batch's last chunk has fewer than EC).
// Slab: untouched.
        const uint64_t left = nelmt - c * EC;
        const int evalid    = left >= EC ? EC : (int)left;
