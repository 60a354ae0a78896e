// frag/ae_prologue.inc -- the element constants of an any-extent kernel, at the top of the kernel body.
// Expects: DIM; nq0, nq1, nq2.
// Declares: nm0, nm1, nm2 (2D: 1), nz (2D: 1), n01, nqt, nmt, tid -- the names every frag/ae_*.inc takes from the scope.
    const int nm0 = nq0 - 1, nm1 = nq1 - 1, nm2 = DIM == 3 ? nq2 - 1 : 1;
    const int nz  = DIM == 3 ? nq2 : 1;
    const int n01 = nq0 * nq1;
    const int nqt = n01 * nz;        // points per element
    const int nmt = nm0 * nm1 * nm2; // modes per element
    const int tid = threadIdx.x;
