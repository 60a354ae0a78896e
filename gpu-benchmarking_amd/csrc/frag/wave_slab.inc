// frag/wave_slab.inc -- the wave's slab.  Kernel-body text, included first; a kernel that keeps point images names
// them (imgU, imgD) right after it.
// Expects: T; G (G::SLAB = scalars of LDS per wave).
// Declares: lds_raw, lane, wib, slab.
// Slab: untouched.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib  = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *slab        = reinterpret_cast<T *>(lds_raw) + wib * G::SLAB;
