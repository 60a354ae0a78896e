// frag/wave_open.inc -- the opening of a wave kernel over several fields (geom, advect, affine_advect, vecgrad): the names
// of the geometry, the slab with its kept images, the wave's chunks, the lane roles and the request of the first chunk.
// The first lines of the kernel body, behind `using G = ...` and the constants that are the kernel's own.
// Expects: T, NQ, EC, WPB, KMAP, MEMF; G (a HelmGeom or a GeomGeom); x0 (the modes of field 0), nelmt.
// Parameters, defined by the kernel just before the #include and undefined here:
//   OPEN_DIM         2 or 3
//   OPEN_KEPT_BASE   where the kept images start in the slab (G::KEPT_BASE; 0 for a kernel that keeps none)
//   OPEN_LANE_SETUP  the statements between the lane roles and the first request: the lane's constants of its columns
//                    (affine_advect's weight product; behind the request it changes the assembly); may be empty
// Declares: M, F, IO; NM, NMP, NQP, NQT, NPASS, NP, ES (3D: NQ2, PL too); what wave_slab, wave_chunks, lane_roles_{2d,3d}
//           and chunk_fetch_first declare; kept; in = x0, the stream the fragments fetch and stage.
// Slab: untouched.
    using M          = typename G::M;
    using F          = typename G::F;
    using IO         = MassIo<M>;
#if OPEN_DIM == 3
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQ2 = NQ * NQ, NQT = NQ2 * NQ;
    constexpr int PL = NQ * NQP, ES = NQ * PL; // plane and element stride of a point image
#else
    constexpr int NM = G::NM, NMP = F::NMP, NQP = G::NQP, NQT = NQ * NQ;
    constexpr int ES = NQ * NQP; // element stride of the point image
#endif
    constexpr int NPASS = G::NPASS, NP = G::NP;
    static_assert(KMAP > 0, "short-lived waves only");

#include "wave_slab.inc"
    T *kept = slab + OPEN_KEPT_BASE; // the images of the fields 0 .. d-2, two per field in 3D, one in 2D
#include "wave_chunks.inc"
#if OPEN_DIM == 3
#include "lane_roles_3d.inc"
#else
#include "lane_roles_2d.inc"
#endif
    OPEN_LANE_SETUP
    const T *in = x0; // the field at hand
#include "chunk_fetch_first.inc"
#undef OPEN_DIM
#undef OPEN_KEPT_BASE
#undef OPEN_LANE_SETUP
