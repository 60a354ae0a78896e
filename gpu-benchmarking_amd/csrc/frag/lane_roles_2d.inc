// frag/lane_roles_2d.inc -- the two roles of a lane per pass: column (e,i) walking j, pencil (e,j) over i.  Lanes
// without a point column (!own) take the roles of the last column: every offset is in bounds.
// Expects: NP, NPASS (point columns per chunk and their passes); NQ, NQP; ES (element stride of the point image); lane.
// Declares: own, colp, colo, ecol, bi.
// Slab: untouched.
    static_assert(NP == G::NP && NPASS == G::NPASS && ES == NQ * NQP, "the point image of HelmGeom");
    bool own[NPASS];
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ, b = tc - e * NQ;
        ecol[s] = e;
        colp[s] = b;          // i: offset inside a row of a point array in HBM
        colo[s] = e * ES + b; // (e,i): offset of the column's j = 0 point in the image, stride NQP
        bi[s]   = tc * NQP;   // (e,j): its i-pencil
    }
