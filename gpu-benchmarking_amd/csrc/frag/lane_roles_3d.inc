// frag/lane_roles_3d.inc -- the three roles of a lane per pass: column (e,j,i) walking k, pencil (e,k,j) over i, pencil
// (e,k,i) over j.  Lanes without a point column (!own) take the roles of the last column: every offset is in bounds.
// Expects: NP, NPASS (point columns per chunk and their passes); NQ, NQ2, NQP; PL, ES (plane and element stride of a
//          point image); lane.
// Declares: own, colp, colo, ecol, bi, bj.
// Slab: untouched.
    static_assert(NP == G::NP && NPASS == G::NPASS && PL == NQ * NQP && ES == NQ * PL, "the point image of HelmGeom");
    bool own[NPASS];
    int colp[NPASS], colo[NPASS], ecol[NPASS], bi[NPASS], bj[NPASS];
#pragma unroll
    for (int s = 0; s < NPASS; ++s)
    {
        const int t  = s * kWave + lane;
        own[s]       = (s + 1) * kWave <= NP || t < NP;
        const int tc = own[s] ? t : NP - 1;
        const int e = tc / NQ2, ab = tc - e * NQ2, a = ab / NQ, b = ab - a * NQ;
        ecol[s] = e;
        colp[s] = ab;                   // (j,i): offset inside a plane of a point array in HBM
        colo[s] = e * ES + a * NQP + b; // (e,j,i): offset of the column's k = 0 point in an image
        bi[s]   = tc * NQP;             // (e,k,j): its i-pencil
        bj[s]   = e * ES + a * PL + b;  // (e,k,i): its j-pencil, stride NQP
    }
