// frag/planes_store.inc -- one point's values of PLANES_N planes that follow one another per element (df, g, grad).
// Expects: T, NQT; e0, ecol, oo (the point's offset in a plane of the chunk, one plane per element); s.
// Parameters, defined by the kernel just before the #include and undefined here:
//   PLANES_DST       the output array
//   PLANES_N         planes per element
//   PLANES_VAL(cc)   the value of plane cc
// Slab: untouched.
                            {
                                T *dst = PLANES_DST + e0 * (PLANES_N * NQT) + ecol[s] * ((PLANES_N - 1) * NQT) + oo;
#pragma unroll
                                for (int cc = 0; cc < PLANES_N; ++cc)
                                    dst[cc * NQT] = PLANES_VAL(cc);
                            }
#undef PLANES_DST
#undef PLANES_N
#undef PLANES_VAL
