// capi.hip -- the extern "C" boundary of libsumfact.so (declared in include/sumfact.h).
// Validation + dispatch only, no kernels: every operator entry point forwards to one template <int DIM, typename T>
// function below, which declares its operands (Operands), has them checked in the documented order (check()), builds the
// args structs and routes to the launchers that sf_dispatch.h and the *_args.h headers declare.  DESIGN.md lists which
// translation unit holds which kernels.
#include "advect_args.h"
#include "affine_advect_args.h"
#include "geom_args.h"
#include "sf_dispatch.h"
#include "vecgrad_args.h"

#include <cassert>
#include <cstdio>
#include <cstring>
#include <initializer_list>


using namespace sf;

static inline bool aligned(const void *p, size_t a)
{
    return ((uintptr_t)p & (a - 1)) == 0;
}

// byte ranges [p, p + np) and [q, q + nq) share a byte
static inline bool overlaps(const void *p, size_t np, const void *q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

// ---- the operands of a call and the one check of them ----------------------------------------------------------------
// What an operand is to the check, OR-ed together.
enum : unsigned
{
    kIn  = 1u << 0, // the call reads it
    kOut = 1u << 1, // the call writes it: it may lie over no kGuard operand and over no other output
    // Outputs may not lie over this one.  The families with an overlap rule guard what they read per element (in, x, c, w,
    // g, df and the per-element constants) and sf_diag_helmholtz_* its tables.  Bases, derivative matrices and
    // quadrature weights are guarded by sf_vecgrad_* alone (bases and derivative matrices): elsewhere an output over
    // one of them goes through to the launch.  That difference came with the family, nobody decided it; it is kept as
    // it is here, because unifying it changes what a caller sees.  sf_bwdtrans_* and sf_iproduct_* guard nothing.
    kGuard  = 1u << 2,
    kStream = 1u << 3, // a 16-byte stream of the wave kernels: its address enters the bits that route() tests
    kAbsent = 1u << 4, // a null that the call documents as "not looked at": no step of the check sees it
};

struct Operand
{
    const void *p;
    size_t bytes; // what the call touches from p on
    unsigned role;
};
constexpr int kMaxOperands = 20; // sf_aff_advect_hex_*: three each of basis, deriv, qw, c, in, out, and dfe, je

// Steps (1)-(4) of the validation order documented in include/sumfact.h, before any HIP call: the extents / variant range
// (SF_EINVAL), an empty batch (SF_OK), a null among the operands that are present or a refused value (SF_EINVAL), an
// operand that is not aligned to the scalar (SF_EALIGN).  kProceed: none of these, the caller goes on.
constexpr int kProceed = 1 << 30; // neither an SF_* code nor a hipError_t
static int check_present(bool range_ok, size_t nelmt, const Operand *ops, int n, size_t scalar, bool values_ok)
{
    if (!range_ok)
        return SF_EINVAL;
    if (nelmt == 0)
        return SF_OK;
    for (int i = 0; i < n; ++i)
        if (!(ops[i].role & kAbsent) && !ops[i].p)
            return SF_EINVAL;
    if (!values_ok)
        return SF_EINVAL;
    for (int i = 0; i < n; ++i)
        if (!(ops[i].role & kAbsent) && !aligned(ops[i].p, scalar))
            return SF_EALIGN;
    return kProceed;
}

// Step (5): every output against every guarded operand and every earlier output, as byte ranges (SF_EINVAL).
static int check_disjoint(const Operand *ops, int n)
{
    for (int i = 0; i < n; ++i)
    {
        if ((ops[i].role & (kOut | kAbsent)) != kOut)
            continue;
        for (int j = 0; j < n; ++j)
        {
            const unsigned r = ops[j].role;
            if (!(r & kAbsent) && ((r & kGuard) || ((r & kOut) && j < i)) &&
                overlaps(ops[i].p, ops[i].bytes, ops[j].p, ops[j].bytes))
                return SF_EINVAL;
        }
    }
    return kProceed;
}

// Steps (1)-(5).  On kProceed `streams` is the OR of the addresses of the kStream operands that are present: 16-byte
// aligned exactly when every one of them is, which is what route() asks of its `in` and `out`.
static int check(bool range_ok, size_t nelmt, const Operand *ops, int n, size_t scalar, bool values_ok, const void *&streams)
{
    int rc = check_present(range_ok, nelmt, ops, n, scalar, values_ok);
    if (rc == kProceed)
        rc = check_disjoint(ops, n);
    if (rc != kProceed)
        return rc;
    uintptr_t bits = 0;
    for (int i = 0; i < n; ++i)
        if ((ops[i].role & (kStream | kAbsent)) == kStream)
            bits |= (uintptr_t)ops[i].p;
    streams = (const void *)bits;
    return kProceed;
}

// Steps (1)-(4) for the calls that pass bare pointers, all of them required (sf_bwdtrans_hex_f64_mfma4,
// sf_bwdtrans_specialised).  A pointer the call does not take (the third basis in 2D) is passed as one that it does.
static int validate(bool range_ok, size_t nelmt, std::initializer_list<const void *> ptrs, size_t align)
{
    Operand ops[kMaxOperands];
    int n = 0;
    for (const void *p : ptrs)
        ops[n++] = {p, 0, kIn};
    return check_present(range_ok, nelmt, ops, n, align, true);
}

// The operand list of one call, on the stack, with the byte lengths its entries are written in: over the batch, one
// scalar per element (`elmt`), one field of modes (`modes`), one field of quadrature points (`points`).
template <int DIM, typename T> struct Operands
{
    const unsigned (&nq)[3];
    const size_t nelmt, elmt, modes, points;
    Operand v[kMaxOperands];
    int n               = 0;
    const void *streams = nullptr; // set by check(): what route() takes as `in` and as `out`

    Operands(const unsigned (&nq_)[3], size_t nelmt_)
        : nq(nq_), nelmt(nelmt_), elmt(sizeof(T) * nelmt_),
          modes(sizeof(T) * nelmt_ * (nq_[0] - 1) * (nq_[1] - 1) * (DIM == 3 ? nq_[2] - 1 : 1)),
          points(sizeof(T) * nelmt_ * nq_[0] * nq_[1] * (DIM == 3 ? nq_[2] : 1))
    {
    }
    void add(const void *p, size_t bytes, unsigned role)
    {
        assert(n < kMaxOperands);
        v[n++] = {p, bytes, role};
    }
    // an operand the call looks at only on a condition it documents
    void add_if(bool looked_at, const void *p, size_t bytes, unsigned role)
    {
        add(p, bytes, looked_at ? role : role | kAbsent);
    }
    // one operand per direction, the first `count` of them looked at
    template <typename P> void each(P *const (&p)[3], size_t bytes, unsigned role, unsigned count = DIM)
    {
        for (unsigned a = 0; a < (unsigned)DIM; ++a)
            add_if(a < count, p[a], bytes, role);
    }
    void bases(const T *const (&b)[3], unsigned role = kIn) // nm x nq per direction
    {
        for (int a = 0; a < DIM; ++a)
            add(b[a], sizeof(T) * (nq[a] - 1) * nq[a], role);
    }
    void matrices(const T *const (&b)[3], const T *const (&d)[3], unsigned role = kIn) // the bases, then nq x nq per direction
    {
        bases(b, role);
        for (int a = 0; a < DIM; ++a)
            add(d[a], sizeof(T) * nq[a] * nq[a], role);
    }
    void weights(const T *const (&qw)[3], bool looked_at = true) // the nq one-dimensional quadrature weights per direction
    {
        for (int a = 0; a < DIM; ++a)
            add_if(looked_at, qw[a], sizeof(T) * nq[a], kIn);
    }
    int check(bool range_ok, bool values_ok = true)
    {
        return ::check(range_ok, nelmt, v, n, sizeof(T), values_ok, streams);
    }
};

template <int DIM> static bool range_ok(int variant, const unsigned (&nq)[3])
{
    return nq[0] >= 2 && nq[1] >= 2 && (DIM == 2 || nq[2] >= 2) && variant >= 0 && variant < SF_NUM_VARIANTS;
}

template <int DIM, typename T>
static ArgsT<DIM, T> make_args(const T *const (&b)[3], const T *in, T *wsp, T *out, size_t nelmt)
{
    if constexpr (DIM == 3)
        return {b[0], b[1], b[2], in, wsp, out, (uint64_t)nelmt};
    else
        return {b[0], b[1], in, wsp, out, (uint64_t)nelmt};
}

// The shared tail of sf_iproduct_*, sf_mass_*, sf_helmholtz_*, sf_affine_helmholtz_*, sf_physderiv_*, sf_iprodderiv_* and their affine forms: AUTO takes the wave kernel for an isotropic order of
// its table (`wave_built`) when in / out are 16-byte aligned, and the any-extent kernel otherwise.
template <int DIM, class Wave, class Generic>
static int route(int variant, const unsigned (&nq)[3], bool generic_built, bool wave_built, const void *in,
                 const void *out, Wave wave, Generic generic)
{
    if (!generic_built)
        return SF_ENOTBUILT;
    if (variant != SF_VARIANT_AUTO && variant != SF_VARIANT_WAVE && variant != SF_VARIANT_GENERIC)
        return SF_ENOTBUILT;
    const bool wave_ok = nq[0] == nq[1] && (DIM == 2 || nq[1] == nq[2]) && wave_built;
    const bool vec_ok  = aligned(in, 16) && aligned(out, 16);
    if (variant == SF_VARIANT_WAVE)
    {
        if (!wave_ok)
            return SF_ENOTBUILT;
        return vec_ok ? wave() : SF_EALIGN;
    }
    if (variant == SF_VARIANT_AUTO && wave_ok && vec_ok)
        return wave();
    return generic();
}

// ---- BwdTrans: one validation and routing for both dimensions and both scalar types ----------------------------------
// The wave and matrix-core kernels read `in` and write `out` with 16-byte lanes (`vec_ok`) and are built for isotropic
// extents (`iso`), 3D also for the anisotropic triples of bwdtrans_rt.hip.  The fp32 entry points pass SF_VARIANT_AUTO.
template <int DIM, typename T>
static int bwdtrans(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *in, T *wsp, T *out,
                    void *stream)
{
    Operands<DIM, T> o(nq, nelmt); // no overlap rule: nothing is guarded
    o.bases(b);
    o.add(in, o.modes, kIn | kStream);
    o.add(out, o.points, kOut | kStream);
    const int pre = o.check(range_ok<DIM>(variant, nq));
    if (pre != kProceed)
        return pre;
    constexpr bool f64 = std::is_same<T, double>::value, hex64 = DIM == 3 && f64;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, wsp, out, nelmt);
    const bool iso      = nq[0] == nq[1] && (DIM == 2 || nq[1] == nq[2]);
    const bool vec_ok   = aligned(in, 16) && aligned(out, 16);
    auto wave3          = [&] {
        if constexpr (hex64)
            return launch_hex_wave3(nq[0], nq[1], nq[2], a, s);
        else
            return (int)SF_ENOTBUILT;
    };
    auto wave_rt = [&] {
        if constexpr (hex64)
            return launch_hex_rt(nq[0], nq[1], nq[2], a, s);
        else
            return (int)SF_ENOTBUILT;
    };
    if (variant == SF_VARIANT_AUTO)
    {
        // the first leg that answers something other than SF_ENOTBUILT
        int rc   = SF_ENOTBUILT;
        auto leg = [&](bool applies, auto launch) {
            if (rc == SF_ENOTBUILT && applies)
                rc = launch();
        };
        leg(iso && vec_ok, [&] { return launch_bwd_iso_auto<DIM, T>(nq[0], a, s); }); // the order's table
        leg(!iso && vec_ok, wave3);                                                   // compile-time triples
        leg(vec_ok, [&] { // a specialisation the caller made ready (sf_specialise)
            return launch_specialised(DIM, nq[0], nq[1], nq[2], (int)sizeof(T), b[0], b[1], b[2], in, out, a.nelmt, s);
        });
        // the run-time-extent wave kernel (bwdtrans_rt.h), also for buffers that are only 8-byte aligned: ahead of the
        // block kernel up to nq = 8 per direction (0.39-0.52 of the roofline against 0.28-0.34; above that its
        // unrolled-to-the-bound loops lose: profiles/r03/anisotropic_shapes.log)
        leg(nq[0] <= 8 && nq[1] <= 8 && nq[2] <= 8, wave_rt);
        leg(true, [&] { return launch_bwd_generic<DIM, T>(SF_VARIANT_GENERIC, nq, a, s); });
        return rc;
    }
    if constexpr (f64)
    {
        // an explicit vector variant: off its table, then 8-byte-aligned buffers, then the launch
        auto run = [&](bool built, auto launch) {
            return !built ? (int)SF_ENOTBUILT : (!vec_ok ? (int)SF_EALIGN : launch());
        };
        switch (variant)
        {
        case SF_VARIANT_WAVE: // 3D: the triple table answers for anisotropic extents at launch, after the alignment
            return run(iso || hex64, [&] { return iso ? launch_bwd_wave<DIM, T>(nq[0], a, s) : wave3(); });
        case SF_VARIANT_MFMA: return run(iso, [&] { return launch_bwd_mfma<DIM, T>(nq[0], a, s); });
        case SF_VARIANT_MFMA4: return run(iso, [&] { return launch_bwd_mfma4<DIM, T>(nq[0], a, s); });
        case SF_VARIANT_WAVE_RT: return wave_rt();
        case SF_VARIANT_GENERIC:
        case SF_VARIANT_THREAD:
        case SF_VARIANT_BLOCK_LDS:
        case SF_VARIANT_BLOCK_GLB: return launch_bwd_generic<DIM, T>(variant, nq, a, s);
        default: break;
        }
    }
    return SF_ENOTBUILT;
}

// ---- the operator families: each declares its operands, has them checked, builds its args and routes ------------------
// Where a family reads "not in-place safe": the word-grid loads of a chunk read 16-byte words that straddle the
// neighbouring element, so an output may not lie over what the call reads per element.

// ---- IProductWRTBase --------------------------------------------------------------------------------------------------
template <int DIM, typename T>
static int iprod(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *in, T *out,
                 void *stream)
{
    Operands<DIM, T> o(nq, nelmt); // no overlap rule: nothing is guarded
    o.bases(b);
    o.add(in, o.points, kIn | kStream);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, out, nelmt);
    return route<DIM>(
        variant, nq, iprod_generic_built(DIM, nq[0], nq[1], nq[2]), iprod_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_iprod_wave<DIM, T>(nq[0], a, s); }, [&] { return launch_iprod_generic<DIM, T>(nq, a, s); });
}

// ---- the tensor-product apply with independent input / output extents (sf_tensor_*) -----------------------------------
// Its own order: steps (1)-(4), then tensor_generic_built, and only then the overlap of out and in, because the byte
// lengths below can overflow for extents that the fallback does not take.  AUTO on 16-byte-aligned in / out: the compiled
// table, then a specialisation the caller made ready (sf_specialise_tensor), then the any-extent kernel, which also
// takes buffers aligned only to the scalar.
template <int DIM, typename T>
static int tensor(int variant, const unsigned (&ni)[3], const unsigned (&no)[3], int trans, size_t nelmt,
                  const T *const (&m)[3], const T *in, T *out, void *stream)
{
    bool range = (trans == 0 || trans == 1) && variant >= 0 && variant < SF_NUM_VARIANTS;
    for (int d = 0; d < DIM; ++d)
        range = range && ni[d] >= 1 && no[d] >= 1;
    const Operand ops[5] = {
        {m[0], sizeof(T) * ni[0] * no[0], kIn},
        {m[1], sizeof(T) * ni[1] * no[1], kIn},
        {m[2], sizeof(T) * ni[2] * no[2], DIM == 3 ? kIn : kIn | kAbsent},
        {in, sizeof(T) * nelmt * ni[0] * ni[1] * (DIM == 3 ? ni[2] : 1), kIn | kGuard}, // not in-place safe
        {out, sizeof(T) * nelmt * no[0] * no[1] * (DIM == 3 ? no[2] : 1), kOut},
    };
    const int rc = check_present(range, nelmt, ops, 5, sizeof(T), true);
    if (rc != kProceed)
        return rc;
    if (!tensor_generic_built(DIM, ni, no)) // bounds the extents: the byte lengths above mean something from here on
        return SF_ENOTBUILT;
    if (check_disjoint(ops, 5) != kProceed)
        return SF_EINVAL;
    if (variant != SF_VARIANT_AUTO && variant != SF_VARIANT_WAVE && variant != SF_VARIANT_GENERIC)
        return SF_ENOTBUILT;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(m, in, nullptr, out, nelmt);
    const bool vec_ok   = aligned(in, 16) && aligned(out, 16);
    const bool table    = tensor_wave_built(DIM, ni, no);
    if (variant == SF_VARIANT_WAVE)
        return !table ? (int)SF_ENOTBUILT : (!vec_ok ? (int)SF_EALIGN : launch_tensor_wave<DIM, T>(ni, no, trans, a, s));
    if (variant == SF_VARIANT_AUTO && vec_ok)
    {
        if (table)
            return launch_tensor_wave<DIM, T>(ni, no, trans, a, s);
        const int spec = launch_tensor_specialised(DIM, ni, no, trans, (int)sizeof(T), m[0], m[1], m[2], in, out, a.nelmt, s);
        if (spec != SF_ENOTBUILT)
            return spec;
    }
    return launch_tensor_generic<DIM, T>(ni, no, trans, a, s);
}

// ---- the fused mass operator B^T diag(w) B ------------------------------------------------------------------------------
template <int DIM, typename T>
static int mass(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *w, const T *in,
                T *out, void *stream)
{
    Operands<DIM, T> o(nq, nelmt); // not in-place safe
    o.bases(b);
    o.add(w, o.points, kIn | kGuard);
    o.add(in, o.modes, kIn | kGuard | kStream);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, out, nelmt);
    return route<DIM>(
        variant, nq, mass_generic_built(DIM, nq[0], nq[1], nq[2]), mass_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_mass_wave<DIM, T>(nq[0], a, w, s); },
        [&] { return launch_mass_generic<DIM, T>(nq, a, w, s); });
}

// ---- the fused Helmholtz operator ----------------------------------------------------------------------------------------
// `w` is looked at only when lambda != 0; a lambda that is not finite is the refused value.
template <int DIM, typename T>
static int helmholtz(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                     const T *g, const T *w, double lambda, const T *in, T *out, void *stream)
{
    const bool has_w = lambda != 0.0; // false for NaN too, which is refused with the nulls
    Operands<DIM, T> o(nq, nelmt);    // not in-place safe
    o.matrices(b, d);
    o.add(g, DIM * (DIM + 1) / 2 * o.points, kIn | kGuard);
    o.add_if(has_w, w, o.points, kIn | kGuard);
    o.add(in, o.modes, kIn | kGuard | kStream);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq), lambda - lambda == 0.0);
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, out, nelmt);
    const HelmArgsT<T> x{d[0], d[1], d[2], g, has_w ? w : nullptr, (T)lambda}; // lambda is rounded to T here, once
    return route<DIM>(
        variant, nq, helmholtz_generic_built(DIM, nq[0], nq[1], nq[2]), helmholtz_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_helmholtz_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_helmholtz_generic<DIM, T>(nq, a, x, s); });
}

// ---- the fused Helmholtz operator on affine elements ----------------------------------------------------------------------
// sf_helmholtz_* with the quadrature weights and ge in the place of g and je in the place of w: `je` is looked at only
// when lambda != 0.
template <int DIM, typename T>
static int affine(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                  const T *const (&qw)[3], const T *ge, const T *je, double lambda, const T *in, T *out, void *stream)
{
    const bool has_j = lambda != 0.0; // false for NaN too, which is refused with the nulls
    Operands<DIM, T> o(nq, nelmt);    // not in-place safe
    o.matrices(b, d);
    o.weights(qw);
    o.add(ge, DIM * (DIM + 1) / 2 * o.elmt, kIn | kGuard);
    o.add_if(has_j, je, o.elmt, kIn | kGuard);
    o.add(in, o.modes, kIn | kGuard | kStream);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq), lambda - lambda == 0.0);
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, out, nelmt);
    // lambda is rounded to T here, once
    const AffineArgsT<T> x{d[0], d[1], d[2], qw[0], qw[1], qw[2], ge, has_j ? je : nullptr, (T)lambda};
    return route<DIM>(
        variant, nq, affine_generic_built(DIM, nq[0], nq[1], nq[2]), affine_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_affine_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_affine_generic<DIM, T>(nq, a, x, s); });
}

// ---- BwdTrans fused with the physical-space gradient ------------------------------------------------------------------------
// df is looked at only when it is not null; DIM outputs of nq^d points per element each.
template <int DIM, typename T>
static int physderiv(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                     const T *df, const T *in, T *const (&out)[3], void *stream)
{
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.add_if(df != nullptr, df, DIM * DIM * o.points, kIn | kGuard);
    o.add(in, o.modes, kIn | kGuard | kStream);
    o.each(out, o.points, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, nullptr, nelmt);
    const PhysDerivArgsT<T> x{d[0], d[1], d[2], df, out[0], out[1], out[2]};
    return route<DIM>(
        variant, nq, physderiv_generic_built(DIM, nq[0], nq[1], nq[2]), physderiv_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_physderiv_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_physderiv_generic<DIM, T>(nq, a, x, s); });
}

// ---- IProductWRTDerivBase, the transpose of the gradient ----------------------------------------------------------------
// DIM inputs of nq^d points per element each; df and w are each looked at only when not null.  Only `out` is a 16-byte
// stream of the wave kernels.
template <int DIM, typename T>
static int iprodderiv(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                      const T *df, const T *w, const T *const (&in)[3], T *out, void *stream)
{
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.add_if(df != nullptr, df, DIM * DIM * o.points, kIn | kGuard);
    o.add_if(w != nullptr, w, o.points, kIn | kGuard);
    o.each(in, o.points, kIn | kGuard);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, out, nelmt);
    const IprodDerivArgsT<T> x{d[0], d[1], d[2], df, w, in[0], in[1], in[2]};
    return route<DIM>(
        variant, nq, iprodderiv_generic_built(DIM, nq[0], nq[1], nq[2]), iprodderiv_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_iprodderiv_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_iprodderiv_generic<DIM, T>(nq, a, x, s); });
}

// ---- the gradient on affine elements -------------------------------------------------------------------------------------
// sf_physderiv_* with the d*d constants per element dfe in the place of df; dfe is required.
template <int DIM, typename T>
static int affine_physderiv(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3],
                            const T *const (&d)[3], const T *dfe, const T *in, T *const (&out)[3], void *stream)
{
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.add(dfe, DIM * DIM * o.elmt, kIn | kGuard);
    o.add(in, o.modes, kIn | kGuard | kStream);
    o.each(out, o.points, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, in, nullptr, nullptr, nelmt);
    const AffinePhysDerivArgsT<T> x{d[0], d[1], d[2], dfe, out[0], out[1], out[2]};
    return route<DIM>(
        variant, nq, affine_deriv_generic_built(DIM, nq[0], nq[1], nq[2]), affine_deriv_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_affine_physderiv_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_affine_physderiv_generic<DIM, T>(nq, a, x, s); });
}

// ---- the weak divergence on affine elements --------------------------------------------------------------------------------
// sf_iprodderiv_* with dfe (required) in the place of df and the quadrature weights and je in the place of w: `je` and
// every `qw` are looked at only when je is not null.  Only `out` is a 16-byte stream of the wave kernels.
template <int DIM, typename T>
static int affine_iprodderiv(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3],
                             const T *const (&d)[3], const T *const (&qw)[3], const T *dfe, const T *je,
                             const T *const (&in)[3], T *out, void *stream)
{
    const bool has_w = je != nullptr;
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.weights(qw, has_w);
    o.add(dfe, DIM * DIM * o.elmt, kIn | kGuard);
    o.add_if(has_w, je, o.elmt, kIn | kGuard);
    o.each(in, o.points, kIn | kGuard);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, out, nelmt);
    const AffineIprodDerivArgsT<T> x{d[0],  d[1], d[2], has_w ? qw[0] : nullptr, has_w ? qw[1] : nullptr,
                                     has_w ? qw[2] : nullptr, dfe, je, in[0], in[1], in[2]};
    return route<DIM>(
        variant, nq, affine_deriv_generic_built(DIM, nq[0], nq[1], nq[2]), affine_deriv_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_affine_iprodderiv_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_affine_iprodderiv_generic<DIM, T>(nq, a, x, s); });
}

// ---- the diagonal of the fused Helmholtz operator ------------------------------------------------------------------------
// sf_helmholtz_* without `in`: the table triples of sf_diag_tables_* stand where the bases do (and are guarded), `w` is
// looked at only when lambda != 0, `out` is the only 16-byte stream of the wave kernels.
template <int DIM, typename T>
static int diag(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&tab)[3], const T *g, const T *w,
                double lambda, T *out, void *stream)
{
    const bool has_w = lambda != 0.0; // false for NaN too, which is refused with the nulls
    Operands<DIM, T> o(nq, nelmt);
    for (int d = 0; d < DIM; ++d)
        o.add(tab[d], sizeof(T) * 3 * (nq[d] - 1) * nq[d], kIn | kGuard);
    o.add(g, DIM * (DIM + 1) / 2 * o.points, kIn | kGuard);
    o.add_if(has_w, w, o.points, kIn | kGuard);
    o.add(out, o.modes, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq), lambda - lambda == 0.0);
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(tab, nullptr, nullptr, out, nelmt); // the tables in the place of the bases
    const DiagArgsT<T> x{g, has_w ? w : nullptr, (T)lambda};                    // lambda is rounded to T here, once
    return route<DIM>(
        variant, nq, diag_generic_built(DIM, nq[0], nq[1], nq[2]), diag_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_diag_wave<DIM, T>(nq[0], a, x, s); }, [&] { return launch_diag_generic<DIM, T>(nq, a, x, s); });
}

// the tables of one direction: range, nulls, scalar alignment, `tab` overlapping an input, then the one kernel
template <typename T> static int diag_tables(unsigned nq, const T *basis, const T *deriv, T *tab, void *stream)
{
    if (nq < 2 || nq > 1024)
        return SF_EINVAL;
    if (!basis || !deriv || !tab)
        return SF_EINVAL;
    if (!aligned(basis, sizeof(T)) || !aligned(deriv, sizeof(T)) || !aligned(tab, sizeof(T)))
        return SF_EALIGN;
    const size_t nb = sizeof(T) * (nq - 1) * nq;
    if (overlaps(tab, 3 * nb, basis, nb) || overlaps(tab, 3 * nb, deriv, sizeof(T) * nq * nq))
        return SF_EINVAL;
    return launch_diag_tables<T>(nq, basis, deriv, tab, (hipStream_t)stream);
}

// ---- the geometric factors from element coordinates ----------------------------------------------------------------------
// DIM coordinate streams of modes and four outputs, each looked at only when it is not null (all four null: refused with
// the nulls); the quadrature weights are looked at only when w or g is asked for.  Every x_a and every output that is
// asked for is a 16-byte stream of the wave kernels.
template <int DIM, typename T>
static int geom(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                const T *const (&qw)[3], const T *const (&x)[3], T *df, T *w, T *g, T *detj, void *stream)
{
    const bool has_q = w || g;
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.weights(qw, has_q);
    o.each(x, o.modes, kIn | kGuard | kStream);
    o.add_if(df != nullptr, df, DIM * DIM * o.points, kOut | kStream);
    o.add_if(w != nullptr, w, o.points, kOut | kStream);
    o.add_if(g != nullptr, g, DIM * (DIM + 1) / 2 * o.points, kOut | kStream);
    o.add_if(detj != nullptr, detj, o.points, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq), df || w || g || detj);
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, nullptr, nelmt);
    const GeomArgsT<T> ga{d[0], d[1], d[2], has_q ? qw[0] : nullptr, has_q ? qw[1] : nullptr, has_q ? qw[2] : nullptr,
                          x[0], x[1], x[2], df, w, g, detj};
    return route<DIM>(
        variant, nq, geom_generic_built(DIM, nq[0], nq[1], nq[2]), geom_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_geom_wave<DIM, T>(nq[0], a, ga, s); },
        [&] { return launch_geom_generic<DIM, T>(nq, a, ga, s); });
}

// The affine form: sf_geom_* without a variant and without quadrature weights; one small kernel for any extents the
// fallback takes.
template <int DIM, typename T>
static int geom_affine(const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                       const T *const (&x)[3], T *dfe, T *ge, T *je, void *stream)
{
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.each(x, o.modes, kIn | kGuard);
    o.add_if(dfe != nullptr, dfe, DIM * DIM * o.elmt, kOut);
    o.add_if(ge != nullptr, ge, DIM * (DIM + 1) / 2 * o.elmt, kOut);
    o.add_if(je != nullptr, je, o.elmt, kOut);
    const int rc = o.check(range_ok<DIM>(SF_VARIANT_AUTO, nq), dfe || ge || je);
    if (rc != kProceed)
        return rc;
    if (!geom_generic_built(DIM, nq[0], nq[1], nq[2]))
        return SF_ENOTBUILT;
    const auto a = make_args<DIM, T>(b, nullptr, nullptr, nullptr, nelmt);
    const GeomArgsT<T> ga{d[0], d[1], d[2], nullptr, nullptr, nullptr, x[0], x[1], x[2], dfe, je, ge, nullptr};
    return launch_geom_affine<DIM, T>(nq, a, ga, (hipStream_t)stream);
}

// ---- the weak advection term ------------------------------------------------------------------------------------------------
// df, w and the DIM planes of the advecting velocity in front of nf = 1 or DIM fields of modes in and out (another nf is
// out of range); all of df, w, c_j are required.  Every in_a and out_a that the call takes (a < nf) is a 16-byte stream of
// the wave kernels; those with a >= nf are not looked at, and the args carry field 0 in their place.
template <int DIM, typename T>
static int advect(int variant, const unsigned (&nq)[3], size_t nelmt, unsigned nf, const T *const (&b)[3],
                  const T *const (&d)[3], const T *df, const T *w, const T *const (&c)[3], const T *const (&in)[3],
                  T *const (&out)[3], void *stream)
{
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.add(df, DIM * DIM * o.points, kIn | kGuard);
    o.add(w, o.points, kIn | kGuard);
    o.each(c, o.points, kIn | kGuard);
    o.each(in, o.modes, kIn | kGuard | kStream, nf);
    o.each(out, o.modes, kOut | kStream, nf);
    const int rc = o.check(range_ok<DIM>(variant, nq) && (nf == 1 || nf == (unsigned)DIM));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, nullptr, nelmt);
    const int f1 = nf > 1 ? 1 : 0, f2 = nf > 2 ? 2 : 0;
    const AdvectArgsT<T> x{d[0], d[1], d[2], df, w, c[0], c[1], c[2], in[0], in[f1], in[f2], out[0], out[f1], out[f2],
                           (int)nf};
    return route<DIM>(
        variant, nq, advect_generic_built(DIM, nq[0], nq[1], nq[2]), advect_wave_built(DIM, nq[0]), o.streams, o.streams,
        [&] { return launch_advect_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_advect_generic<DIM, T>(nq, a, x, s); });
}

// ---- the weak advection term on affine elements -----------------------------------------------------------------------------
// sf_advect_* with dfe (required) in the place of df and the quadrature weights and je in the place of w: `je` and every
// `qw` are looked at only when je is not null.
template <int DIM, typename T>
static int affine_advect(int variant, const unsigned (&nq)[3], size_t nelmt, unsigned nf, const T *const (&b)[3],
                         const T *const (&d)[3], const T *const (&qw)[3], const T *dfe, const T *je,
                         const T *const (&c)[3], const T *const (&in)[3], T *const (&out)[3], void *stream)
{
    const bool has_w = je != nullptr;
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d);
    o.weights(qw, has_w);
    o.add(dfe, DIM * DIM * o.elmt, kIn | kGuard);
    o.add_if(has_w, je, o.elmt, kIn | kGuard);
    o.each(c, o.points, kIn | kGuard);
    o.each(in, o.modes, kIn | kGuard | kStream, nf);
    o.each(out, o.modes, kOut | kStream, nf);
    const int rc = o.check(range_ok<DIM>(variant, nq) && (nf == 1 || nf == (unsigned)DIM));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, nullptr, nelmt);
    const int f1 = nf > 1 ? 1 : 0, f2 = nf > 2 ? 2 : 0;
    const AffineAdvectArgsT<T> x{d[0], d[1], d[2], has_w ? qw[0] : nullptr, has_w ? qw[1] : nullptr,
                                 has_w ? qw[2] : nullptr, dfe, je, c[0], c[1], c[2], in[0], in[f1], in[f2], out[0],
                                 out[f1], out[f2], (int)nf};
    return route<DIM>(
        variant, nq, affine_advect_generic_built(DIM, nq[0], nq[1], nq[2]), affine_advect_wave_built(DIM, nq[0]),
        o.streams, o.streams, [&] { return launch_affine_advect_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_affine_advect_generic<DIM, T>(nq, a, x, s); });
}

// ---- gradient, divergence and curl of a vector field ------------------------------------------------------------------------
// df (required) and DIM fields of modes, and up to five outputs, each looked at only when it is not null (all null:
// refused with the nulls; 3D: curl0..2 all null or none, refused with the nulls too; 2D: curl1, curl2 are not looked at).
// Every in_a and every output that is asked for is a 16-byte stream of the wave kernels.  The one family whose outputs
// may not lie over a basis or a derivative matrix (see kGuard).
template <int DIM, typename T>
static int vecgrad(int variant, const unsigned (&nq)[3], size_t nelmt, const T *const (&b)[3], const T *const (&d)[3],
                   const T *df, const T *const (&in)[3], T *grad, T *div, T *const (&curl)[3], void *stream)
{
    constexpr int NC = DIM == 3 ? 3 : 1; // planes of the curl
    T *c[3]          = {curl[0], DIM == 3 ? curl[1] : nullptr, DIM == 3 ? curl[2] : nullptr};
    const int ncurl  = (c[0] != nullptr) + (c[1] != nullptr) + (c[2] != nullptr);
    Operands<DIM, T> o(nq, nelmt);
    o.matrices(b, d, kIn | kGuard);
    o.add(df, DIM * DIM * o.points, kIn | kGuard);
    o.each(in, o.modes, kIn | kGuard | kStream);
    o.add_if(grad != nullptr, grad, DIM * DIM * o.points, kOut | kStream);
    o.add_if(div != nullptr, div, o.points, kOut | kStream);
    for (int k = 0; k < 3; ++k)
        o.add_if(c[k] != nullptr, c[k], o.points, kOut | kStream);
    const int rc = o.check(range_ok<DIM>(variant, nq), (grad || div || ncurl) && (ncurl == 0 || ncurl == NC));
    if (rc != kProceed)
        return rc;
    const hipStream_t s = (hipStream_t)stream;
    const auto a        = make_args<DIM, T>(b, nullptr, nullptr, nullptr, nelmt);
    const VecgradArgsT<T> x{d[0], d[1], d[2], df, in[0], in[1], in[2], grad, div, c[0], c[1], c[2]};
    return route<DIM>(
        variant, nq, vecgrad_generic_built(DIM, nq[0], nq[1], nq[2]), vecgrad_wave_built(DIM, nq[0]), o.streams,
        o.streams, [&] { return launch_vecgrad_wave<DIM, T>(nq[0], a, x, s); },
        [&] { return launch_vecgrad_generic<DIM, T>(nq, a, x, s); });
}

// ---- gather-scatter: the checks of the four calls, in the order include/sumfact.h documents --------------------------
// counts beyond 2^31 - 1 (SF_EINVAL), a count of zero (SF_OK), a null among `ptrs` (SF_EINVAL), an index array that is not
// 4-byte aligned or a value array that is not `align`-aligned (SF_EALIGN); `sign` may be null
constexpr size_t kGsMaxCount = 0x7fffffffull;
static int gs_validate(size_t n0, size_t n1, std::initializer_list<const void *> index, size_t align,
                       std::initializer_list<const void *> values, const void *sign)
{
    if (n0 > kGsMaxCount || n1 > kGsMaxCount)
        return SF_EINVAL;
    if (n0 == 0 || n1 == 0)
        return SF_OK;
    for (const void *p : index)
        if (!p)
            return SF_EINVAL;
    for (const void *p : values)
        if (!p)
            return SF_EINVAL;
    for (const void *p : index)
        if (!aligned(p, sizeof(int32_t)))
            return SF_EALIGN;
    for (const void *p : values)
        if (!aligned(p, align))
            return SF_EALIGN;
    return aligned(sign, align) ? kProceed : (int)SF_EALIGN;
}

template <typename T>
static int global_to_local(size_t nlocal, const int32_t *l2g, const T *sign, const T *global, T *local, void *stream)
{
    const int rc = gs_validate(nlocal, 1, {l2g}, sizeof(T), {global, local}, sign);
    return rc != kProceed ? rc : launch_global_to_local<T>(nlocal, l2g, sign, global, local, (hipStream_t)stream);
}

template <typename T>
static int assemble(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, const T *local, T *global,
                    void *stream)
{
    const int rc = gs_validate(nglobal, 1, {rows, perm}, sizeof(T), {local, global}, sign);
    return rc != kProceed ? rc : launch_assemble<T>(nglobal, rows, perm, sign, local, global, (hipStream_t)stream);
}

template <typename T>
static int gs(size_t nglobal, const int32_t *rows, const int32_t *perm, const T *sign, T *local, void *stream)
{
    const int rc = gs_validate(nglobal, 1, {rows, perm}, sizeof(T), {local}, sign);
    return rc != kProceed ? rc : launch_gs<T>(nglobal, rows, perm, sign, local, (hipStream_t)stream);
}

extern "C" {

int sf_version(void)
{
    return SF_VERSION;
}

const char *sf_error_string(int rc)
{
    switch (rc)
    {
    case SF_OK: return "success";
    case SF_EINVAL: return "invalid argument (nq < 2, null pointer, unknown variant or missing workspace)";
    case SF_EALIGN: return "pointer not sufficiently aligned";
    case SF_ENOTBUILT: return "variant not instantiated for these extents";
    case SF_ENOMEM: return "internal workspace allocation failed";
    case SF_ECOMPILE: return "run-time specialisation unavailable (hiprtc missing, compile failed, or it would spill)";
    default: return rc > 0 ? hipGetErrorString((hipError_t)rc) : "unknown sumfact error";
    }
}

const char *sf_variant_name(int variant)
{
    static const char *names[SF_NUM_VARIANTS] = {"auto",      "wave",    "thread", "block-lds",
                                                 "block-glb", "generic", "mfma",   "mfma4",
                                                 "wave-rt"};
    return (variant >= 0 && variant < SF_NUM_VARIANTS) ? names[variant] : "?";
}

// ---- the operator entry points ---------------------------------------------------------------------------------------
// Every operator family has six: sf_<stem>_{hex,quad}_f64_variant (the variant first), sf_<stem>_{hex,quad}_f64 and
// sf_<stem>_{hex,quad}_f32 (both SF_VARIANT_AUTO).  All six forward to the family's one function above, family<DIM, T>,
// with the per-direction operands in brace groups.  A family spells its parameter list and its forwarding call once, in
// a macro SF_<FAMILY>(name, D, T, V) -- D: 3 or 2, T: double or float, V: VAR or AUTO -- and SF_ENTRIES stamps the six
// definitions out of it.  include/sumfact.h declares every one of them by hand: a definition whose type differs from
// its declaration does not compile.
// To add a family: write family<DIM, T> above, its macro here from the words below, and one SF_ENTRIES line.
//   SF_P<D>(q, n)   one parameter `q *n<d>` per direction      SF_A<D>(n)   the group {n0, n1, n2} / {n0, n1, nullptr}
//   SF_NQ_P<D>      the extents as parameters                  SF_NQ_A<D>   {nq0, nq1, nq2} / {nq0, nq1, 0u}
//   SF_VP_<V>       `int variant,` / nothing                   SF_VA_<V>    variant / SF_VARIANT_AUTO
#define SF_P3(q, n) q *n##0, q *n##1, q *n##2
#define SF_P2(q, n) q *n##0, q *n##1
#define SF_A3(n) {n##0, n##1, n##2}
#define SF_A2(n) {n##0, n##1, nullptr}
#define SF_NQ_P3 unsigned nq0, unsigned nq1, unsigned nq2
#define SF_NQ_P2 unsigned nq0, unsigned nq1
#define SF_NQ_A3 {nq0, nq1, nq2}
#define SF_NQ_A2 {nq0, nq1, 0u}
#define SF_VP_VAR int variant,
#define SF_VP_AUTO
#define SF_VA_VAR variant
#define SF_VA_AUTO SF_VARIANT_AUTO
#define SF_ENTRIES(FAMILY, stem)                                                                                       \
    FAMILY(sf_##stem##_hex_f64_variant, 3, double, VAR)                                                                \
    FAMILY(sf_##stem##_hex_f64, 3, double, AUTO)                                                                       \
    FAMILY(sf_##stem##_quad_f64_variant, 2, double, VAR)                                                               \
    FAMILY(sf_##stem##_quad_f64, 2, double, AUTO)                                                                      \
    FAMILY(sf_##stem##_hex_f32, 3, float, AUTO)                                                                        \
    FAMILY(sf_##stem##_quad_f32, 2, float, AUTO)

// ---- BwdTrans: the variant form alone takes the caller-owned workspace ---------------------------------------------
#define SF_WSP_P_VAR(T) T *wsp,
#define SF_WSP_P_AUTO(T)
#define SF_WSP_A_VAR wsp
#define SF_WSP_A_AUTO nullptr
#define SF_BWDTRANS(name, D, T, V)                                                                                     \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), const T *in, SF_WSP_P_##V(T) T *out,         \
             void *stream)                                                                                             \
    {                                                                                                                  \
        return bwdtrans<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), in, SF_WSP_A_##V, out, stream);            \
    }
SF_ENTRIES(SF_BWDTRANS, bwdtrans)

// SF_VARIANT_MFMA4's leg of bwdtrans<3, double> with the output path named instead of chosen per order
int sf_bwdtrans_hex_f64_mfma4(int direct, unsigned nq, size_t nelmt, const double *basis0, const double *basis1,
                              const double *basis2, const double *in, double *out, void *stream)
{
    const int pre = validate(range_ok<3>(SF_VARIANT_MFMA4, {nq, nq, nq}), nelmt, {basis0, basis1, basis2, in, out}, sizeof(double));
    if (pre != kProceed)
        return pre;
    if (!aligned(in, 16) || !aligned(out, 16))
        return SF_EALIGN;
    const HexArgs a{basis0, basis1, basis2, in, nullptr, out, (uint64_t)nelmt};
    return launch_hex_mfma4_path(direct != 0, nq, a, (hipStream_t)stream);
}

int sf_bwdtrans_hex_f64_interleaved(unsigned nq0, unsigned nq1, unsigned nq2, size_t nelmt,
                                    const double *basis0, const double *basis1, const double *basis2,
                                    const double *in_il, double *wsp_il, double *out_il, void *stream)
{
    if (nq0 < 2 || nq1 < 2 || nq2 < 2)
        return SF_EINVAL;
    if (nelmt == 0)
        return SF_OK;
    if (!basis0 || !basis1 || !basis2 || !in_il || !wsp_il || !out_il)
        return SF_EINVAL;
    if (!aligned(in_il, 8) || !aligned(out_il, 8) || !aligned(wsp_il, 8)) // not the bases: validate() would check them
        return SF_EALIGN;
    HexArgs a{basis0, basis1, basis2, in_il, wsp_il, out_il, (uint64_t)nelmt};
    return launch_hex_interleaved(nq0, nq1, nq2, a, (hipStream_t)stream);
}

int sf_interleave64_f64(const double *src, double *dst, size_t nelmt, size_t n, int inverse,
                        void *stream)
{
    if ((!src || !dst) && nelmt * n)
        return SF_EINVAL;
    return launch_interleave64(src, dst, nelmt, n, inverse, (hipStream_t)stream);
}

// ---- IProductWRTBase, the transpose of BwdTrans ----------------------------------------------------------------------
#define SF_IPRODUCT(name, D, T, V)                                                                                     \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), const T *in, T *out, void *stream)           \
    {                                                                                                                  \
        return iprod<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), in, out, stream);                             \
    }
SF_ENTRIES(SF_IPRODUCT, iproduct)

// ---- the fused mass operator: BwdTrans, pointwise weight, IProductWRTBase in one kernel -------------------------------
#define SF_MASS(name, D, T, V)                                                                                         \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), const T *w, const T *in, T *out,             \
             void *stream)                                                                                             \
    {                                                                                                                  \
        return mass<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), w, in, out, stream);                           \
    }
SF_ENTRIES(SF_MASS, mass)

// ---- the fused Helmholtz operator: BwdTrans, derivatives, metric, transposed derivatives, IProductWRTBase in one kernel -
#define SF_HELMHOLTZ(name, D, T, V)                                                                                    \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), const T *g,         \
             const T *w, double lambda, const T *in, T *out, void *stream)                                             \
    {                                                                                                                  \
        return helmholtz<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), g, w, lambda, in, out,    \
                               stream);                                                                                \
    }
SF_ENTRIES(SF_HELMHOLTZ, helmholtz)

// ---- the fused Helmholtz operator on affine elements: a constant metric per element, shared quadrature weights ---------
#define SF_AFFINE_HELMHOLTZ(name, D, T, V)                                                                             \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv),                     \
             SF_P##D(const T, qw), const T *ge, const T *je, double lambda, const T *in, T *out, void *stream)         \
    {                                                                                                                  \
        return affine<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), SF_A##D(qw), ge, je, lambda, \
                            in, out, stream);                                                                          \
    }
SF_ENTRIES(SF_AFFINE_HELMHOLTZ, affine_helmholtz)

// ---- BwdTrans fused with the physical-space gradient: d outputs, no point image in HBM ---------------------------------
#define SF_PHYSDERIV(name, D, T, V)                                                                                    \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), const T *df,        \
             const T *in, SF_P##D(T, out), void *stream)                                                               \
    {                                                                                                                  \
        return physderiv<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), df, in, SF_A##D(out),     \
                               stream);                                                                                \
    }
SF_ENTRIES(SF_PHYSDERIV, physderiv)

// ---- IProductWRTDerivBase: d inputs at the points, the weak divergence in modes -----------------------------------------
#define SF_IPRODDERIV(name, D, T, V)                                                                                   \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), const T *df,        \
             const T *w, SF_P##D(const T, in), T *out, void *stream)                                                   \
    {                                                                                                                  \
        return iprodderiv<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), df, w, SF_A##D(in), out, \
                                stream);                                                                               \
    }
SF_ENTRIES(SF_IPRODDERIV, iprodderiv)

// ---- the gradient on affine elements: d*d constants per element in the place of the planes --------------------------------
#define SF_AFF_PHYSDERIV(name, D, T, V)                                                                                \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), const T *dfe,       \
             const T *in, SF_P##D(T, out), void *stream)                                                               \
    {                                                                                                                  \
        return affine_physderiv<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), dfe, in,           \
                                      SF_A##D(out), stream);                                                           \
    }
SF_ENTRIES(SF_AFF_PHYSDERIV, aff_physderiv)

// ---- the weak divergence on affine elements: the transpose of the gradient above, weighted by je (x) qw -------------------
#define SF_AFF_IPRODDERIV(name, D, T, V)                                                                               \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv),                     \
             SF_P##D(const T, qw), const T *dfe, const T *je, SF_P##D(const T, in), T *out, void *stream)              \
    {                                                                                                                  \
        return affine_iprodderiv<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), SF_A##D(qw), dfe, \
                                       je, SF_A##D(in), out, stream);                                                  \
    }
SF_ENTRIES(SF_AFF_IPRODDERIV, aff_iprodderiv)

// ---- the diagonal of the fused Helmholtz operator: Jacobi preconditioner, Chebyshev smoother, diagonal scaling ----------
int sf_diag_tables_f64(unsigned nq, const double *basis, const double *deriv, double *tab, void *stream)
{
    return diag_tables<double>(nq, basis, deriv, tab, stream);
}

int sf_diag_tables_f32(unsigned nq, const float *basis, const float *deriv, float *tab, void *stream)
{
    return diag_tables<float>(nq, basis, deriv, tab, stream);
}

#define SF_DIAG_HELMHOLTZ(name, D, T, V)                                                                               \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, tab), const T *g, const T *w, double lambda, T *out, \
             void *stream)                                                                                             \
    {                                                                                                                  \
        return diag<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(tab), g, w, lambda, out, stream);                      \
    }
SF_ENTRIES(SF_DIAG_HELMHOLTZ, diag_helmholtz)

// ---- the geometric factors df, w, g, detj from the modal coordinates of every element -----------------------------------
#define SF_GEOM(name, D, T, V)                                                                                         \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv),                     \
             SF_P##D(const T, qw), SF_P##D(const T, x), T *df, T *w, T *g, T *detj, void *stream)                      \
    {                                                                                                                  \
        return geom<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), SF_A##D(qw), SF_A##D(x), df,   \
                          w, g, detj, stream);                                                                         \
    }
SF_ENTRIES(SF_GEOM, geom)

// the affine form has no variant: four entries
#define SF_GEOM_AFFINE(name, D, T)                                                                                     \
    int name(SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), SF_P##D(const T, x), T *dfe,  \
             T *ge, T *je, void *stream)                                                                               \
    {                                                                                                                  \
        return geom_affine<D, T>(SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), SF_A##D(x), dfe, ge, je, stream);  \
    }
SF_GEOM_AFFINE(sf_geom_affine_hex_f64, 3, double)
SF_GEOM_AFFINE(sf_geom_affine_quad_f64, 2, double)
SF_GEOM_AFFINE(sf_geom_affine_hex_f32, 3, float)
SF_GEOM_AFFINE(sf_geom_affine_quad_f32, 2, float)

// ---- the weak advection term out_a = B^T [w (c . grad) B in_a], nf = 1 or d fields ------------------------------------
#define SF_ADVECT(name, D, T, V)                                                                                       \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, unsigned nf, SF_P##D(const T, basis), SF_P##D(const T, deriv),        \
             const T *df, const T *w, SF_P##D(const T, c), SF_P##D(const T, in), SF_P##D(T, out), void *stream)        \
    {                                                                                                                  \
        return advect<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, nf, SF_A##D(basis), SF_A##D(deriv), df, w, SF_A##D(c),       \
                            SF_A##D(in), SF_A##D(out), stream);                                                        \
    }
SF_ENTRIES(SF_ADVECT, advect)

// ---- the weak advection term on affine elements, out_a = B^T [(je q) (c . grad) B in_a], nf = 1 or d fields ---------
#define SF_AFF_ADVECT(name, D, T, V)                                                                                   \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, unsigned nf, SF_P##D(const T, basis), SF_P##D(const T, deriv),        \
             SF_P##D(const T, qw), const T *dfe, const T *je, SF_P##D(const T, c), SF_P##D(const T, in),               \
             SF_P##D(T, out), void *stream)                                                                            \
    {                                                                                                                  \
        return affine_advect<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, nf, SF_A##D(basis), SF_A##D(deriv), SF_A##D(qw), dfe, \
                                   je, SF_A##D(c), SF_A##D(in), SF_A##D(out), stream);                                 \
    }
SF_ENTRIES(SF_AFF_ADVECT, aff_advect)

// ---- the gradient, divergence and curl of a vector field at the quadrature points ---------------------------------------
// the planes of the curl number d(d-1)/2, not d: a parameter list and a group of their own
#define SF_CURL_P3(q) q *curl0, q *curl1, q *curl2
#define SF_CURL_P2(q) q *curl0
#define SF_CURL_A3 {curl0, curl1, curl2}
#define SF_CURL_A2 {curl0, nullptr, nullptr}
#define SF_VECGRAD(name, D, T, V)                                                                                      \
    int name(SF_VP_##V SF_NQ_P##D, size_t nelmt, SF_P##D(const T, basis), SF_P##D(const T, deriv), const T *df,        \
             SF_P##D(const T, in), T *grad, T *div, SF_CURL_P##D(T), void *stream)                                     \
    {                                                                                                                  \
        return vecgrad<D, T>(SF_VA_##V, SF_NQ_A##D, nelmt, SF_A##D(basis), SF_A##D(deriv), df, SF_A##D(in), grad, div, \
                             SF_CURL_A##D, stream);                                                                    \
    }
SF_ENTRIES(SF_VECGRAD, vecgrad)

// ---- gather-scatter: Q, Q^T and Q Q^T of a local-to-global map, and the setup that inverts the map --------------------
int sf_gs_setup(size_t nlocal, size_t nglobal, const int32_t *l2g, int32_t *rows, int32_t *perm, void *stream)
{
    const int rc = gs_validate(nlocal, nglobal, {l2g, rows, perm}, sizeof(int32_t), {}, nullptr);
    return rc != kProceed ? rc : gs_setup(nlocal, nglobal, l2g, rows, perm, (hipStream_t)stream);
}

int sf_global_to_local_f64(size_t nlocal, const int32_t *l2g, const double *sign, const double *global, double *local,
                           void *stream)
{
    return global_to_local<double>(nlocal, l2g, sign, global, local, stream);
}

int sf_global_to_local_f32(size_t nlocal, const int32_t *l2g, const float *sign, const float *global, float *local,
                           void *stream)
{
    return global_to_local<float>(nlocal, l2g, sign, global, local, stream);
}

int sf_assemble_f64(size_t nglobal, const int32_t *rows, const int32_t *perm, const double *sign, const double *local,
                    double *global, void *stream)
{
    return assemble<double>(nglobal, rows, perm, sign, local, global, stream);
}

int sf_assemble_f32(size_t nglobal, const int32_t *rows, const int32_t *perm, const float *sign, const float *local,
                    float *global, void *stream)
{
    return assemble<float>(nglobal, rows, perm, sign, local, global, stream);
}

int sf_gs_f64(size_t nglobal, const int32_t *rows, const int32_t *perm, const double *sign, double *local, void *stream)
{
    return gs<double>(nglobal, rows, perm, sign, local, stream);
}

int sf_gs_f32(size_t nglobal, const int32_t *rows, const int32_t *perm, const float *sign, float *local, void *stream)
{
    return gs<float>(nglobal, rows, perm, sign, local, stream);
}

int sf_sumsq_f32(const float *x, size_t n, double *result_host, void *stream)
{
    if (!result_host || (!x && n))
        return SF_EINVAL;
    if (n == 0)
    {
        *result_host = 0.0;
        return SF_OK;
    }
    return sumsq_f32_blocking(x, n, result_host, (hipStream_t)stream);
}

int sf_fill_sincos_f32(float *in, size_t nelmt, size_t nm_tot, void *stream)
{
    if ((!in && nelmt * nm_tot) || nm_tot > 0xffffffffull)
        return SF_EINVAL;
    return fill_sincos_f32(in, nelmt, nm_tot, (hipStream_t)stream);
}

int sf_fill_basis_f32(float *basis, size_t nm, size_t nq, void *stream)
{
    if ((!basis && nm * nq) || nm * nq > 0xffffffffull)
        return SF_EINVAL;
    return fill_basis_f32(basis, nm, nq, (hipStream_t)stream);
}

int sf_fill_random_f32(float *x, size_t n, uint64_t seed, uint64_t first_idx, void *stream)
{
    if (!x && n)
        return SF_EINVAL;
    return fill_random_f32(x, n, seed, first_idx, (hipStream_t)stream);
}

int sf_sumsq_f64(const double *x, size_t n, double *result_host, void *stream)
{
    if (!result_host || (!x && n))
        return SF_EINVAL;
    if (n == 0)
    {
        *result_host = 0.0;
        return SF_OK;
    }
    if (!aligned(x, 8))
        return SF_EALIGN;
    return sumsq_blocking(x, n, result_host, (hipStream_t)stream);
}

int sf_sumsq_f64_async(const double *x, size_t n, double *result_dev, void *stream)
{
    if (!result_dev || (!x && n))
        return SF_EINVAL;
    if (!aligned(x, 8))
        return SF_EALIGN;
    return sumsq_async(x, n, result_dev, (hipStream_t)stream);
}

int sf_fill_sincos_f64(double *in, size_t nelmt, size_t nm_tot, void *stream)
{
    if ((!in && nelmt * nm_tot) || nm_tot > 0xffffffffull)
        return SF_EINVAL;
    return fill_sincos(in, nelmt, nm_tot, (hipStream_t)stream);
}

int sf_fill_basis_f64(double *basis, size_t nm, size_t nq, void *stream)
{
    if ((!basis && nm * nq) || nm * nq > 0xffffffffull)
        return SF_EINVAL;
    return fill_basis(basis, nm, nq, (hipStream_t)stream);
}

int sf_fill_random_f64(double *x, size_t n, uint64_t seed, uint64_t first_idx, void *stream)
{
    if (!x && n)
        return SF_EINVAL;
    return fill_random(x, n, seed, first_idx, (hipStream_t)stream);
}

int sf_fill_l2norm_f64(double *x, size_t n, void *stream)
{
    if (!x && n)
        return SF_EINVAL;
    return fill_l2norm(x, n, (hipStream_t)stream);
}

int sf_stream_copy_f64(const double *src, double *dst, size_t n, void *stream)
{
    if ((!src || !dst) && n)
        return SF_EINVAL;
    return stream_copy(src, dst, n, (hipStream_t)stream);
}

int sf_vector_add_f64(double *x, const double *y, size_t n, void *stream)
{
    if ((!x || !y) && n)
        return SF_EINVAL;
    if (!aligned(x, 8) || !aligned(y, 8))
        return SF_EALIGN;
    return vector_add(x, y, n, (hipStream_t)stream);
}

int sf_fill_vecadd_f64(double *x, double *y, size_t n, void *stream)
{
    if ((!x || !y) && n)
        return SF_EINVAL;
    return fill_vecadd(x, y, n, (hipStream_t)stream);
}

int sf_matvec_f64(unsigned m, unsigned n, const double *A, const double *x, double *y, void *stream)
{
    if ((!A || !x || !y) && m && n)
        return SF_EINVAL;
    if (!aligned(A, 8) || !aligned(x, 8) || !aligned(y, 8))
        return SF_EALIGN;
    return matvec(m, n, A, x, y, (hipStream_t)stream);
}

int sf_fill_matvec_f64(double *A, double *x, unsigned m, unsigned n, void *stream)
{
    if ((!A || !x) && m && n)
        return SF_EINVAL;
    return fill_matvec(A, x, m, n, (hipStream_t)stream);
}

int sf_set_launch_hint(unsigned threads, unsigned elblocks)
{
    return set_launch_hint(threads, elblocks);
}

int sf_device_info(int *num_cu, int *wave_size, char *name, size_t name_len)
{
    int dev      = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return (int)e;
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess)
        return (int)e;
    if (num_cu)
        *num_cu = p.multiProcessorCount;
    if (wave_size)
        *wave_size = p.warpSize;
    if (name && name_len)
    {
        std::snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName);
    }
    return SF_OK;
}

// ---- tensor-product apply ----------------------------------------------------------------------------------------
// two extent triples, padded with 1u in 2D, and an _f32_variant form besides the six
#define SF_NIO_P3 unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1, unsigned no2
#define SF_NIO_P2 unsigned ni0, unsigned ni1, unsigned no0, unsigned no1
#define SF_NIO_A3 {ni0, ni1, ni2}, {no0, no1, no2}
#define SF_NIO_A2 {ni0, ni1, 1u}, {no0, no1, 1u}
#define SF_TENSOR(name, D, T, V)                                                                                       \
    int name(SF_VP_##V SF_NIO_P##D, int trans, size_t nelmt, SF_P##D(const T, m), const T *in, T *out, void *stream)   \
    {                                                                                                                  \
        return tensor<D, T>(SF_VA_##V, SF_NIO_A##D, trans, nelmt, SF_A##D(m), in, out, stream);                        \
    }
SF_ENTRIES(SF_TENSOR, tensor)
SF_TENSOR(sf_tensor_hex_f32_variant, 3, float, VAR)
SF_TENSOR(sf_tensor_quad_f32_variant, 2, float, VAR)

int sf_specialise_tensor(int dim, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1, unsigned no2,
                         int trans, int scalar_bytes)
{
    return rtc_specialise_tensor(dim, {ni0, ni1, ni2}, {no0, no1, no2}, trans, scalar_bytes);
}

int sf_tensor_specialisation_state(int dim, unsigned ni0, unsigned ni1, unsigned ni2, unsigned no0, unsigned no1,
                                   unsigned no2, int trans, int scalar_bytes, uint64_t *launches)
{
    return rtc_tensor_state(dim, {ni0, ni1, ni2}, {no0, no1, no2}, trans, scalar_bytes, launches);
}

// ---- run-time specialisation (rtc.hip) -------------------------------------------------------------------------
int sf_specialise(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes)
{
    return rtc_specialise(dim, nq0, nq1, nq2, scalar_bytes);
}

int sf_specialisation_state(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, uint64_t *launches)
{
    return rtc_state(dim, nq0, nq1, nq2, scalar_bytes, launches);
}

int sf_bwdtrans_specialised(int dim, unsigned nq0, unsigned nq1, unsigned nq2, int scalar_bytes, size_t nelmt,
                            const void *basis0, const void *basis1, const void *basis2, const void *in, void *out,
                            void *stream)
{
    const unsigned mx = dim == 3 ? 16u : 24u;
    const bool range  = (dim == 2 || dim == 3) && (scalar_bytes == 4 || scalar_bytes == 8) && nq0 >= 2 && nq1 >= 2 &&
                       nq0 <= mx && nq1 <= mx && (dim == 2 || (nq2 >= 2 && nq2 <= mx));
    const int pre = validate(range, nelmt, {basis0, basis1, dim == 3 ? basis2 : basis0, in, out}, (size_t)scalar_bytes);
    if (pre != kProceed)
        return pre;
    if (!aligned(in, 16) || !aligned(out, 16)) // the specialised kernels have no scalar-aligned path
        return SF_EALIGN;
    return launch_specialised(dim, nq0, nq1, dim == 3 ? nq2 : 0, scalar_bytes, basis0, basis1, basis2, in, out,
                              (uint64_t)nelmt, (hipStream_t)stream);
}

const char *sf_last_specialise_log(void)
{
    return rtc_last_log();
}

int sf_shutdown(void)
{
    const int rtc = rtc_release();
    (void)release_counters();
    const int rc = release_workspaces();
    return rc != SF_OK ? rc : rtc;
}

#undef SF_P3
#undef SF_P2
#undef SF_A3
#undef SF_A2
#undef SF_NQ_P3
#undef SF_NQ_P2
#undef SF_NQ_A3
#undef SF_NQ_A2
#undef SF_VP_VAR
#undef SF_VP_AUTO
#undef SF_VA_VAR
#undef SF_VA_AUTO
#undef SF_ENTRIES
#undef SF_WSP_P_VAR
#undef SF_WSP_P_AUTO
#undef SF_WSP_A_VAR
#undef SF_WSP_A_AUTO
#undef SF_CURL_P3
#undef SF_CURL_P2
#undef SF_CURL_A3
#undef SF_CURL_A2
#undef SF_NIO_P3
#undef SF_NIO_P2
#undef SF_NIO_A3
#undef SF_NIO_A2
#undef SF_BWDTRANS
#undef SF_IPRODUCT
#undef SF_MASS
#undef SF_HELMHOLTZ
#undef SF_AFFINE_HELMHOLTZ
#undef SF_PHYSDERIV
#undef SF_IPRODDERIV
#undef SF_AFF_PHYSDERIV
#undef SF_AFF_IPRODDERIV
#undef SF_DIAG_HELMHOLTZ
#undef SF_GEOM
#undef SF_GEOM_AFFINE
#undef SF_ADVECT
#undef SF_AFF_ADVECT
#undef SF_VECGRAD
#undef SF_TENSOR

} // extern "C"
