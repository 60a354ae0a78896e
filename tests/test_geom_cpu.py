"""CPU tests of the geometric factors (include/sumfact.h sf_geom_*, sf_geom_affine_*): the reference of tests/geom_ref.py
against closed forms (affine elements, the volume of trilinear elements, the patch test through the gradient's
reference), an evaluation in the working precision against the running bound and deliberate mutants that must exceed it
(the tests can fail), the header's text, the binding's symbol table, every validation rule by return code, and the
registers of every wave instantiation.  No GPU.
"""
import os
import re

import numpy as np
import pytest
from numpy.polynomial import legendre as _leg

from geom_ref import (LD, OUTPUTS, U32, U64, GeomRef, deformed, gamma, geom_eval, gll_operands, ref_geom, sizes)
from helm_ref import COMPONENTS
from physderiv_ref import _inv_ld, physderiv_n, ref_physderiv
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")
ULD = float(np.finfo(np.longdouble).eps) / 2                    # unit roundoff of the reference's own arithmetic
SHAPES = [(3, 3, 3), (5, 5, 5), (8, 8, 8), (6, 4, 5), (5, 5), (12, 12), (4, 9)]
NEW = ([f"sf_geom_{shape}_{sfx}" for shape in ("hex", "quad") for sfx in ("f64", "f64_variant", "f32")]
       + [f"sf_geom_affine_{shape}_{sfx}" for shape in ("hex", "quad") for sfx in ("f64", "f32")])
ids = lambda s: "x".join(map(str, s))      # noqa: E731


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


@pytest.mark.parametrize("nq", SHAPES, ids=ids)
def test_affine_elements_give_the_inverse_transpose_of_a(nq):
    """x = A xi + c: df[a d + b] = (A^-1)[b][a], detj = det A, w = |det A| q, g = w A^-1 A^-T at every point.  The
    reference's arithmetic is long double, but the GLL points, the basis values and the differentiation matrix it is given
    are fp64 numbers a few u64 from the exact ones (D P_1 is 1 only to that accuracy): the distance to the closed form
    is held to the running bound at u64, which charges every operand and operation that much on absolute values."""
    nelmt, d = 6, len(nq)
    B, D, Q = gll_operands(nq)
    xs, A = deformed(nq, nelmt, 11, affine=True)
    ref = GeomRef(nq, nelmt, B, D, Q, xs, U64)
    ref.check_condition()
    nqt = sizes(nq)[1]
    Ainv = _inv_ld(A)
    Al = np.asarray(A, dtype=LD)
    if d == 2:
        detA = Al[:, 0, 0] * Al[:, 1, 1] - Al[:, 0, 1] * Al[:, 1, 0]
    else:
        detA = sum(Al[:, 0, j] * (Al[:, 1, (j + 1) % 3] * Al[:, 2, (j + 2) % 3] - Al[:, 1, (j + 2) % 3] * Al[:, 2, (j + 1) % 3])
                   for j in range(3))
    qv = np.asarray(Q[0], dtype=LD)
    for b in range(1, d):
        qv = np.multiply.outer(np.asarray(Q[b], dtype=LD), qv)
    qv = qv.reshape(-1)
    want_df = np.empty((nelmt, d * d, nqt), dtype=LD)
    for a in range(d):
        for b in range(d):
            want_df[:, a * d + b] = Ainv[:, b, a][:, None]
    K = Ainv @ np.swapaxes(Ainv, 1, 2)                              # A^-1 A^-T
    want_w = np.abs(detA)[:, None] * qv[None]
    want_g = np.stack([want_w * K[:, a, b][:, None] for a, b in COMPONENTS[d]], axis=1)
    # the closed forms are themselves rounded (A in fp64, its inverse in long double): a few roundoffs of slack on top
    for name, want in (("df", want_df), ("w", want_w), ("g", want_g)):
        err = np.abs(ref.val[name] - want.reshape(-1))
        assert np.all(err <= 2 * ref.err[name] + 64 * ULD * np.abs(want.reshape(-1))), name
    det = ref.val["detj"].reshape(nelmt, nqt)
    assert np.all(np.abs(det - detA[:, None]) <= 2 * ref.err["detj"].reshape(nelmt, nqt) + 1e-15 * np.abs(detA)[:, None])


def test_trilinear_volume_is_the_gauss_legendre_integral_of_the_determinant():
    """Modes up to order one per direction: det J is a polynomial of degree <= 2 per direction, so the GLL sum of w and a
    12-point Gauss-Legendre integral of the analytic determinant are both exact up to rounding (the fp64 GLL points and
    weights carry a few 1e-16 each: 1e-13 relative on the sum)."""
    nq, nelmt = (4, 4, 4), 5
    B, D, Q = gll_operands(nq)
    rng = np.random.default_rng(5)
    coef = 0.15 * rng.uniform(-1, 1, (3, nelmt, 2, 2, 2))             # [a][e][r][q][p], p, q, r in {0, 1}
    for a in range(3):
        at = [0, 0, 0]
        at[2 - a] = 1
        coef[(a, slice(None)) + tuple(at)] += 1.0
    xs = []
    for a in range(3):
        x = np.zeros((nelmt, 3, 3, 3))
        x[:, :2, :2, :2] = coef[a]
        xs.append(x.reshape(-1))
    ref = ref_geom(nq, nelmt, B, D, Q, xs, U64)
    got = ref.val["w"].reshape(nelmt, -1).sum(axis=1)
    xg, wg = _leg.leggauss(12)
    P = np.stack([np.ones_like(xg), xg]).astype(LD)                  # P_0, P_1 at the Gauss points
    dP = np.stack([np.zeros_like(xg), np.ones_like(xg)]).astype(LD)
    J = np.empty((3, 3, nelmt, 12, 12, 12), dtype=LD)
    for a in range(3):
        for b in range(3):
            f = [dP if dd == b else P for dd in range(3)]
            J[a, b] = np.einsum("erqp,pi,qj,rk->ekji", coef[a].astype(LD), f[0], f[1], f[2])
    det = (J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])
           + J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))
    W = np.einsum("k,j,i->kji", wg, wg, wg).astype(LD)
    want = np.sum(np.abs(det) * W[None], axis=(1, 2, 3))
    assert np.all(det > 0)
    assert np.all(np.abs(got - want) <= 1e-13 * want), (got, want)


@pytest.mark.parametrize("nq", [(5, 5, 5), (8, 8, 8), (9, 9), (6, 4, 5)], ids=ids)
def test_patch_test_through_the_gradient_reference(nq):
    """in = sum_a c_a x_a is the linear function c . x of the physical coordinates: ref_physderiv on the reference's df
    returns c at every point, within the gradient's bound plus the propagated bound of df, both at long-double roundoff."""
    nelmt, d = 5, len(nq)
    B, D, Q = gll_operands(nq)
    xs, _ = deformed(nq, nelmt, 3)
    ref = ref_geom(nq, nelmt, B, D, Q, xs, ULD)
    c = np.asarray([0.7, -1.3, 0.4][:d])
    inp = sum(c[a] * xs[a] for a in range(d))
    out, absout = ref_physderiv(nq, nelmt, B, D, ref.val["df"], inp)
    du, _ = ref_physderiv(nq, nelmt, B, D, None, inp)
    nqt = sizes(nq)[1]
    edf = ref.err["df"].reshape(nelmt, d * d, nqt)
    dur = np.abs(du).reshape(d, nelmt, nqt)
    for a in range(d):
        tol = gamma(physderiv_n(nq), ULD) * absout[a].reshape(nelmt, nqt) + sum(edf[:, a * d + b] * dur[b] for b in range(d))
        # inp itself is rounded to fp64 once per mode: |c| |x| 2^-53 through the exact operator, below 64 u64 |c|
        err = np.abs(out[a].reshape(nelmt, nqt) - c[a])
        assert np.all(err <= 2 * tol + 64 * U64 * np.sum(np.abs(c))), (a, float(np.max(err)))
    assert float(np.max(np.abs(out))) > 0.3


@pytest.mark.parametrize("nq", [(3, 3, 3), (5, 5, 5), (8, 8, 8), (6, 6, 12), (5, 5), (16, 16), (23, 5)], ids=ids)
def test_working_precision_meets_the_bound_and_mutants_do_not(nq):
    """The documented order of operations in fp64 (numpy) is inside 2 e of the long-double reference at every value of
    every output; each deliberate mutant exceeds it at some point of the output it touches."""
    nelmt = 9
    B, D, Q = gll_operands(nq)
    xs, _ = deformed(nq, nelmt, 4)
    ref = ref_geom(nq, nelmt, B, D, Q, xs, U64)
    got = geom_eval(nq, nelmt, B, D, Q, xs, np.float64)
    for name in OUTPUTS:
        q = ref.excess(name, got[name])
        print(f"{nq} float64 {name}: max |err| / (2 e) = {q:.3g}")
        assert q <= 1.0, (name, q)
    touched = {"transposed-cofactor": ("df", "g"), "g-order": ("g",), "no-q": ("w", "g"), "c-order": ("df",)}
    for mutant, names in touched.items():
        bad = geom_eval(nq, nelmt, B, D, Q, xs, np.float64, mutant)
        for name in names:
            assert ref.excess(name, bad[name]) > 1e3, (mutant, name)
    # det without |.| in w shows on an inverted element only: negate one coordinate
    inv = [xs[0], -xs[1]] + xs[2:]
    rinv = ref_geom(nq, nelmt, B, D, Q, inv, U64)
    assert np.all(rinv.val["detj"] < 0) and np.all(rinv.val["w"] > 0)
    good, bad = geom_eval(nq, nelmt, B, D, Q, inv, np.float64), geom_eval(nq, nelmt, B, D, Q, inv, np.float64, "signed-w")
    assert rinv.excess("w", good["w"]) <= 1.0 and rinv.excess("g", good["g"]) <= 1.0
    assert rinv.excess("w", bad["w"]) > 1e3 and rinv.excess("g", bad["g"]) > 1e3


@pytest.mark.parametrize("nq", [(5, 5, 5), (8, 8, 8), (5, 5)], ids=ids)
def test_float32_evaluation_meets_its_bound(nq):
    nelmt = 9
    B, D, Q = gll_operands(nq)
    xs, _ = deformed(nq, nelmt, 6)
    r32 = lambda a: [np.asarray(v, dtype=np.float32).astype(np.float64) for v in a]      # noqa: E731  inputs rounded
    B, D, Q, xs = r32(B), r32(D), r32(Q), r32(xs)
    ref = ref_geom(nq, nelmt, B, D, Q, xs, U32)
    got = geom_eval(nq, nelmt, B, D, Q, xs, np.float32)
    for name in OUTPUTS:
        assert got[name].dtype == np.float32
        assert ref.excess(name, got[name]) <= 1.0, name


def test_condition_is_asserted_and_the_affine_reference_is_point_zero():
    nq, nelmt = (4, 4, 4), 3
    B, D, Q = gll_operands(nq)
    xs, _ = deformed(nq, nelmt, 8)
    flat = [np.zeros_like(x) for x in xs]                           # every element collapsed to a point: det = 0
    with pytest.raises(AssertionError, match="too close to singular"):
        ref_geom(nq, nelmt, B, D, Q, flat, U64)
    full, aff = ref_geom(nq, nelmt, B, D, Q, xs, U64), ref_geom(nq, nelmt, B, D, Q, xs, U64, affine=True)
    nqt = sizes(nq)[1]
    assert np.array_equal(aff.val["dfe"], full.val["df"].reshape(nelmt, 9, nqt)[:, :, 0].reshape(-1))
    assert np.array_equal(aff.val["je"], np.abs(full.val["detj"].reshape(nelmt, nqt)[:, 0]))
    assert aff.val["ge"].shape == (nelmt * 6,) and np.all(aff.err["ge"] > 0)
    assert np.isinf(full.excess("w", np.full(nelmt * nqt, np.nan)))


def test_binding_and_header_name_the_new_symbols(pkg):
    capi = pkg.capi
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    assert re.search(r"#define SF_VERSION 100\b", text) and capi.lib().sf_version() == 100
    for name in NEW:
        assert name in capi.SYMBOLS, name
        assert hasattr(capi.lib(), name), name
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(capi.SYMBOLS[name][1]), (name, params)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sf_geom_\w+)\s*\(", code))
    assert declared == set(NEW) == {n for n in capi.SYMBOLS if n.startswith("sf_geom_")}
    assert len(capi.SYMBOLS["sf_geom_hex_f64_variant"][1]) == 1 + 3 + 1 + 9 + 3 + 4 + 1   # variant nq nelmt b d qw x out s
    assert len(capi.SYMBOLS["sf_geom_quad_f32"][1]) == 2 + 1 + 6 + 2 + 4 + 1
    assert len(capi.SYMBOLS["sf_geom_affine_hex_f32"][1]) == 3 + 1 + 6 + 3 + 3 + 1
    for needle in ("df[e][c][k][j][i],   c = a*d + b for d xi_b / d x_a", "w[e][k][j][i] = |det J| * q",
                   "q = qw2[k] * (qw1[j] * qw0[i])", "c = 00, 01, 02, 11, 12, 22 (2D: 00, 01, 11)",
                   "G_ab = w * sum_x df[x*d + a] * df[x*d + b]", "detj[e][k][j][i] = det J, with its sign",
                   "cof[a][b] = fma(J[a+1][b+1], J[a+2][b+2], -(J[a+1][b+2] * J[a+2][b+1])), indices mod 3",
                   "cof = (J11, -J10, -J01, J00) in the order of c", "det = fma(J[0][b], cof[0][b], det)",
                   "r = 1 / det (a correctly rounded division)", "G_ab = w * (sum_x df[x*d + a] * df[x*d + b]), x ascending",
                   "Any output may be NULL: it is then neither written nor validated", "All four\n * NULL: SF_EINVAL",
                   "qw_d may be NULL when w and g are both NULL", "inf / NaN at that point only",
                   "any output overlapping any x_a or another output, compared as byte ranges of their full sizes",
                   "je[e] = |det J|", "ge[e][c] = je * sum_x dfe[x*d + a] * dfe[x*d + b]", "BIT\n * FOR BIT"):
        assert needle in text, needle


def test_validation_without_a_gpu(pkg):
    """Every rule of the documented order by return code; no call here reaches a launch."""
    lib, c = pkg.capi.lib(), pkg.capi
    A = 0x100000                                                       # 16-byte-aligned dummies, never dereferenced
    wave, generic, thread = pkg.VARIANTS["wave"], pkg.VARIANTS["generic"], pkg.VARIANTS["thread"]

    def hex_(variant, nq, nelmt, b=(A,) * 3, d=(A,) * 3, qw=(A,) * 3, x=(A + 0x100000, A + 0x200000, A + 0x300000),
             out=(A + 0x1000000, A + 0x3000000, A + 0x4000000, A + 0x6000000)):
        return lib.sf_geom_hex_f64_variant(variant, *nq, nelmt, *b, *d, *qw, *x, *out, None)

    def quad(variant, nq, nelmt, b=(A,) * 2, d=(A,) * 2, qw=(A,) * 2, x=(A + 0x100000, A + 0x200000),
             out=(A + 0x1000000, A + 0x3000000, A + 0x4000000, A + 0x6000000)):
        return lib.sf_geom_quad_f64_variant(variant, *nq, nelmt, *b, *d, *qw, *x, *out, None)

    n3, n2, N = (9, 9, 9), (17, 17), (None,) * 4
    # (1) an extent < 2, a variant out of range -- before everything else
    assert hex_(wave, (1, 9, 9), 4, b=(None,) * 3) == c.SF_EINVAL and quad(wave, (9, 1), 4) == c.SF_EINVAL
    assert hex_(99, n3, 4) == c.SF_EINVAL and hex_(-1, n3, 0) == c.SF_EINVAL
    # (2) an empty batch, whatever the pointers
    assert hex_(wave, n3, 0, b=(None,) * 3, out=N) == c.SF_OK and quad(thread, n2, 0, x=(None, None)) == c.SF_OK
    # (3) nulls: a basis, a derivative matrix, a coordinate, all four outputs, a weight while w or g is asked for
    assert hex_(wave, n3, 4, b=(A, None, A)) == c.SF_EINVAL and hex_(wave, n3, 4, d=(A, A, None)) == c.SF_EINVAL
    assert hex_(wave, n3, 4, x=(A + 0x100000, None, A + 0x300000)) == c.SF_EINVAL
    assert hex_(wave, n3, 4, out=N) == c.SF_EINVAL and quad(wave, n2, 4, out=N) == c.SF_EINVAL
    assert hex_(wave, n3, 4, qw=(A, A, None)) == c.SF_EINVAL
    assert hex_(wave, n3, 4, qw=(None, A, A), out=(None, None, A + 0x1000000, None)) == c.SF_EINVAL
    assert quad(wave, n2, 4, qw=(A, None), out=(None, A + 0x1000000, None, None)) == c.SF_EINVAL
    #     ... the weights may be null when neither is: the call goes on to (6)/(7); so may any three outputs
    assert hex_(wave, n3, 4, qw=(None,) * 3, out=(A + 0x1000000, None, None, A + 0x6000000)) == c.SF_ENOTBUILT
    for keep in range(4):
        out = tuple(A + 0x1000000 if o == keep else None for o in range(4))
        assert hex_(wave, n3, 4, out=out) == c.SF_ENOTBUILT and quad(wave, n2, 4, out=out) == c.SF_ENOTBUILT
    #     a null comes before a misaligned pointer
    assert hex_(wave, n3, 4, b=(A + 1, None, A)) == c.SF_EINVAL
    # (4) scalar alignment of what is looked at
    assert hex_(wave, n3, 4, b=(A + 4, A, A)) == c.SF_EALIGN and hex_(wave, n3, 4, x=(A + 0x100004, A, A)) == c.SF_EALIGN
    assert hex_(wave, n3, 4, out=(A + 0x1000000, A + 0x3000001, None, None)) == c.SF_EALIGN
    assert hex_(wave, n3, 4, qw=(A, A + 2, A)) == c.SF_EALIGN
    assert hex_(wave, n3, 4, qw=(A, A + 2, A), out=(A + 0x1000000, None, None, None)) == c.SF_ENOTBUILT     # not looked at
    assert lib.sf_geom_quad_f32(9, 9, 4, A, A, A, A, A, A, A + 0x100000, A + 0x200002, A + 0x1000000, None, None, None,
                                None) == c.SF_EALIGN
    #     alignment comes before overlap
    assert hex_(wave, n3, 4, b=(A + 4, A, A), out=(A + 0x100000, None, None, None)) == c.SF_EALIGN
    # (5) an output over a coordinate array or another output, as byte ranges of their full sizes
    modes, points = 8 * 4 * 8 ** 3, 8 * 4 * 9 ** 3
    x = (A + 0x100000, A + 0x200000, A + 0x300000)
    for o in range(4):
        for a in range(3):
            out = tuple(x[a] + modes - 8 if k == o else None for k in range(4))
            assert hex_(wave, n3, 4, out=out) == c.SF_EINVAL, (o, a)
            out = tuple(x[a] + modes if k == o else None for k in range(4))        # the next byte: no overlap
            assert hex_(wave, n3, 4, out=out) == c.SF_ENOTBUILT, (o, a)
    base = A + 0x1000000
    assert hex_(wave, n3, 4, out=(base, base + 9 * points - 8, None, None)) == c.SF_EINVAL          # w inside df's last plane
    assert hex_(wave, n3, 4, out=(base, base + 9 * points, None, None)) == c.SF_ENOTBUILT
    assert hex_(wave, n3, 4, out=(None, base + 6 * points - 8, base, None)) == c.SF_EINVAL          # w inside g
    assert hex_(wave, n3, 4, out=(None, base + points - 8, None, base)) == c.SF_EINVAL              # w over detj's end
    assert hex_(wave, n3, 4, out=(None, None, base, base - points + 8)) == c.SF_EINVAL              # detj's end over g
    p2 = 8 * 4 * 17 ** 2
    assert quad(wave, n2, 4, out=(base, base + 4 * p2 - 8, None, None)) == c.SF_EINVAL
    assert quad(wave, n2, 4, out=(base, base + 4 * p2, None, None)) == c.SF_ENOTBUILT
    #     overlap comes before the routes
    assert hex_(thread, (13, 4, 4), 4, out=(x[0], None, None, None)) == c.SF_EINVAL
    # (6) extents beyond the fallback's bounds, then (7) an unsupported variant, "wave" off its table or unaligned
    for v in (0, wave, generic, thread):
        assert hex_(v, (13, 4, 4), 4) == c.SF_ENOTBUILT and quad(v, (33, 5), 4) == c.SF_ENOTBUILT
    for v in ("thread", "block-lds", "block-glb", "mfma", "mfma4", "wave-rt"):
        assert hex_(pkg.VARIANTS[v], (8, 8, 8), 4) == c.SF_ENOTBUILT and quad(pkg.VARIANTS[v], (8, 8), 4) == c.SF_ENOTBUILT
    assert hex_(wave, (6, 6, 12), 4) == c.SF_ENOTBUILT and hex_(wave, n3, 4) == c.SF_ENOTBUILT
    assert quad(wave, n2, 4) == c.SF_ENOTBUILT and quad(wave, (4, 9), 4) == c.SF_ENOTBUILT
    assert hex_(wave, (8, 8, 8), 4, x=(x[0] + 8, x[1], x[2])) == c.SF_EALIGN           # a coordinate only 8-byte aligned
    assert hex_(wave, (8, 8, 8), 4, out=(base, base + 0x2000008, None, None)) == c.SF_EALIGN
    assert quad(wave, (8, 8), 4, out=(None, None, None, base + 8)) == c.SF_EALIGN
    # the affine form: the same order without a variant
    aff = lib.sf_geom_affine_hex_f64
    o3 = (base, base + 0x1000, base + 0x2000)
    assert aff(1, 8, 8, 4, *(A,) * 6, *x, *o3, None) == c.SF_EINVAL
    assert aff(8, 8, 8, 0, *(None,) * 6, *x, *o3, None) == c.SF_OK
    assert aff(8, 8, 8, 4, A, A, None, A, A, A, *x, *o3, None) == c.SF_EINVAL
    assert aff(8, 8, 8, 4, *(A,) * 6, *x, None, None, None, None) == c.SF_EINVAL
    assert aff(8, 8, 8, 4, *(A,) * 6, *x, base + 4, None, None, None) == c.SF_EALIGN
    assert aff(8, 8, 8, 4, *(A,) * 6, *x, None, x[1] + 8 * 4 * 7 ** 3 - 8, None, None) == c.SF_EINVAL
    assert aff(8, 8, 8, 4, *(A,) * 6, *x, base, base + 8 * 4 * 9 - 8, None, None) == c.SF_EINVAL
    assert aff(13, 4, 4, 4, *(A,) * 6, *x, *o3, None) == c.SF_ENOTBUILT
    assert lib.sf_geom_affine_quad_f32(33, 5, 4, *(A,) * 4, x[0], x[1], *o3, None) == c.SF_ENOTBUILT
    assert lib.sf_geom_affine_quad_f64(9, 9, 4, *(A,) * 4, x[0], None, *o3, None) == c.SF_EINVAL


NAME = re.compile(r"(hex|quad)_geom_wave_kernel<(\d+), .*, (\d+), (double|float)>")


def test_wave_instantiations_use_no_scratch():
    """Every wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D nq 2..16
    for double and float, each with the four output masks all (15), df (1), w (2), g and w (6): 176 kernels.  Prints
    VGPRs / occupancy per kernel (the table of DESIGN.md s4.18)."""
    got = set()
    for src, r in kernel_resources(("geom.hip", "geom_f32.hip"), "geom_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, mask, t = 3 if m.group(1) == "hex" else 2, int(m.group(2)), int(m.group(3)), m.group(4)
        assert (t == "float") == (src == "geom_f32.hip"), (src, r.name)
        got.add((dim, nq, t, mask))
        print(f"{dim}D nq {nq:2d} {t:6s} mask {mask:2d}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, mask) for d, n in orders for t in ("double", "float") for mask in (15, 1, 2, 6)}
    assert len(want) == 176 and got == want, sorted(map(str, want ^ got))
