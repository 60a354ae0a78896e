"""CPU-side checks of the weak advection term (include/sumfact.h sf_advect_*): the exports and their Python binding,
argument validation before any HIP call, the refusals of the Python layer, and the test reference (tests/advect_ref.py)
against a dense restatement, against the composition of the references of its parts, against deliberately wrong
variants and against a closed form.  No test here needs a GPU."""
import os
import re

import numpy as np
import pytest

from advect_ref import U64, advect_excess, advect_f64, advect_n, dense_advect, gamma, ref_advect
from geom_ref import deformed, gll_operands, ref_geom
from iprod_ref import iprod_f64, ref_iprod
from physderiv_ref import physderiv_f64, physderiv_n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")
NEW = ["sf_advect_hex_f64", "sf_advect_hex_f64_variant", "sf_advect_quad_f64", "sf_advect_quad_f64_variant",
       "sf_advect_hex_f32", "sf_advect_quad_f32"]
SHAPES = [(3, 3, 3), (4, 3, 5), (4, 4), (5, 3)]
ids = lambda nq: "x".join(str(q) for q in nq)      # noqa: E731


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def case(nq, nelmt, seed, nf=None):
    """Bases, derivative matrices, df, w, c and nf fields, uniform in [-1, 1)."""
    rng = np.random.default_rng(seed)
    d = len(nq)
    nmt, nqt = int(np.prod([q - 1 for q in nq])), int(np.prod(nq))
    B = [rng.uniform(-1, 1, (q - 1) * q) for q in nq]
    D = [rng.uniform(-1, 1, q * q) for q in nq]
    df, w = rng.uniform(-1, 1, nelmt * d * d * nqt), rng.uniform(-1, 1, nelmt * nqt)
    c = [rng.uniform(-1, 1, nelmt * nqt) for _ in range(d)]
    x = [rng.uniform(-1, 1, nelmt * nmt) for _ in range(d if nf is None else nf)]
    return B, D, df, w, c, x


def test_the_count_of_the_bound():
    assert advect_n((8, 8, 8)) == 2 * 24 + 8 + 6 + 1 and advect_n((5, 3)) == 2 * 8 + 5 + 4 + 1
    # the chain sf_physderiv_* -> dot with c -> weight -> sf_iproduct_* makes the same count
    for nq in SHAPES:
        assert advect_n(nq) == physderiv_n(nq) + len(nq) + 1 + sum(nq)


@pytest.mark.parametrize("nq", SHAPES, ids=ids)
def test_reference_against_a_dense_matrix(nq):
    """Two restatements in long double: the sweeps of ref_advect and dense point x mode matrices, element by element and
    field by field.  They differ by long-double rounding only: held to the bound at u = 2^-63."""
    nelmt, d = 3, len(nq)
    nmt, nqt = int(np.prod([q - 1 for q in nq])), int(np.prod(nq))
    B, D, df, w, c, x = case(nq, nelmt, 5)
    for fields in (x, x[-1:]):
        ref, absref = ref_advect(nq, nelmt, B, D, df, w, c, fields)
        assert ref.shape == (len(fields), nelmt * nmt)
        dense = np.stack([np.concatenate([
            dense_advect(nq, B, D, df.reshape(nelmt, -1)[e], w.reshape(nelmt, -1)[e], [v.reshape(nelmt, nqt)[e] for v in c],
                         f.reshape(nelmt, nmt)[e]) for e in range(nelmt)]) for f in fields])
        assert advect_excess(dense, ref, absref, nq, 2.0 ** -63) <= 1.0
        assert float(np.max(np.abs(ref))) > 0
    assert np.array_equal(ref[0], ref_advect(nq, nelmt, B, D, df, w, c, x)[0][d - 1])      # nf = 1 is row a of nf = d


@pytest.mark.parametrize("nq", SHAPES, ids=ids)
def test_reference_against_the_composition_of_its_parts(nq):
    """ref_physderiv -> dot with c -> times w -> ref_iprod, evaluated in fp64: the chain makes N operations on the same
    absolute operator (test_the_count_of_the_bound), so it is within gamma_N absref of the long-double reference, and so
    is the fp64 evaluation of the operator itself; the two are within the sum of the two bounds of each other."""
    nelmt, d = 4, len(nq)
    B, D, df, w, c, x = case(nq, nelmt, 7)
    ref, absref = ref_advect(nq, nelmt, B, D, df, w, c, x)
    own, _ = advect_f64(nq, nelmt, B, D, df, w, c, x)
    chain = []
    for a in range(d):
        grad, _ = physderiv_f64(nq, nelmt, B, D, df, x[a])
        chain.append(iprod_f64(nq, nelmt, B, w * sum(c[j] * grad[j] for j in range(d)))[0])
    chain = np.stack(chain)
    assert advect_excess(own, ref, absref, nq, U64) <= 1.0
    assert advect_excess(chain, ref, absref, nq, U64) <= 1.0
    assert advect_excess(chain, own, absref, nq, U64, factor=2.0) <= 1.0
    own32, _ = advect_f64(nq, nelmt, B, D, df, w, c, x, dt=np.float32)
    r32 = lambda vs: [np.asarray(v, dtype=np.float32).astype(np.float64) for v in vs]      # noqa: E731  inputs rounded
    ref32, abs32 = ref_advect(nq, nelmt, r32(B), r32(D), r32([df])[0], r32([w])[0], r32(c), r32(x))
    assert own32.dtype == np.float32 and advect_excess(own32, ref32, abs32, nq, 2.0 ** -24) <= 1.0


@pytest.mark.parametrize("mutate", ["df-transposed", "c-field-swapped", "no-w"])
@pytest.mark.parametrize("nq", SHAPES, ids=ids)
def test_wrong_variants_exceed_the_bound(nq, mutate):
    nelmt = 4
    B, D, df, w, c, x = case(nq, nelmt, 9)
    ref, absref = ref_advect(nq, nelmt, B, D, df, w, c, x)
    bad, _ = advect_f64(nq, nelmt, B, D, df, w, c, x, mutate=mutate)
    assert advect_excess(bad, ref, absref, nq, U64) > 1e6, mutate


CLOSED_FORM_MEASURED = {(5, 5, 5): 1.34e-19, (9, 9): 1.35e-19}


@pytest.mark.parametrize("nq", [(5, 5, 5), (9, 9)], ids=ids)
def test_closed_form_on_the_elements_own_coordinates(nq):
    """The fields are the element's own modal coordinates on a deformed element, df and w geom_ref's long-double values:
    grad x_a = e_a, so out_a = B^T (w c_a) = ref_iprod(w c_a).  The deviation is the conditioning of the geometry (df is
    the inverse of a Jacobian known to long-double rounding), not a derived quantity: it is measured in long double as
    max |out - iprod| / max |iprod|, and 16 x the measured value is asserted.  Measured: 1.34e-19 at (5, 5, 5),
    1.35e-19 at (9, 9) (long double, eps 2^-63 = 1.08e-19)."""
    nelmt, d = 6, len(nq)
    B, D, Q = gll_operands(nq)
    xs, _ = deformed(nq, nelmt, 12)
    geo = ref_geom(nq, nelmt, B, D, Q, xs, U64)
    df, w = geo.val["df"], geo.val["w"]
    assert df.dtype == np.longdouble and w.dtype == np.longdouble
    rng = np.random.default_rng(3)
    c = [rng.uniform(-1, 1, w.size) for _ in range(d)]
    out, _ = ref_advect(nq, nelmt, B, D, df, w, c, xs)
    worst = 0.0
    for a in range(d):
        want, _ = ref_iprod(nq, nelmt, B, w * np.asarray(c[a], dtype=np.longdouble))
        worst = max(worst, float(np.max(np.abs(out[a] - want)) / np.max(np.abs(want))))
    print(f"closed form {nq}: max |out_a - B^T (w c_a)| / max |B^T (w c_a)| = {worst:.3g}")
    assert worst <= 16 * CLOSED_FORM_MEASURED[tuple(nq)]


def test_advect_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(sf_advect_\w+)\s*\(", code))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_advect_")}
    want = {"sf_advect_hex_f64": 23, "sf_advect_hex_f64_variant": 24, "sf_advect_hex_f32": 23,
            "sf_advect_quad_f64": 17, "sf_advect_quad_f64_variant": 18, "sf_advect_quad_f32": 17}
    for name in NEW:
        assert hasattr(lib, name), name
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]) == want[name], name
    for name in ("advect_hex", "advect_quad"):
        assert callable(getattr(pkg, name)), name
    for needle in ("beta_b   = sum_j c_j[e] * df[e][j*d + b]", "r_a      = w[e] * (sum_b beta_b * J[a][b])",
                   "Any other nf: SF_EINVAL", "All of df, w, c_j are required"):
        assert needle in header, needle


def test_validation_without_a_gpu(pkg):
    """Every rule of the documented order by return code; no call here reaches a launch."""
    lib, c = pkg.capi.lib(), pkg.capi
    A = 0x100000                                                       # 16-byte-aligned dummies, never dereferenced
    wave, generic, thread = pkg.VARIANTS["wave"], pkg.VARIANTS["generic"], pkg.VARIANTS["thread"]
    DF, W, C, X, O = A + 0x1000000, A + 0x3000000, A + 0x4000000, A + 0x8000000, A + 0xC000000
    step = 0x1000000

    def hex_(variant, nq, nelmt, nf=3, b=(A,) * 3, d=(A,) * 3, df=DF, w=W, cs=(C, C + step, C + 2 * step),
             x=(X, X + step, X + 2 * step), out=(O, O + step, O + 2 * step)):
        return lib.sf_advect_hex_f64_variant(variant, *nq, nelmt, nf, *b, *d, df, w, *cs, *x, *out, None)

    def quad(variant, nq, nelmt, nf=2, b=(A,) * 2, d=(A,) * 2, df=DF, w=W, cs=(C, C + step), x=(X, X + step),
             out=(O, O + step)):
        return lib.sf_advect_quad_f64_variant(variant, *nq, nelmt, nf, *b, *d, df, w, *cs, *x, *out, None)

    n3, n2, N3 = (8, 8, 8), (9, 9), (None,) * 3
    # (1) an extent < 2, a variant out of range, nf other than 1 or d -- before everything else
    assert hex_(0, (1, 8, 8), 4) == c.SF_EINVAL and quad(0, (9, 1), 4) == c.SF_EINVAL and hex_(99, n3, 4) == c.SF_EINVAL
    for nf in (0, 2, 4):
        assert hex_(0, n3, 4, nf=nf) == c.SF_EINVAL and hex_(0, n3, 0, nf=nf) == c.SF_EINVAL
    for nf in (0, 3):
        assert quad(0, n2, 4, nf=nf) == c.SF_EINVAL
    # (2) an empty batch, whatever the pointers
    assert hex_(0, n3, 0, b=N3, df=None, out=N3) == c.SF_OK and quad(0, n2, 0, x=(None, None)) == c.SF_OK
    # (3) nulls: df, w, a c_j, a field that the call takes; with nf = 1 the slots beyond are not looked at
    assert hex_(0, n3, 4, df=None) == c.SF_EINVAL and hex_(0, n3, 4, w=None) == c.SF_EINVAL
    assert hex_(0, n3, 4, cs=(C, None, C + step)) == c.SF_EINVAL and quad(0, n2, 4, cs=(C, None)) == c.SF_EINVAL
    assert hex_(0, n3, 4, x=(X, X + step, None)) == c.SF_EINVAL and hex_(0, n3, 4, out=(O, None, O + step)) == c.SF_EINVAL
    assert hex_(0, n3, 4, b=(A, None, A)) == c.SF_EINVAL and hex_(0, n3, 4, d=(A, A, None)) == c.SF_EINVAL
    assert hex_(wave, (9, 9, 9), 4, nf=1, x=(X, None, None), out=(O, None, None)) == c.SF_ENOTBUILT
    assert quad(wave, (17, 17), 4, nf=1, x=(X, None), out=(O, None)) == c.SF_ENOTBUILT
    assert hex_(0, n3, 4, nf=1, x=(None, X, X)) == c.SF_EINVAL
    # (4) scalar alignment, after the nulls
    assert hex_(0, n3, 4, df=DF + 4) == c.SF_EALIGN and hex_(0, n3, 4, cs=(C, C + step + 2, C)) == c.SF_EALIGN
    assert hex_(0, n3, 4, df=DF + 4, w=None) == c.SF_EINVAL
    assert lib.sf_advect_quad_f32(9, 9, 4, 2, A, A, A, A, DF, W + 2, C, C + step, X, X + step, O, O + step, None) == c.SF_EALIGN
    # (5) an output over anything the call reads or another output, as byte ranges of their full sizes
    modes, points = 8 * 4 * 7 ** 3, 8 * 4 * 8 ** 3
    assert hex_(wave, (9, 9, 9), 4, out=(O, O + 8 * 4 * 8 ** 3 - 8, O + step)) == c.SF_EINVAL          # out1 inside out0
    assert hex_(wave, (9, 9, 9), 4, out=(O, O + 8 * 4 * 8 ** 3, O + step)) == c.SF_ENOTBUILT
    for what, base, size in (("df", DF, 9 * points), ("w", W, points), ("c1", C + step, points), ("in2", X + 2 * step, modes)):
        for a in range(3):
            out = tuple(base + size - 8 if k == a else O + k * step for k in range(3))
            assert hex_(generic, n3, 4, out=out) == c.SF_EINVAL, (what, a)
            out = tuple(base - modes + 8 if k == a else O + k * step for k in range(3))
            assert hex_(generic, n3, 4, out=out) == c.SF_EINVAL, (what, a)
    assert hex_(thread, (13, 4, 4), 4, out=(X, O, O + step)) == c.SF_EINVAL                           # before the routes
    assert hex_(wave, (9, 9, 9), 4, nf=1, out=(O, X, DF)) == c.SF_ENOTBUILT                           # slots beyond nf: not looked at
    # (6) extents beyond the fallback's bounds, then (7) an unsupported variant, "wave" off its table or unaligned
    for v in (0, wave, generic, thread):
        assert hex_(v, (13, 2, 2), 4) == c.SF_ENOTBUILT and quad(v, (33, 2), 4) == c.SF_ENOTBUILT
    for v in ("thread", "block-lds", "block-glb", "mfma", "mfma4", "wave-rt"):
        assert hex_(pkg.VARIANTS[v], n3, 4) == c.SF_ENOTBUILT and quad(pkg.VARIANTS[v], (8, 8), 4) == c.SF_ENOTBUILT
    assert hex_(wave, (6, 6, 12), 4) == c.SF_ENOTBUILT and hex_(wave, (9, 9, 9), 4) == c.SF_ENOTBUILT
    assert quad(wave, (17, 17), 4) == c.SF_ENOTBUILT
    assert hex_(wave, n3, 4, x=(X + 8, X + step, X + 2 * step)) == c.SF_EALIGN                        # a field only 8-byte aligned
    assert hex_(wave, n3, 4, out=(O, O + step + 8, O + 2 * step)) == c.SF_EALIGN


def test_the_python_layer_refuses_without_a_device(pkg):
    """nf other than 1 or d, sizes and overlapping buffers are refused before any pointer reaches the library: host
    tensors are enough to show it."""
    import torch
    nq, nelmt = (4, 4, 4), 3
    nmt, nqt = 27, 64
    t = lambda n: torch.zeros(n, dtype=torch.float64)                  # noqa: E731
    bs, ds = [t(12)] * 3, [t(16)] * 3
    df, w, c = t(nelmt * 9 * nqt), t(nelmt * nqt), torch.zeros((3, nelmt * nqt), dtype=torch.float64)
    x = torch.zeros((3, nelmt * nmt), dtype=torch.float64)
    for bad in (x[:2], [x[0], x[1]], torch.zeros((4, nelmt * nmt), dtype=torch.float64)):
        with pytest.raises(pkg.capi.SumfactError) as ei:
            pkg.advect_hex(nq, *bs, *ds, df, w, c, bad)
        assert ei.value.rc == pkg.capi.SF_EINVAL
    with pytest.raises(pkg.capi.SumfactError) as ei:
        pkg.advect_quad((4, 4), *bs[:2], *ds[:2], t(nelmt * 4 * 16), t(nelmt * 16), torch.zeros((2, nelmt * 16)), x)
    assert ei.value.rc == pkg.capi.SF_EINVAL
    for out in (x, [x[0], t(nelmt * nmt), t(nelmt * nmt)], [t(nelmt * nmt), w[:nelmt * nmt], t(nelmt * nmt)],
                [t(nelmt * nmt), t(nelmt * nmt), c[2][5:5 + nelmt * nmt]]):
        with pytest.raises(pkg.capi.SumfactError) as ei:
            pkg.advect_hex(nq, *bs, *ds, df, w, c, x, out=out)
        assert ei.value.rc == pkg.capi.SF_EINVAL
    o = t(nelmt * nmt)
    with pytest.raises(pkg.capi.SumfactError) as ei:
        pkg.advect_hex(nq, *bs, *ds, df, w, c, x, out=[o, o, t(nelmt * nmt)])
    assert ei.value.rc == pkg.capi.SF_EINVAL
    with pytest.raises(ValueError):
        pkg.advect_hex(nq, *bs, *ds, df[:-1], w, c, x)
    with pytest.raises(ValueError):
        pkg.advect_hex(nq, *bs, *ds, df, w, c[:2], x)
    with pytest.raises(ValueError):
        pkg.advect_hex(nq, *bs, *ds, df, w, c, x.float())
