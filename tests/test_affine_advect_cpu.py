"""CPU tests of the weak advection term on affine elements (include/sumfact.h sf_aff_advect_*): the reference of
tests/affine_advect_ref.py against the deformed reference on expanded planes, fp64 and fp32 evaluations inside the bound
and wrong variants outside it (the tests can fail), the weight association that the GPU bit-equality rests on, the count
of the bound, the exports and their Python binding, argument validation before any HIP call, the refusals of the Python
layer, and the registers of every wave instantiation.  No test here needs a GPU."""
import math
import os
import re

import numpy as np
import pytest

from advect_ref import advect_n, ref_advect
from affine_advect_ref import (U32, U64, affine_advect_eval, affine_advect_excess, affine_advect_n, expand_df, expand_w,
                               ref_affine_advect)
from affine_deriv_ref import affine_iprodderiv_n
from iprodderiv_ref import iprodderiv_n
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")
ULD = float(np.finfo(np.longdouble).eps) / 2                    # unit roundoff of the reference's own arithmetic
NEW = [f"sf_aff_advect_{shape}_{sfx}" for shape in ("hex", "quad") for sfx in ("f64", "f64_variant", "f32")]
SHAPES = [(3, 3, 3), (4, 3, 5), (4, 4), (5, 3)]
ids = lambda nq: "x".join(str(q) for q in nq)      # noqa: E731


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def case(nq, nelmt, seed):
    """Bases, derivative matrices, quadrature weights, dfe, je, c and d fields, uniform in [-1, 1)."""
    rng = np.random.default_rng(seed)
    d = len(nq)
    nmt, nqt = int(np.prod([q - 1 for q in nq])), int(np.prod(nq))
    u = lambda n: rng.uniform(-1, 1, n)      # noqa: E731
    return dict(B=[u((q - 1) * q) for q in nq], D=[u(q * q) for q in nq], Q=[u(q) for q in nq], dfe=u(nelmt * d * d),
                je=u(nelmt), c=[u(nelmt * nqt) for _ in range(d)], x=[u(nelmt * nmt) for _ in range(d)])


def test_the_count_of_the_bound():
    """advect_n plus the products that form the weight from je and the qw_d: d - 1 for q and one for je q; the product
    with the sum is the one advect_n holds.  The step affine_iprodderiv_n takes over iprodderiv_n."""
    for nq in SHAPES + [(8, 8, 8), (16, 16)]:
        d = len(nq)
        assert affine_advect_n(nq, True) == advect_n(nq) + (d - 1) + 1 == 2 * sum(nq) + max(nq) + 3 * d + 1
        assert affine_advect_n(nq, True) - advect_n(nq) == affine_iprodderiv_n(nq) - iprodderiv_n(nq)
        assert affine_advect_n(nq, False) == affine_advect_n(nq, True)      # kept where the weight does not happen
    assert affine_advect_n((8, 8, 8)) == 48 + 8 + 9 + 1 and affine_advect_n((5, 3)) == 16 + 5 + 6 + 1
    assert math.isinf(affine_advect_excess(np.ones(1), np.zeros(1), np.zeros(1), (8, 8), U64))


@pytest.mark.parametrize("with_je", [True, False], ids=["je", "no-je"])
@pytest.mark.parametrize("nq", SHAPES, ids=ids)
def test_reference_is_the_deformed_one_on_expanded_planes(nq, with_je):
    """Long double against long double: the two restatements do the same operations, so they agree within the rounding of
    the reference's own arithmetic, gamma_N(2^-64) absref.  Without je the deformed weight is a plane of ones."""
    nelmt, k = 5, case(nq, 5, 1)
    je = k["je"] if with_je else None
    npt = int(np.prod(nq))
    w = expand_w(nq, nelmt, k["Q"], je) if with_je else np.ones(nelmt * npt, dtype=np.longdouble)
    for fields in (k["x"], k["x"][-1:]):
        ref, absref = ref_affine_advect(nq, nelmt, k["B"], k["D"], k["Q"], k["dfe"], je, k["c"], fields)
        want, wabs = ref_advect(nq, nelmt, k["B"], k["D"], expand_df(nq, nelmt, k["dfe"]), w, k["c"], fields)
        assert ref.shape == want.shape == (len(fields), nelmt * int(np.prod([q - 1 for q in nq])))
        assert affine_advect_excess(ref, want, wabs, nq, ULD) <= 1.0
        assert affine_advect_excess(absref, wabs, wabs, nq, ULD) <= 1.0
        assert float(np.max(np.abs(want))) > 0
    full, _ = ref_affine_advect(nq, nelmt, k["B"], k["D"], k["Q"], k["dfe"], je, k["c"], k["x"])
    assert np.array_equal(ref[0], full[len(nq) - 1])                        # nf = 1 is row a of nf = d


def _rounded(k, dt):
    r = lambda a: [np.asarray(v, dtype=dt).astype(np.float64) for v in a]      # noqa: E731  inputs rounded to dt
    return dict(B=r(k["B"]), D=r(k["D"]), Q=r(k["Q"]), dfe=r([k["dfe"]])[0], je=r([k["je"]])[0], c=r(k["c"]), x=r(k["x"]))


@pytest.mark.parametrize("with_je", [True, False], ids=["je", "no-je"])
@pytest.mark.parametrize("nq", SHAPES + [(8, 8, 8), (12, 12)], ids=ids)
def test_fp64_and_fp32_evaluations_meet_the_bound(nq, with_je):
    """The documented order of operations in fp64 and fp32 (numpy) is inside gamma_N absref of the long-double reference
    on the inputs rounded to the working precision."""
    nelmt, k = 6, case(nq, 6, 4)
    for dt, u in ((np.float64, U64), (np.float32, U32)):
        r = _rounded(k, dt)
        je = r["je"] if with_je else None
        ref, absref = ref_affine_advect(nq, nelmt, r["B"], r["D"], r["Q"], r["dfe"], je, r["c"], r["x"])
        got = affine_advect_eval(nq, nelmt, r["B"], r["D"], r["Q"], r["dfe"], je, r["c"], r["x"], dt)
        assert got.dtype == dt
        q = affine_advect_excess(got, ref, absref, nq, u, with_je=with_je)
        print(f"{nq} {np.dtype(dt).name} {'je' if with_je else 'no je'}: {q:.3g} of the bound")
        assert q <= 1.0


@pytest.mark.parametrize("nq", SHAPES + [(5, 3, 5)], ids=ids)
def test_wrong_variants_exceed_the_bound(nq):
    """A transposed dfe, swapped planes of c, a weight that leaves one direction out, and -- where two directions have the
    same extent, so that their weights can change places: (3, 3, 3), (4, 4) and the anisotropic (5, 3, 5) -- swapped
    quadrature weights are outside the bound by orders of magnitude: the bound can tell."""
    nelmt, k = 4, case(nq, 4, 9)
    d = len(nq)
    args = (nq, nelmt, k["B"], k["D"], k["Q"], k["dfe"], k["je"])
    ref, absref = ref_affine_advect(*args, k["c"], k["x"])
    bad = {m: affine_advect_eval(*args, k["c"], k["x"], np.float64, mutate=m) for m in ("dfe-transposed", "weight-short")}
    bad["c-swapped"] = affine_advect_eval(*args, [k["c"][1], k["c"][0]] + k["c"][2:], k["x"], np.float64)
    if len(set(nq)) < d:
        bad["qw-swapped"] = affine_advect_eval(*args, k["c"], k["x"], np.float64, mutate="qw-swapped")
    assert ("qw-swapped" in bad) == (tuple(nq) in ((3, 3, 3), (4, 4), (5, 3, 5)))
    for m, got in bad.items():
        assert affine_advect_excess(got, ref, absref, nq, U64) > 1e6, m
    assert affine_advect_excess(affine_advect_eval(*args, k["c"], k["x"], np.float64), ref, absref, nq, U64) <= 1.0


def test_weight_association_defines_the_bits():
    """w = je * (qw2 * (qw1 * qw0)) in the working precision: another association rounds differently somewhere -- in the
    weight plane and in the operator's result -- while staying inside the bound.  The bit-equality tests of the GPU files
    depend on this one (and can fail)."""
    nq, nelmt = (8, 8, 8), 11
    k = case(nq, nelmt, 5)
    for dt, u in ((np.float64, U64), (np.float32, U32)):
        r = _rounded(k, dt)
        q = [np.asarray(v, dtype=dt) for v in r["Q"]]
        je = np.asarray(r["je"], dtype=dt)
        w = expand_w(nq, nelmt, q, je, dt)
        assert w.dtype == dt
        kk, j, i = 5, 3, 6
        assert w.reshape(nelmt, 8, 8, 8)[4, kk, j, i] == je[4] * (q[2][kk] * (q[1][j] * q[0][i]))
        other = ((je.reshape(-1, 1, 1, 1) * q[2].reshape(1, -1, 1, 1)) * q[1].reshape(1, 1, -1, 1)) * q[0].reshape(1, 1, 1, -1)
        assert not np.array_equal(w, other.reshape(-1))
        args = (nq, nelmt, r["B"], r["D"], r["Q"], r["dfe"], r["je"], r["c"], r["x"])
        own = affine_advect_eval(*args, dt)
        left = affine_advect_eval(*args, dt, mutate="weight-left")
        assert own.dtype == left.dtype == dt and not np.array_equal(own, left)
        ref, absref = ref_affine_advect(*args)
        assert affine_advect_excess(left, ref, absref, nq, u) <= 1.0


def test_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(sf_aff_advect_\w+)\s*\(", code))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_aff_advect_")}
    want = {"sf_aff_advect_hex_f64": 26, "sf_aff_advect_hex_f64_variant": 27, "sf_aff_advect_hex_f32": 26,
            "sf_aff_advect_quad_f64": 19, "sf_aff_advect_quad_f64_variant": 20, "sf_aff_advect_quad_f32": 19}
    for name in NEW:
        assert hasattr(lib, name), name
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]) == want[name], name
    for name in ("affine_advect_hex", "affine_advect_quad"):
        assert callable(getattr(pkg, name)), name
    for needle in ("beta_b   = sum_j c_j[e][pt] * dfe[e][j*d + b]", "r_a      = (je[e] * q) * (sum_b beta_b * J[a][b])",
                   "q        = qw2[k] * (qw1[j] * qw0[i])", "je * (qw2 * (qw1 * qw0))", "w a plane of ones",
                   "je and every qw_d are then never read (nor\n * validated)", "Any other nf: SF_EINVAL"):
        assert needle in header, needle


def test_validation_without_a_gpu(pkg):
    """Every rule of the documented order by return code; no call here reaches a launch."""
    lib, c = pkg.capi.lib(), pkg.capi
    A = 0x100000                                                       # 16-byte-aligned dummies, never dereferenced
    wave, generic, thread = pkg.VARIANTS["wave"], pkg.VARIANTS["generic"], pkg.VARIANTS["thread"]
    QW, DFE, JE, C, X, O = A + 0x1000, A + 0x1000000, A + 0x3000000, A + 0x4000000, A + 0x8000000, A + 0xC000000
    step = 0x1000000

    def hex_(variant, nq, nelmt, nf=3, b=(A,) * 3, d=(A,) * 3, qw=(QW,) * 3, dfe=DFE, je=JE, cs=(C, C + step, C + 2 * step),
             x=(X, X + step, X + 2 * step), out=(O, O + step, O + 2 * step)):
        return lib.sf_aff_advect_hex_f64_variant(variant, *nq, nelmt, nf, *b, *d, *qw, dfe, je, *cs, *x, *out, None)

    def quad(variant, nq, nelmt, nf=2, b=(A,) * 2, d=(A,) * 2, qw=(QW,) * 2, dfe=DFE, je=JE, cs=(C, C + step),
             x=(X, X + step), out=(O, O + step)):
        return lib.sf_aff_advect_quad_f64_variant(variant, *nq, nelmt, nf, *b, *d, *qw, dfe, je, *cs, *x, *out, None)

    n3, n2, N3 = (8, 8, 8), (9, 9), (None,) * 3
    off = (9, 9, 9)                           # off the wave table: SF_VARIANT_WAVE answers SF_ENOTBUILT after steps 1-5
    # (1) an extent < 2, a variant out of range, nf other than 1 or d -- before everything else
    assert hex_(0, (1, 8, 8), 4) == c.SF_EINVAL and quad(0, (9, 1), 4) == c.SF_EINVAL and hex_(99, n3, 4) == c.SF_EINVAL
    for nf in (0, 2, 4):
        assert hex_(0, n3, 4, nf=nf) == c.SF_EINVAL and hex_(0, n3, 0, nf=nf) == c.SF_EINVAL
    for nf in (0, 3):
        assert quad(0, n2, 4, nf=nf) == c.SF_EINVAL
    # (2) an empty batch, whatever the pointers
    assert hex_(0, n3, 0, b=N3, dfe=None, out=N3) == c.SF_OK and quad(0, n2, 0, x=(None, None)) == c.SF_OK
    # (3) nulls: dfe, a c_j, a field that the call takes, a basis, a derivative matrix; qw_d only with je
    assert hex_(0, n3, 4, dfe=None) == c.SF_EINVAL and quad(0, n2, 4, dfe=None) == c.SF_EINVAL
    assert hex_(0, n3, 4, cs=(C, None, C + step)) == c.SF_EINVAL and quad(0, n2, 4, cs=(C, None)) == c.SF_EINVAL
    assert hex_(0, n3, 4, x=(X, X + step, None)) == c.SF_EINVAL and hex_(0, n3, 4, out=(O, None, O + step)) == c.SF_EINVAL
    assert hex_(0, n3, 4, b=(A, None, A)) == c.SF_EINVAL and hex_(0, n3, 4, d=(A, A, None)) == c.SF_EINVAL
    assert hex_(0, n3, 4, qw=(QW, None, QW)) == c.SF_EINVAL and quad(0, n2, 4, qw=(None, QW)) == c.SF_EINVAL
    # je = NULL: no weight; je and the qw_d are not looked at -- null or misaligned, the call goes on to the routes
    assert hex_(wave, off, 4, je=None, qw=N3) == c.SF_ENOTBUILT
    assert hex_(wave, off, 4, je=None, qw=(QW + 1, QW + 3, None)) == c.SF_ENOTBUILT
    assert quad(wave, (17, 17), 4, je=None, qw=(None, QW + 2)) == c.SF_ENOTBUILT
    assert lib.sf_aff_advect_quad_f32(17, 33, 4, 2, A, A, A, A, None, QW + 1, DFE, None, C, C + step, X, X + step, O, O + step,
                                      None) == c.SF_ENOTBUILT
    assert hex_(0, n3, 4, je=None, dfe=None) == c.SF_EINVAL                                           # dfe stays required
    # nf = 1: the slots beyond are not looked at
    assert hex_(wave, off, 4, nf=1, x=(X, None, None), out=(O, None, None)) == c.SF_ENOTBUILT
    assert quad(wave, (17, 17), 4, nf=1, x=(X, None), out=(O, None)) == c.SF_ENOTBUILT
    assert hex_(wave, off, 4, nf=1, x=(X, X + 1, X + 2), out=(O, O + 1, O + 3)) == c.SF_ENOTBUILT
    assert hex_(0, n3, 4, nf=1, x=(None, X, X)) == c.SF_EINVAL
    # (4) scalar alignment, after the nulls
    assert hex_(0, n3, 4, dfe=DFE + 4) == c.SF_EALIGN and hex_(0, n3, 4, cs=(C, C + step + 2, C)) == c.SF_EALIGN
    assert hex_(0, n3, 4, je=JE + 4) == c.SF_EALIGN and hex_(0, n3, 4, qw=(QW, QW, QW + 4)) == c.SF_EALIGN
    assert quad(0, n2, 4, qw=(QW + 2, QW)) == c.SF_EALIGN
    assert hex_(0, n3, 4, dfe=DFE + 4, cs=(C, None, C)) == c.SF_EINVAL
    assert lib.sf_aff_advect_quad_f32(9, 9, 4, 2, A, A, A, A, QW, QW, DFE, JE + 2, C, C + step, X, X + step, O, O + step,
                                      None) == c.SF_EALIGN
    # (5) an output over anything the call reads or another output, as byte ranges of their full sizes
    modes, points = 8 * 4 * 7 ** 3, 8 * 4 * 8 ** 3
    assert hex_(wave, off, 4, out=(O, O + 8 * 4 * 8 ** 3 - 8, O + step)) == c.SF_EINVAL                # out1 inside out0
    assert hex_(wave, off, 4, out=(O, O + 8 * 4 * 8 ** 3, O + step)) == c.SF_ENOTBUILT
    for what, base, size in (("dfe", DFE, 8 * 4 * 9), ("je", JE, 8 * 4), ("c1", C + step, points), ("in2", X + 2 * step, modes)):
        for a in range(3):
            out = tuple(base + size - 8 if k == a else O + k * step for k in range(3))
            assert hex_(generic, n3, 4, out=out) == c.SF_EINVAL, (what, a)
            out = tuple(base - modes + 8 if k == a else O + k * step for k in range(3))
            assert hex_(generic, n3, 4, out=out) == c.SF_EINVAL, (what, a)
    for base, size in ((DFE, 8 * 4 * 9), (JE, 8 * 4)):                                                # one past the end: fine
        assert hex_(wave, off, 4, out=(base + size, O + step, O + 2 * step)) == c.SF_ENOTBUILT
    assert hex_(wave, off, 4, je=None, out=(JE, O, O + step)) == c.SF_ENOTBUILT                       # je = NULL is not read
    assert hex_(thread, (13, 4, 4), 4, out=(X, O, O + step)) == c.SF_EINVAL                           # before the routes
    assert hex_(wave, off, 4, nf=1, out=(O, X, DFE)) == c.SF_ENOTBUILT                                # slots beyond nf: not looked at
    # (6) extents beyond the fallback's bounds, then (7) an unsupported variant, "wave" off its table or unaligned
    for v in (0, wave, generic, thread):
        assert hex_(v, (13, 2, 2), 4) == c.SF_ENOTBUILT and quad(v, (33, 2), 4) == c.SF_ENOTBUILT
    for v in ("thread", "block-lds", "block-glb", "mfma", "mfma4", "wave-rt"):
        assert hex_(pkg.VARIANTS[v], n3, 4) == c.SF_ENOTBUILT and quad(pkg.VARIANTS[v], (8, 8), 4) == c.SF_ENOTBUILT
    assert hex_(wave, (6, 6, 12), 4) == c.SF_ENOTBUILT and hex_(wave, off, 4) == c.SF_ENOTBUILT
    assert quad(wave, (17, 17), 4) == c.SF_ENOTBUILT
    assert hex_(wave, n3, 4, x=(X + 8, X + step, X + 2 * step)) == c.SF_EALIGN                        # a field only 8-byte aligned
    assert hex_(wave, n3, 4, out=(O, O + step + 8, O + 2 * step)) == c.SF_EALIGN
    assert quad(wave, (8, 8), 4, je=None, qw=(None, None), out=(O + 8, O + step)) == c.SF_EALIGN


def test_the_python_layer_refuses_without_a_device(pkg):
    """nf other than 1 or d, sizes and overlapping buffers are refused before any pointer reaches the library: host
    tensors are enough to show it."""
    import torch
    nq, nelmt = (4, 4, 4), 3
    nmt, nqt = 27, 64
    t = lambda n: torch.zeros(n, dtype=torch.float64)                  # noqa: E731
    bs, ds, qs = [t(12)] * 3, [t(16)] * 3, [t(4)] * 3
    dfe, je, c = t(nelmt * 9), t(nelmt), torch.zeros((3, nelmt * nqt), dtype=torch.float64)
    x = torch.zeros((3, nelmt * nmt), dtype=torch.float64)
    for bad in (x[:2], [x[0], x[1]], torch.zeros((4, nelmt * nmt), dtype=torch.float64)):
        with pytest.raises(pkg.capi.SumfactError) as ei:
            pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, je, c, bad)
        assert ei.value.rc == pkg.capi.SF_EINVAL
    with pytest.raises(pkg.capi.SumfactError) as ei:
        pkg.affine_advect_quad((4, 4), *bs[:2], *ds[:2], *qs[:2], t(nelmt * 4), je, torch.zeros((2, nelmt * 16)), x)
    assert ei.value.rc == pkg.capi.SF_EINVAL
    big = t(nelmt * nmt + 16)
    for out in (x, [x[0], t(nelmt * nmt), t(nelmt * nmt)], [t(nelmt * nmt), t(nelmt * nmt), c[2][5:5 + nelmt * nmt]]):
        with pytest.raises(pkg.capi.SumfactError) as ei:
            pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, je, c, x, out=out)
        assert ei.value.rc == pkg.capi.SF_EINVAL
    for name, shared in (("dfe", big[:nelmt * 9]), ("je", big[4:4 + nelmt])):                          # an output over dfe / je
        kw = dict(dfe=dfe, je=je)
        kw[name] = shared
        with pytest.raises(pkg.capi.SumfactError) as ei:
            pkg.affine_advect_hex(nq, *bs, *ds, *qs, kw["dfe"], kw["je"], c, x,
                                  out=[big[:nelmt * nmt], t(nelmt * nmt), t(nelmt * nmt)])
        assert ei.value.rc == pkg.capi.SF_EINVAL
    o = t(nelmt * nmt)
    with pytest.raises(pkg.capi.SumfactError) as ei:
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, je, c, x, out=[o, o, t(nelmt * nmt)])
    assert ei.value.rc == pkg.capi.SF_EINVAL
    with pytest.raises(ValueError):
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe[:-1], je, c, x)
    with pytest.raises(ValueError):
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, t(nelmt + 1), c, x)
    with pytest.raises(ValueError):
        pkg.affine_advect_hex(nq, *bs, *ds, qs[0], t(5), qs[2], dfe, je, c, x)
    with pytest.raises(ValueError):
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, je, c[:2], x)
    with pytest.raises(ValueError):
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, dfe, je, c, x.float())
    with pytest.raises(TypeError):
        pkg.affine_advect_hex(nq, *bs, *ds, *qs, None, je, c, x)                                        # dfe is required
    with pytest.raises(TypeError):
        pkg.affine_advect_hex(nq, *bs, *ds, None, qs[1], qs[2], dfe, je, c, x)                          # qw_d with je


NAME = re.compile(r"(hex|quad)_affine_advect_wave_kernel<(\d+), .*, (\d+), (true|false), (float|double)>")


def test_wave_instantiations_use_no_scratch():
    """Every wave instantiation of the family, from the compiler's resource report of the two translation units: no
    scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D nq 2..16 for double and float, one field
    and d, with and without je (176).  Prints VGPRs / occupancy per kernel (the table of DESIGN.md s4.21)."""
    got = set()
    for src, r in kernel_resources(("affine_advect.hip", "affine_advect_f32.hip"), "advect_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, nf, hasw, t = 3 if m.group(1) == "hex" else 2, int(m.group(2)), int(m.group(3)), m.group(4) == "true", m.group(5)
        assert (t == "float") == (src == "affine_advect_f32.hip"), (src, r.name)
        assert (dim, nq, t, nf, hasw) not in got, r.name
        got.add((dim, nq, t, nf, hasw))
        print(f"{dim}D nq {nq:2d} {t:6s} nf {nf} {'je' if hasw else '--'}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, "
              f"occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, nf, h) for d, n in orders for t in ("double", "float") for nf in (1, d) for h in (True, False)}
    assert len(want) == 176 and got == want, sorted(map(str, want ^ got))
