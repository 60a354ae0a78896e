"""CPU-side checks of BwdTrans fused with the physical-space gradient (include/sumfact.h sf_physderiv_*): the exports and
their Python binding, argument validation before any HIP call (NULL df accepted, the overlap refusals among the outputs
and against the inputs), the Python size / dtype / out= checks, the test reference (tests/physderiv_ref.py) against a
dense einsum restatement, against tests/helm_ref.py's Laplacian energy and against an analytic gradient, and the
register / scratch budget of every wave instantiation (hipcc cross-compiles, no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from helm_ref import COMPONENTS, per_element_dots, ref_helmholtz, symmetry_bound
from physderiv_ref import (U32, U64, _physderiv, analytic_case, dense_physderiv, gamma, physderiv_excess, physderiv_f64,
                           physderiv_n, ref_physderiv)
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

NEW = ["sf_physderiv_hex_f64", "sf_physderiv_hex_f64_variant", "sf_physderiv_quad_f64", "sf_physderiv_quad_f64_variant",
       "sf_physderiv_hex_f32", "sf_physderiv_quad_f32"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def test_physderiv_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the header and the binding agree on every sf_physderiv_* name, and on the number of arguments of each
    declared = set(re.findall(r"\b(sf_physderiv_\w+)\s*\(", header))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_physderiv_")}
    want = {"sf_physderiv_hex_f64": 16, "sf_physderiv_hex_f64_variant": 17, "sf_physderiv_hex_f32": 16,
            "sf_physderiv_quad_f64": 12, "sf_physderiv_quad_f64_variant": 13, "sf_physderiv_quad_f32": 12}
    for name in NEW:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]) == want[name], name
    for name in ("physderiv_hex", "physderiv_quad"):
        assert callable(getattr(pkg, name)), name


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, extents, nelmt, (b0, b1, b2), (d0, d1, d2), df, in, (o0, o1, o2)))."""
    def hex64(v, e, n, b, d, df, i, o):
        return lib.sf_physderiv_hex_f64_variant(v, *e, n, *b, *d, df, i, *o, None)

    def quad64(v, e, n, b, d, df, i, o):
        return lib.sf_physderiv_quad_f64_variant(v, *e[:2], n, *b[:2], *d[:2], df, i, *o[:2], None)

    def hex32(v, e, n, b, d, df, i, o):
        assert v == 0
        return lib.sf_physderiv_hex_f32(*e, n, *b, *d, df, i, *o, None)

    def quad32(v, e, n, b, d, df, i, o):
        assert v == 0
        return lib.sf_physderiv_quad_f32(*e[:2], n, *b[:2], *d[:2], df, i, *o[:2], None)

    return [("hex64", 3, 8, hex64), ("quad64", 2, 8, quad64), ("hex32", 3, 4, hex32), ("quad32", 2, 4, quad32)]


def test_physderiv_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call, so it is testable on a machine without a GPU.  One block per step of
    the validation order of include/sumfact.h."""
    lib = pkg.capi.lib()
    # fake device addresses, far enough apart for 10 elements of 8^3 (df: 368 640 bytes, an output 40 960): never touched
    B0, B1, B2, D0, D1, D2 = 0x10000, 0x11000, 0x12000, 0x13000, 0x14000, 0x15000
    DF, IN, O0, O1, O2 = 0x100000, 0x300000, 0x400000, 0x500000, 0x600000
    BS, DS, OS = (B0, B1, B2), (D0, D1, D2), (O0, O1, O2)
    N = (None, None, None)
    for name, dim, size, f in _calls(lib):
        ok = (8, 8, 8)
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(0, bad, 10, BS, DS, DF, IN, OS) == EINVAL, (name, bad)
            assert f(0, bad, 0, N, N, None, None, N) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(0, ok, 0, N, N, None, None, N) == 0, name
        # (3) each null pointer; df may be null
        for d in range(dim):
            bs = tuple(None if x == d else BS[x] for x in range(3))
            ds = tuple(None if x == d else DS[x] for x in range(3))
            os_ = tuple(None if x == d else OS[x] for x in range(3))
            assert f(0, ok, 10, bs, DS, DF, IN, OS) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, ds, DF, IN, OS) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, os_) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, None, IN, os_) == EINVAL, (name, d)
        assert f(0, ok, 10, BS, DS, DF, None, OS) == EINVAL, name
        # ... df == NULL passes (3) and (4): with an odd `in` the call reaches step (4), with sound arguments step (6)
        assert f(0, ok, 10, BS, DS, None, IN + 1, OS) == EALIGN, name
        big = 13 if dim == 3 else 33
        assert f(0, (big, 8, 8), 10, BS, DS, None, IN, OS) == ENOTBUILT, name
        # (3) before (4)
        assert f(0, ok, 10, BS, DS, DF + 1, None, OS) == EINVAL, name
        # (4) each odd address; df only if it is not null
        for d in range(dim):
            bs = tuple(BS[x] + 1 if x == d else BS[x] for x in range(3))
            ds = tuple(DS[x] + 1 if x == d else DS[x] for x in range(3))
            os_ = tuple(OS[x] + 1 if x == d else OS[x] for x in range(3))
            assert f(0, ok, 10, bs, DS, DF, IN, OS) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, ds, DF, IN, OS) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, os_) == EALIGN, (name, d)
        assert f(0, ok, 10, BS, DS, DF + 1, IN, OS) == EALIGN, name
        assert f(0, ok, 10, BS, DS, DF, IN + 1, OS) == EALIGN, name
        # (5) overlap of every out_a with in, with df (its first and its last plane), with another output
        modes = size * 10 * 7 ** dim
        points = size * 10 * 8 ** dim
        for d in range(dim):
            def at(addr):
                return tuple(addr if x == d else OS[x] for x in range(3))
            assert f(0, ok, 10, BS, DS, DF, IN, at(IN)) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, at(IN + modes - 16)) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, at(IN - points + 16)) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, at(DF)) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, IN, at(DF + dim * dim * points - 16)) == EINVAL, (name, d)  # the last plane
            assert f(0, ok, 10, BS, DS, DF, IN, at(DF - points + 16)) == EINVAL, (name, d)
            other = OS[(d + 1) % dim]
            assert f(0, ok, 10, BS, DS, DF, IN, at(other)) == EINVAL, (name, d)                           # out_a == out_b
            assert f(0, ok, 10, BS, DS, DF, IN, at(other + points - 16)) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, None, IN, at(other)) == EINVAL, (name, d)
            # ... with df == NULL the range of df is no argument at all
            assert f(0, (big, 8, 8), 10, BS, DS, None, IN, at(DF)) == ENOTBUILT, (name, d)
            # ... the ranges just touch: accepted by (5), refused by (6) only
            assert f(0, (big, 8, 8), 10, BS, DS, DF, IN, at(DF + dim * dim * size * 10 * big * 8 ** (dim - 1))) == ENOTBUILT, (name, d)
        # ... and overlap is refused before the extent bounds and the variant are looked at
        assert f(0, (big, 8, 8), 10, BS, DS, DF, IN, (O0, O0, O2) if dim == 3 else (O0, O0, None)) == EINVAL, name
        assert f(0, (big, 8, 8), 10, BS, DS, DF, IN, (IN, O1, O2)) == EINVAL, name
        # (6) extents above the fallback's bounds
        for ext in ((big, 8, 8), (8, big, 8)) + (((8, 8, big),) if dim == 3 else ()):
            assert f(0, ext, 10, BS, DS, DF, IN, OS) == ENOTBUILT, (name, ext)
    for name, dim, size, f in _calls(lib)[:2]:
        # (1) variant out of range
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, BS, DS, DF, IN, OS) == EINVAL, (name, v)
        assert f(-1, (8, 8, 8), 0, N, N, None, None, N) == EINVAL, name
        # (5) before (7)
        assert f(2, (8, 8, 8), 10, BS, DS, DF, IN, (O0, O0, O0)) == EINVAL, name
        # (7) the variants that have no fused kernel: thread, block-lds, block-glb, mfma, mfma4, wave-rt
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, (8, 8, 8), 10, BS, DS, DF, IN, OS) == ENOTBUILT, (name, v)
            assert f(v, (8, 8, 8), 10, BS, DS, None, IN, OS) == ENOTBUILT, (name, v)
        # the inputs may overlap each other (all are only read): the call reaches step (7)
        assert f(2, (8, 8, 8), 10, (B0, B0, B0), (B0, B0, B0), DF, DF, OS) == ENOTBUILT, name
        # WAVE off its table (anisotropic, or above nq 8 / 16) and WAVE on 8-byte-aligned in / out_a
        assert f(1, (6, 6, 12) if dim == 3 else (4, 9, 0), 10, BS, DS, DF, IN, OS) == ENOTBUILT, name
        assert f(1, (9, 9, 9) if dim == 3 else (17, 17, 17), 10, BS, DS, DF, IN, OS) == ENOTBUILT, name
        assert f(1, (8, 8, 8), 10, BS, DS, DF, IN + 8, OS) == EALIGN, name
        for d in range(dim):
            assert f(1, (8, 8, 8), 10, BS, DS, DF, IN, tuple(OS[x] + 8 if x == d else OS[x] for x in range(3))) == EALIGN, \
                (name, d)


def test_physderiv_python_checks_sizes_without_gpu(pkg):
    import torch
    f64 = torch.float64
    b, d = torch.zeros(56, dtype=f64), torch.zeros(64, dtype=f64)
    x3, df3 = torch.zeros(2 * 343, dtype=f64), torch.zeros(2 * 9 * 512, dtype=f64)
    x2, df2 = torch.zeros(2 * 49, dtype=f64), torch.zeros(2 * 4 * 64, dtype=f64)
    hx, qd = pkg.physderiv_hex, pkg.physderiv_quad
    with pytest.raises(ValueError):      # inp not a whole number of elements
        hx((8, 8, 8), b, b, b, d, d, d, df3, torch.zeros(2 * 343 - 1, dtype=f64))
    with pytest.raises(ValueError):      # df
        hx((8, 8, 8), b, b, b, d, d, d, df3[:-1], x3)
    with pytest.raises(ValueError):      # df with the six planes of a symmetric tensor
        hx((8, 8, 8), b, b, b, d, d, d, df3[:2 * 6 * 512], x3)
    with pytest.raises(ValueError):      # out as one tensor of the wrong size
        hx((8, 8, 8), b, b, b, d, d, d, df3, x3, out=torch.zeros(3 * 2 * 512 + 1, dtype=f64))
    with pytest.raises(ValueError):      # out as two tensors
        hx((8, 8, 8), b, b, b, d, d, d, df3, x3, out=[torch.zeros(2 * 512, dtype=f64)] * 2)
    with pytest.raises(ValueError):      # one of three too short
        hx((8, 8, 8), b, b, b, d, d, d, df3, x3, out=[torch.zeros(2 * 512, dtype=f64), torch.zeros(2 * 512, dtype=f64),
                                                       torch.zeros(2 * 512 - 1, dtype=f64)])
    with pytest.raises(ValueError):      # dtype of an output
        hx((8, 8, 8), b, b, b, d, d, d, None, x3, out=torch.zeros((3, 2 * 512), dtype=torch.float32))
    with pytest.raises(TypeError):       # an output that is no tensor
        hx((8, 8, 8), b, b, b, d, d, d, None, x3, out=[torch.zeros(2 * 512, dtype=f64), None, None])
    with pytest.raises(TypeError):       # a strided view
        hx((8, 8, 8), b, b, b, d, d, d, None, x3, out=torch.zeros((2 * 512, 3), dtype=f64).t())
    with pytest.raises(ValueError):      # a basis
        hx((8, 8, 8), b, b[:55], b, d, d, d, df3, x3)
    with pytest.raises(ValueError):      # a derivative matrix
        hx((8, 8, 8), b, b, b, d, d[:56], d, df3, x3)
    with pytest.raises(ValueError):      # dtype of df
        hx((8, 8, 8), b, b, b, d, d, d, df3.float(), x3)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, df2, torch.zeros(2 * 49 + 3, dtype=f64))
    with pytest.raises(ValueError):      # df with three planes
        qd((8, 8), b, b, d, d, df2[:2 * 3 * 64], x2)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, df2, x2, out=torch.zeros(2 * 2 * 64 - 1, dtype=f64))
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, df2, x2, out=[torch.zeros(2 * 64, dtype=f64)] * 3)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d[:63], d, df2, x2)
    with pytest.raises(ValueError):      # dtype of a derivative matrix
        qd((8, 8), b, b, d, d.float(), df2, x2)
    with pytest.raises(ValueError):      # float32 has the AUTO route only, with and without df
        qd((8, 8), b.float(), b.float(), d.float(), d.float(), df2.float(), x2.float(), variant="wave")
    with pytest.raises(ValueError):
        hx((8, 8, 8), b.float(), b.float(), b.float(), d.float(), d.float(), d.float(), None, x3.float(), variant="generic")
    # df=None and sound sizes pass every Python check: the refusal is then the library's (host tensors are no device memory)
    with pytest.raises(TypeError, match="CUDA/HIP"):
        hx((8, 8, 8), b, b, b, d, d, d, None, x3)
    with pytest.raises(TypeError, match="CUDA/HIP"):
        qd((8, 8), b, b, d, d, df2, x2, out=(torch.zeros(2 * 64, dtype=f64), torch.zeros(2 * 64, dtype=f64)))


CASES3 = [(2, 2, 2), (3, 3, 3), (5, 5, 5), (8, 8, 8), (12, 12, 12), (6, 6, 12), (3, 5, 4)]
CASES2 = [(2, 2), (8, 8), (16, 16), (32, 32), (4, 9), (23, 5)]
CASES = [(nq, 2 if max(nq) >= 12 else 3) for nq in CASES3 + CASES2]


def _data(nq, nelmt, seed=0):
    rng = np.random.default_rng(2000 + seed + 17 * sum(nq))
    nm = [q - 1 for q in nq]
    dim, nmt, nqt = len(nq), int(np.prod(nm)), int(np.prod(nq))
    bases = [rng.uniform(-1, 1, nm[d] * nq[d]) for d in range(dim)]
    derivs = [rng.uniform(-1, 1, nq[d] * nq[d]) for d in range(dim)]
    df = rng.uniform(-1, 1, nelmt * dim * dim * nqt)
    x = rng.uniform(-1, 1, nelmt * nmt)
    return bases, derivs, df, x


_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_reference_is_the_dense_operator(nq, nelmt):
    """The sweep-by-sweep reference against dense point x mode matrices assembled with einsum (long double both):
    agreement to long-double rounding, <= 1e-2 of gamma_N(2^-53) absref, with and without df."""
    if int(np.prod(nq)) > 2048:
        nelmt = 1
    bases, derivs, df, x = _data(nq, nelmt)
    dim, nmt = len(nq), int(np.prod([q - 1 for q in nq]))
    for dd in (df, None):
        ref, absref = ref_physderiv(nq, nelmt, bases, derivs, dd, x)
        assert ref.shape == absref.shape == (dim, nelmt * int(np.prod(nq)))
        dense = np.empty_like(ref).reshape(dim, nelmt, -1)
        for e in range(nelmt):
            dense[:, e] = dense_physderiv(nq, bases, derivs, None if dd is None else df.reshape(nelmt, -1)[e],
                                          x[e * nmt:(e + 1) * nmt])
        q = physderiv_excess(dense.reshape(dim, -1), ref, absref, nq, U64)
        print(f"{nq} df={'yes' if dd is not None else 'None'}: max |dense - ref| / (gamma_N absref) = {q:.3g}")
        assert q <= 1e-2
        assert float(np.max(np.abs(ref))) > 0 and float(np.min(absref)) > 0


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_fp64_and_fp32_evaluations_sit_inside_the_bound(nq, nelmt):
    """numpy evaluations of the same sweeps in fp64 and fp32 against the long-double reference: inside the bound with
    room (0.001 .. 0.36 of it on this data), with and without df: the reference alone stays well inside it."""
    bases, derivs, df, x = _data(nq, nelmt)
    f = np.float32
    b32, d32, df32, x32 = [b.astype(f) for b in bases], [d.astype(f) for d in derivs], df.astype(f), x.astype(f)
    for dd, dd32 in ((df, df32), (None, None)):
        ref, absref = ref_physderiv(nq, nelmt, bases, derivs, dd, x)
        o64, _ = physderiv_f64(nq, nelmt, bases, derivs, dd, x)
        q64 = physderiv_excess(o64, ref, absref, nq, U64)
        o32 = _physderiv(nq, nelmt, b32, d32, dd32, x32, f)
        r32, a32 = ref_physderiv(nq, nelmt, b32, d32, dd32, x32)
        q32 = physderiv_excess(o32, r32, a32, nq, U32)
        print(f"{nq} df={'yes' if dd is not None else 'None'}: fp64 {q64:.3g}, fp32 {q32:.3g} of gamma_N absref")
        assert q64 <= 1.0 and q32 <= 1.0


@pytest.mark.parametrize("nq,nelmt", [((8, 8, 8), 3), ((3, 5, 4), 5), ((5, 5, 5), 4), ((8, 8), 7), ((4, 9), 9),
                                      ((16, 16), 3)], ids=_id)
def test_gradient_energy_is_the_laplacian_energy_of_helm_ref(nq, nelmt):
    """With G_ab = W sum_c df_ca df_cb, the Laplacian energy x^T A x of tests/helm_ref.py's reference equals
    sum W |grad|^2 of this reference: the component order c = a d + b and the direction of the derivative matrices agree
    with sf_helmholtz_*.  Both in long double; <= 1e-2 of symmetry_bound(2^-53) sum_e <|A||x|, |x|>_e."""
    bases, derivs, df, x = _data(nq, nelmt)
    dim, nqt = len(nq), int(np.prod(nq))
    ld = np.longdouble
    W = np.random.default_rng(9).uniform(0.5, 1.5, nelmt * nqt)
    dd = df.astype(ld).reshape(nelmt, dim * dim, nqt)
    g = np.empty((nelmt, len(COMPONENTS[dim]), nqt), dtype=ld)
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        g[:, c] = W.reshape(nelmt, nqt) * sum(dd[:, k * dim + a] * dd[:, k * dim + b] for k in range(dim))
    # helm_ref keeps the planes in long double when it is given them so: nothing is rounded on the way
    ax, aabs = ref_helmholtz(nq, nelmt, bases, derivs, g.reshape(-1), None, 0.0, x)
    lhs = np.sum(np.asarray(ax, dtype=ld) * x.astype(ld))
    grad, _ = ref_physderiv(nq, nelmt, bases, derivs, df, x)
    rhs = np.sum(W.astype(ld) * np.sum(grad.reshape(dim, nelmt * nqt) ** 2, axis=0))
    bound = symmetry_bound(nq, U64) * math.fsum(per_element_dots(np.asarray(aabs, dtype=np.float64), np.abs(x), nelmt))
    print(f"{nq}: |x^T A x - sum W |grad|^2| = {float(abs(lhs - rhs)):.3e}, symmetry bound {bound:.3e}")
    assert abs(lhs - rhs) <= 1e-2 * bound and rhs > 0


@pytest.mark.parametrize("dim,nq", [(3, 3), (3, 5), (3, 8), (2, 4), (2, 12), (2, 16)],
                         ids=["3d-nq3", "3d-nq5", "3d-nq8", "2d-nq4", "2d-nq12", "2d-nq16"])
def test_reference_is_the_analytic_gradient(dim, nq):
    """Legendre modal basis at the Gauss-Lobatto points, the GLL differentiation matrix, affine elements x = A_e xi + c:
    the reference equals the analytic gradient of the polynomial within 0.5 gamma_N absref (measured when the test was
    written: 0.04-0.13)."""
    nelmt, ext = 5, (nq,) * dim
    bases, derivs, df, x, exact = analytic_case(nq, dim, nelmt)
    ref, absref = ref_physderiv(ext, nelmt, bases, derivs, df, x)
    q = physderiv_excess(ref, exact, absref, ext, U64)
    print(f"{ext}: max |ref - analytic| / (gamma_N absref) = {q:.3g}")
    assert q <= 0.5
    assert float(np.max(np.abs(exact))) > 0.1
    # a transposed df is a different gradient: the check can tell
    dft = df.reshape(nelmt, dim, dim, -1).transpose(0, 2, 1, 3).reshape(-1)
    bad, _ = ref_physderiv(ext, nelmt, bases, derivs, dft, x)
    assert physderiv_excess(bad, exact, absref, ext, U64) > 1e6


def test_bound_constants():
    assert physderiv_n((8, 8, 8)) == 24 + 8 + 3 == 35
    assert physderiv_n((4, 9)) == 13 + 9 + 2 == 24
    assert physderiv_n((6, 6, 12)) == 24 + 12 + 3
    assert gamma(35, U64) == 35 * U64 / (1 - 35 * U64)


NAME = re.compile(r"(hex|quad)_physderiv_wave_kernel<(\d+), .*(double|float)>")


def test_wave_instantiations_use_no_scratch():
    """Every fused wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D
    nq 2..16 for double and float, each with and without df (88).  Prints VGPRs / occupancy per kernel (the table of
    DESIGN.md s4.13)."""
    got = set()
    for src, r in kernel_resources(("physderiv.hip", "physderiv_f32.hip"), "physderiv_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, t, flag = 3 if m.group(1) == "hex" else 2, int(m.group(2)), m.group(3), ", true, " in r.name
        assert (t == "float") == (src == "physderiv_f32.hip"), (src, r.name)
        got.add((dim, nq, t, flag))
        print(f"{dim}D nq {nq:2d} {t:6s} {'df' if flag else 'reference-space'}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, "
              f"occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, h) for d, n in orders for t in ("double", "float") for h in (True, False)}
    assert len(want) == 88 and got == want, sorted(want ^ got)


def test_header_documents_physderiv():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "#define SF_VERSION 100" in text
    for needle in ("df[e][c][k][j][i]", "c = a*d + b", "d xi_b / d x_a", "NOT symmetric", "9 in 3D and", "4 in 2D",  # layout
                   "out_a[e][k][j][i] = sum_b df[e][a*d + b][k][j][i] * du_b[e][k][j][i]",
                   "out_a = sum_b df_ab du_b, b ascending", "p -> i, q -> j, r -> k",                                # order
                   "If df is NULL it is never read", "out_a = du_a", "df may be null",                                # NULL df
                   "any out_a overlapping `in`, `df` or another out_b", "NOT in-place safe",                          # overlap
                   "capture-safe", "every out_a are 16-byte aligned", "3D nq 9..11"):
        assert needle in text, needle
