"""CPU-side checks of IProductWRTDerivBase (include/sumfact.h sf_iprodderiv_*): the exports and their Python binding,
argument validation before any HIP call (NULL df / w accepted, the overlap refusals of `out` against every input), the
Python size / dtype / part-count checks, the test reference (tests/iprodderiv_ref.py) against a dense einsum
restatement, its adjointness to tests/physderiv_ref.py's reference, an analytic weak divergence, and the register /
scratch budget of every wave instantiation (hipcc cross-compiles, no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from helm_ref import gll
from iprodderiv_ref import (U32, U64, _iprodderiv, dense_iprodderiv, gamma, iprodderiv_excess, iprodderiv_f64,
                            iprodderiv_n, ref_iprodderiv)
from mass_ref import _forward_sweeps
from physderiv_ref import analytic_case, physderiv_n, ref_physderiv
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

NEW = ["sf_iprodderiv_hex_f64", "sf_iprodderiv_hex_f64_variant", "sf_iprodderiv_quad_f64",
       "sf_iprodderiv_quad_f64_variant", "sf_iprodderiv_hex_f32", "sf_iprodderiv_quad_f32"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def test_iprodderiv_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the header and the binding agree on every sf_iprodderiv_* name, and on the number of arguments of each
    declared = set(re.findall(r"\b(sf_iprodderiv_\w+)\s*\(", header))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_iprodderiv_")}
    want = {"sf_iprodderiv_hex_f64": 17, "sf_iprodderiv_hex_f64_variant": 18, "sf_iprodderiv_hex_f32": 17,
            "sf_iprodderiv_quad_f64": 13, "sf_iprodderiv_quad_f64_variant": 14, "sf_iprodderiv_quad_f32": 13}
    for name in NEW:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]) == want[name], name
    for name in ("iprodderiv_hex", "iprodderiv_quad", "physderiv_autograd"):
        assert callable(getattr(pkg, name)), name
    assert "#define SF_VERSION 100" in header


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, extents, nelmt, (b0, b1, b2), (d0, d1, d2), df, w, (i0, i1, i2), out))."""
    def hex64(v, e, n, b, d, df, w, i, o):
        return lib.sf_iprodderiv_hex_f64_variant(v, *e, n, *b, *d, df, w, *i, o, None)

    def quad64(v, e, n, b, d, df, w, i, o):
        return lib.sf_iprodderiv_quad_f64_variant(v, *e[:2], n, *b[:2], *d[:2], df, w, *i[:2], o, None)

    def hex32(v, e, n, b, d, df, w, i, o):
        assert v == 0
        return lib.sf_iprodderiv_hex_f32(*e, n, *b, *d, df, w, *i, o, None)

    def quad32(v, e, n, b, d, df, w, i, o):
        assert v == 0
        return lib.sf_iprodderiv_quad_f32(*e[:2], n, *b[:2], *d[:2], df, w, *i[:2], o, None)

    return [("hex64", 3, 8, hex64), ("quad64", 2, 8, quad64), ("hex32", 3, 4, hex32), ("quad32", 2, 4, quad32)]


def test_iprodderiv_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call, so it is testable on a machine without a GPU.  One block per step of
    the validation order of include/sumfact.h."""
    lib = pkg.capi.lib()
    # fake device addresses, far enough apart for 10 elements of 8^3 (df: 368 640 bytes, an input 40 960): never touched
    B0, B1, B2, D0, D1, D2 = 0x10000, 0x11000, 0x12000, 0x13000, 0x14000, 0x15000
    DF, W, I0, I1, I2, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    BS, DS, IS = (B0, B1, B2), (D0, D1, D2), (I0, I1, I2)
    N = (None, None, None)
    for name, dim, size, f in _calls(lib):
        ok = (8, 8, 8)
        big = 13 if dim == 3 else 33
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(0, bad, 10, BS, DS, DF, W, IS, OUT) == EINVAL, (name, bad)
            assert f(0, bad, 0, N, N, None, None, N, None) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(0, ok, 0, N, N, None, None, N, None) == 0, name
        # (3) each null pointer; df and w may be null
        for d in range(dim):
            bs = tuple(None if x == d else BS[x] for x in range(3))
            ds = tuple(None if x == d else DS[x] for x in range(3))
            is_ = tuple(None if x == d else IS[x] for x in range(3))
            assert f(0, ok, 10, bs, DS, DF, W, IS, OUT) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, ds, DF, W, IS, OUT) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, W, is_, OUT) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, None, None, is_, OUT) == EINVAL, (name, d)
        assert f(0, ok, 10, BS, DS, DF, W, IS, None) == EINVAL, name
        # ... df == NULL and w == NULL pass (3) and (4): with an odd `out` the call reaches step (4), with sound arguments
        # step (6)
        for df, w in ((None, W), (DF, None), (None, None)):
            assert f(0, ok, 10, BS, DS, df, w, IS, OUT + 1) == EALIGN, name
            assert f(0, (big, 8, 8), 10, BS, DS, df, w, IS, OUT) == ENOTBUILT, name
        # (3) before (4)
        assert f(0, ok, 10, BS, DS, DF + 1, W, IS, None) == EINVAL, name
        assert f(0, ok, 10, BS, DS, DF, W + 1, (None, I1, I2), OUT) == EINVAL, name
        # (4) each odd address; df and w only if they are not null
        for d in range(dim):
            bs = tuple(BS[x] + 1 if x == d else BS[x] for x in range(3))
            ds = tuple(DS[x] + 1 if x == d else DS[x] for x in range(3))
            is_ = tuple(IS[x] + 1 if x == d else IS[x] for x in range(3))
            assert f(0, ok, 10, bs, DS, DF, W, IS, OUT) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, ds, DF, W, IS, OUT) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, DS, DF, W, is_, OUT) == EALIGN, (name, d)
        assert f(0, ok, 10, BS, DS, DF + 1, W, IS, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, DF, W + 1, IS, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, DF, W, IS, OUT + 1) == EALIGN, name
        # (5) overlap of out with every in_a, with df (its first and its last plane) and with w, as full byte ranges
        modes = size * 10 * 7 ** dim
        points = size * 10 * 8 ** dim
        for d in range(dim):
            assert f(0, ok, 10, BS, DS, DF, W, IS, IS[d]) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, W, IS, IS[d] + points - 16) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, DF, W, IS, IS[d] - modes + 16) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, None, None, IS, IS[d]) == EINVAL, (name, d)
        assert f(0, ok, 10, BS, DS, DF, W, IS, DF) == EINVAL, name
        assert f(0, ok, 10, BS, DS, DF, W, IS, DF + dim * dim * points - 16) == EINVAL, name          # the last plane
        assert f(0, ok, 10, BS, DS, DF, W, IS, DF - modes + 16) == EINVAL, name
        assert f(0, ok, 10, BS, DS, DF, W, IS, W) == EINVAL, name
        assert f(0, ok, 10, BS, DS, DF, W, IS, W + points - 16) == EINVAL, name
        assert f(0, ok, 10, BS, DS, DF, W, IS, W - modes + 16) == EINVAL, name
        # ... with df == NULL / w == NULL their ranges are no argument at all
        assert f(0, (big, 8, 8), 10, BS, DS, None, W, IS, DF) == ENOTBUILT, name
        assert f(0, (big, 8, 8), 10, BS, DS, DF, None, IS, W) == ENOTBUILT, name
        # ... the ranges just touch: accepted by (5), refused by (6) only
        pts_big = size * 10 * big * 8 ** (dim - 1)
        assert f(0, (big, 8, 8), 10, BS, DS, DF, W, IS, DF + dim * dim * pts_big) == ENOTBUILT, name
        assert f(0, (big, 8, 8), 10, BS, DS, DF, W, IS, I0 + pts_big) == ENOTBUILT, name
        # ... and overlap is refused before the extent bounds and the variant are looked at
        assert f(0, (big, 8, 8), 10, BS, DS, DF, W, IS, I1) == EINVAL, name
        # (6) extents above the fallback's bounds
        for ext in ((big, 8, 8), (8, big, 8)) + (((8, 8, big),) if dim == 3 else ()):
            assert f(0, ext, 10, BS, DS, DF, W, IS, OUT) == ENOTBUILT, (name, ext)
    for name, dim, size, f in _calls(lib)[:2]:
        # (1) variant out of range
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, BS, DS, DF, W, IS, OUT) == EINVAL, (name, v)
        assert f(-1, (8, 8, 8), 0, N, N, None, None, N, None) == EINVAL, name
        # (5) before (7)
        assert f(2, (8, 8, 8), 10, BS, DS, DF, W, IS, I0) == EINVAL, name
        # (7) the variants that have no fused kernel: thread, block-lds, block-glb, mfma, mfma4, wave-rt
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, (8, 8, 8), 10, BS, DS, DF, W, IS, OUT) == ENOTBUILT, (name, v)
            assert f(v, (8, 8, 8), 10, BS, DS, None, None, IS, OUT) == ENOTBUILT, (name, v)
        # the inputs may overlap each other (all are only read): the call reaches step (7)
        assert f(2, (8, 8, 8), 10, (B0, B0, B0), (B0, B0, B0), DF, DF, (DF, DF, DF), OUT) == ENOTBUILT, name
        # WAVE off its table (anisotropic, or above nq 8 / 16) and WAVE on an 8-byte-aligned out
        assert f(1, (6, 6, 12) if dim == 3 else (4, 9, 0), 10, BS, DS, DF, W, IS, OUT) == ENOTBUILT, name
        assert f(1, (9, 9, 9) if dim == 3 else (17, 17, 17), 10, BS, DS, DF, W, IS, OUT) == ENOTBUILT, name
        assert f(1, (8, 8, 8), 10, BS, DS, DF, W, IS, OUT + 8) == EALIGN, name
        assert f(1, (8, 8, 8), 10, BS, DS, None, None, IS, OUT + 8) == EALIGN, name


def test_iprodderiv_python_checks_sizes_without_gpu(pkg):
    import torch
    f64 = torch.float64
    b, d = torch.zeros(56, dtype=f64), torch.zeros(64, dtype=f64)
    f3, df3, w3 = torch.zeros((3, 2 * 512), dtype=f64), torch.zeros(2 * 9 * 512, dtype=f64), torch.zeros(2 * 512, dtype=f64)
    f2, df2, w2 = torch.zeros((2, 2 * 64), dtype=f64), torch.zeros(2 * 4 * 64, dtype=f64), torch.zeros(2 * 64, dtype=f64)
    hx, qd = pkg.iprodderiv_hex, pkg.iprodderiv_quad
    with pytest.raises(ValueError):      # the parts are no whole number of elements
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, torch.zeros((3, 2 * 512 - 1), dtype=f64))
    with pytest.raises(ValueError):      # two parts for a hex
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, [f3[0], f3[1]])
    with pytest.raises(ValueError):      # a flat tensor that does not split into three
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, torch.zeros(3 * 2 * 512 + 1, dtype=f64))
    with pytest.raises(ValueError):      # one of three shorter
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, [f3[0], f3[1], f3[2][:-512]])
    with pytest.raises(ValueError):      # dtype of one part
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, [f3[0], f3[1].float(), f3[2]])
    with pytest.raises(TypeError):       # a part that is no tensor
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, [f3[0], None, f3[2]])
    with pytest.raises(TypeError):       # a strided view
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, torch.zeros((2 * 512, 3), dtype=f64).t())
    with pytest.raises(ValueError):      # df
        hx((8, 8, 8), b, b, b, d, d, d, df3[:-1], w3, f3)
    with pytest.raises(ValueError):      # df with the six planes of a symmetric tensor
        hx((8, 8, 8), b, b, b, d, d, d, df3[:2 * 6 * 512], w3, f3)
    with pytest.raises(ValueError):      # w
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3[:-1], f3)
    with pytest.raises(ValueError):      # dtype of w
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3.float(), f3)
    with pytest.raises(ValueError):      # out of the wrong size (points, not modes)
        hx((8, 8, 8), b, b, b, d, d, d, df3, w3, f3, out=torch.zeros(2 * 512, dtype=f64))
    with pytest.raises(ValueError):      # dtype of out
        hx((8, 8, 8), b, b, b, d, d, d, None, None, f3, out=torch.zeros(2 * 343, dtype=torch.float32))
    with pytest.raises(ValueError):      # a basis
        hx((8, 8, 8), b, b[:55], b, d, d, d, df3, w3, f3)
    with pytest.raises(ValueError):      # a derivative matrix
        hx((8, 8, 8), b, b, b, d, d[:56], d, df3, w3, f3)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, df2, w2, torch.zeros((2, 2 * 64 + 3), dtype=f64))
    with pytest.raises(ValueError):      # three parts for a quad
        qd((8, 8), b, b, d, d, df2, w2, [f2[0], f2[1], f2[0]])
    with pytest.raises(ValueError):      # df with three planes
        qd((8, 8), b, b, d, d, df2[:2 * 3 * 64], w2, f2)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, df2, w2, f2, out=torch.zeros(2 * 49 - 1, dtype=f64))
    with pytest.raises(ValueError):      # float32 has the AUTO route only
        qd((8, 8), b.float(), b.float(), d.float(), d.float(), df2.float(), w2.float(), f2.float(), variant="wave")
    with pytest.raises(ValueError):
        hx((8, 8, 8), b.float(), b.float(), b.float(), d.float(), d.float(), d.float(), None, None, f3.float(),
           variant="generic")
    # df=None, w=None and sound sizes pass every Python check, in each input form: the refusal is then the library's
    # binding's (host tensors are no device memory)
    padded = torch.zeros((3, 2 * 512 + 32), dtype=f64)[:, :2 * 512]                # rows contiguous, the whole is not
    assert not padded.is_contiguous()
    for inp in (f3, padded, [f3[0], f3[1], f3[2]], f3.reshape(-1)):
        with pytest.raises(TypeError, match="CUDA/HIP"):
            hx((8, 8, 8), b, b, b, d, d, d, None, None, inp)
    with pytest.raises(TypeError, match="CUDA/HIP"):
        qd((8, 8), b, b, d, d, df2, w2, (f2[0], f2[1]))
    # physderiv_autograd: constants that require grad are refused before anything runs
    x3 = torch.zeros(2 * 343, dtype=f64, requires_grad=True)
    for bases, derivs, df in (((b.clone().requires_grad_(), b, b), (d, d, d), df3),
                              ((b, b, b), (d, d.clone().requires_grad_(), d), df3),
                              ((b, b, b), (d, d, d), df3.clone().requires_grad_())):
        with pytest.raises(ValueError, match="constants"):
            pkg.physderiv_autograd((8, 8, 8), bases, derivs, df, x3)
    with pytest.raises(ValueError):
        pkg.physderiv_autograd((8, 8, 8), (b, b), (d, d, d), df3, x3)


CASES3 = [(2, 2, 2), (3, 3, 3), (5, 5, 5), (8, 8, 8), (12, 12, 12), (6, 6, 12), (3, 5, 4)]
CASES2 = [(2, 2), (8, 8), (16, 16), (32, 32), (4, 9), (23, 5)]
CASES = [(nq, 2 if max(nq) >= 12 else 3) for nq in CASES3 + CASES2]
NULLS = [(True, True), (False, True), (True, False), (False, False)]


def _data(nq, nelmt, seed=0):
    rng = np.random.default_rng(3000 + seed + 17 * sum(nq))
    nm = [q - 1 for q in nq]
    dim, nqt = len(nq), int(np.prod(nq))
    bases = [rng.uniform(-1, 1, nm[d] * nq[d]) for d in range(dim)]
    derivs = [rng.uniform(-1, 1, nq[d] * nq[d]) for d in range(dim)]
    df = rng.uniform(-1, 1, nelmt * dim * dim * nqt)
    w = rng.uniform(-1, 1, nelmt * nqt)
    f = rng.uniform(-1, 1, (dim, nelmt * nqt))
    return bases, derivs, df, w, f


_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_reference_is_the_dense_operator(nq, nelmt):
    """The sweep-by-sweep reference against dense point x mode matrices assembled with einsum (long double both):
    agreement to long-double rounding, <= 1e-2 of gamma_N(2^-53) absref, with and without df and w."""
    if int(np.prod(nq)) > 2048:
        nelmt = 1
    bases, derivs, df, w, f = _data(nq, nelmt)
    dim, nmt, nqt = len(nq), int(np.prod([q - 1 for q in nq])), int(np.prod(nq))
    for has_df, has_w in NULLS:
        dd, ww = df if has_df else None, w if has_w else None
        ref, absref = ref_iprodderiv(nq, nelmt, bases, derivs, dd, ww, f)
        assert ref.shape == absref.shape == (nelmt * nmt,)
        dense = np.empty_like(ref).reshape(nelmt, nmt)
        for e in range(nelmt):
            dense[e] = dense_iprodderiv(nq, bases, derivs, None if dd is None else df.reshape(nelmt, -1)[e],
                                        None if ww is None else w.reshape(nelmt, -1)[e],
                                        f.reshape(dim, nelmt, nqt)[:, e])
        q = iprodderiv_excess(dense.reshape(-1), ref, absref, nq, U64)
        print(f"{nq} df={has_df} w={has_w}: max |dense - ref| / (gamma_N absref) = {q:.3g}")
        assert q <= 1e-2
        assert float(np.max(np.abs(ref))) > 0 and float(np.min(absref)) > 0


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_fp64_and_fp32_evaluations_sit_inside_the_bound(nq, nelmt):
    """numpy evaluations of the same sweeps in fp64 and fp32 against the long-double reference: inside the bound, with
    and without df and w: the reference alone stays well inside it."""
    bases, derivs, df, w, f = _data(nq, nelmt)
    t = np.float32
    b32, d32 = [b.astype(t) for b in bases], [d.astype(t) for d in derivs]
    df32, w32, f32 = df.astype(t), w.astype(t), f.astype(t)
    for has_df, has_w in NULLS:
        dd, ww = df if has_df else None, w if has_w else None
        dd32, ww32 = df32 if has_df else None, w32 if has_w else None
        ref, absref = ref_iprodderiv(nq, nelmt, bases, derivs, dd, ww, f)
        o64, _ = iprodderiv_f64(nq, nelmt, bases, derivs, dd, ww, f)
        q64 = iprodderiv_excess(o64, ref, absref, nq, U64)
        o32 = _iprodderiv(nq, nelmt, b32, d32, dd32, ww32, f32, t)
        r32, a32 = ref_iprodderiv(nq, nelmt, b32, d32, dd32, ww32, f32)
        q32 = iprodderiv_excess(o32, r32, a32, nq, U32)
        print(f"{nq} df={has_df} w={has_w}: fp64 {q64:.3g}, fp32 {q32:.3g} of gamma_N absref")
        assert q64 <= 1.0 and q32 <= 1.0


@pytest.mark.parametrize("nq,nelmt", [((8, 8, 8), 3), ((3, 5, 4), 5), ((8, 8), 7), ((4, 9), 9)], ids=_id)
def test_reference_is_the_adjoint_of_the_physderiv_reference(nq, nelmt):
    """<physderiv_ref(x), f> = <x, iprodderiv_ref(df, None, f)> in long double, with and without df: the two references
    are transposes of each other.  <= 1e-2 of (gamma_Nphys + gamma_N)(2^-53) <|physderiv|(|x|), |f|>."""
    bases, derivs, df, _, f = _data(nq, nelmt)
    ld = np.longdouble
    nmt = int(np.prod([q - 1 for q in nq]))
    x = np.random.default_rng(5).uniform(-1, 1, nelmt * nmt)
    for dd in (df, None):
        grad, gabs = ref_physderiv(nq, nelmt, bases, derivs, dd, x)
        div, _ = ref_iprodderiv(nq, nelmt, bases, derivs, dd, None, f)
        lhs = np.sum(grad * f.astype(ld))
        rhs = np.sum(x.astype(ld) * div)
        bound = (gamma(physderiv_n(nq), U64) + gamma(iprodderiv_n(nq), U64)) * np.sum(gabs * np.abs(f).astype(ld))
        print(f"{nq} df={'yes' if dd is not None else 'None'}: |<Gx, f> - <x, G^T f>| = {float(abs(lhs - rhs)):.3e}, "
              f"bound {float(bound):.3e}")
        assert abs(lhs - rhs) <= 1e-2 * bound and abs(lhs) > 0


def _weak_divergence_case(nq, dim, nelmt):
    """The geometry of physderiv_ref.analytic_case (Legendre modal basis at the Gauss-Lobatto points, affine elements
    x = A_e xi + c) with w = |det A_e| x the tensor GLL weight and a polynomial field F_a = sum c_a[r][q][p] P_p P_q P_r.
    Returns (bases, derivs, df, w, f, exact): exact[e][m] = int d phi_m / d x_a F_a dx summed over a, from the closed
    forms of the integrals of Legendre polynomials, in np.longdouble."""
    ld = np.longdouble
    nm = nq - 1
    bases, derivs, df, _, _ = analytic_case(nq, dim, nelmt)
    _, wts, _ = gll(nq)
    npt = nq ** dim
    dfe = df.reshape(nelmt, dim, dim, npt)[:, :, :, 0]                 # [e][a][b] = d xi_b / d x_a, constant per element
    jac = 1.0 / np.abs(np.linalg.det(dfe))                              # |det A_e| as the operator gets it
    W = wts
    for _ in range(dim - 1):
        W = np.multiply.outer(wts, W)
    w = (jac[:, None] * W.reshape(-1)[None, :]).reshape(-1)
    rng = np.random.default_rng(77 + nq + dim)
    c = rng.uniform(-1, 1, (dim, nelmt * nm ** dim))
    f = np.stack([_forward_sweeps((nq,) * dim, nelmt, [np.asarray(b, dtype=ld) for b in bases], c[a], ld)
                  for a in range(dim)])
    # int P_p P_p' = 2 / (2p + 1) for p == p';  int (d P_p / d xi) P_p' = 2 for p > p' with p - p' odd (d P_p / d xi =
    # sum (2k + 1) P_k over k = p - 1, p - 3, ..); both 0 otherwise
    Mm = np.diag([ld(2) / ld(2 * p + 1) for p in range(nm)])
    Sm = np.array([[2.0 if p > q and (p - q) % 2 else 0.0 for q in range(nm)] for p in range(nm)], dtype=ld)
    wl = w.astype(ld).reshape(nelmt, npt)
    scale = wl[:, 0] / ld(W.reshape(-1)[0])                             # the Jacobian the weights carry
    exact = np.zeros((nelmt,) + (nm,) * dim, dtype=ld)
    for a in range(dim):
        ca = c[a].astype(ld).reshape((nelmt,) + (nm,) * dim)
        for b in range(dim):
            y = ca
            for d in range(dim):
                axis = y.ndim - 1 - d
                y = np.moveaxis(np.moveaxis(y, axis, -1) @ (Sm if d == b else Mm).T, -1, axis)
            coef = (scale * dfe[:, a, b].astype(ld)).reshape((nelmt,) + (1,) * dim)
            exact += coef * y
    return bases, derivs, df, w, f, exact.reshape(-1)


@pytest.mark.parametrize("dim,nq", [(3, 3), (3, 5), (3, 8), (2, 4), (2, 12), (2, 16)],
                         ids=["3d-nq3", "3d-nq5", "3d-nq8", "2d-nq4", "2d-nq12", "2d-nq16"])
def test_reference_is_the_analytic_weak_divergence(dim, nq):
    """With w = quadrature weight x Jacobian on affine elements the reference equals the analytic weak divergence
    sum_a int d phi_m / d x_a F_a dx of a polynomial field (the GLL rule is exact for the degrees involved) within
    0.5 gamma_N absref -- the allowance tests/test_physderiv_cpu.py gives the same Gauss-Lobatto points, weights and
    differentiation matrix, which are fp64 values (measured when the test was written: 0.008-0.10)."""
    nelmt, ext = 5, (nq,) * dim
    bases, derivs, df, w, f, exact = _weak_divergence_case(nq, dim, nelmt)
    ref, absref = ref_iprodderiv(ext, nelmt, bases, derivs, df, w, f)
    q = iprodderiv_excess(ref, exact, absref, ext, U64)
    print(f"{ext}: max |ref - analytic| / (gamma_N absref) = {q:.3g}")
    assert q <= 0.5
    assert float(np.max(np.abs(exact))) > 0.1
    # a transposed df is a different operator: the check can tell
    dft = df.reshape(nelmt, dim, dim, -1).transpose(0, 2, 1, 3).reshape(-1)
    bad, _ = ref_iprodderiv(ext, nelmt, bases, derivs, dft, w, f)
    assert iprodderiv_excess(bad, exact, absref, ext, U64) > 1e6


def test_bound_constants():
    assert iprodderiv_n((8, 8, 8)) == 24 + 8 + 6 == 38
    assert iprodderiv_n((4, 9)) == 13 + 9 + 4 == 26
    assert iprodderiv_n((6, 6, 12)) == 24 + 12 + 6
    assert gamma(38, U64) == 38 * U64 / (1 - 38 * U64)
    assert math.isinf(iprodderiv_excess(np.ones(1), np.zeros(1), np.zeros(1), (8, 8), U64))       # zero bound, an error


NAME = re.compile(r"(hex|quad)_iprodderiv_wave_kernel<(\d+), .*, (true|false), (true|false), (float|double)>")


def test_wave_instantiations_use_no_scratch():
    """Every fused wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D
    nq 2..16 for double and float, each with and without df and with and without w (176).  Prints VGPRs / occupancy per
    kernel (the table of DESIGN.md s4.14)."""
    got = set()
    for src, r in kernel_resources(("iprodderiv.hip", "iprodderiv_f32.hip"), "iprodderiv_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, t = 3 if m.group(1) == "hex" else 2, int(m.group(2)), m.group(5)
        hasdf, hasw = m.group(3) == "true", m.group(4) == "true"
        assert (t == "float") == (src == "iprodderiv_f32.hip"), (src, r.name)
        got.add((dim, nq, t, hasdf, hasw))
        print(f"{dim}D nq {nq:2d} {t:6s} {'df' if hasdf else '--'} {'w' if hasw else '-'}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, "
              f"occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, h, w) for d, n in orders for t in ("double", "float") for h in (True, False) for w in (True, False)}
    assert len(want) == 176 and got == want, sorted(want ^ got)


def test_header_documents_iprodderiv():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "#define SF_VERSION 100" in text
    for needle in ("g_b[e][k][j][i] = w[e][k][j][i] * sum_a df[e][a*d + b][k][j][i] * in_a[e][k][j][i]",       # operator
                   "out[e][r][q][p] = sum_b (B^T D_b^T g_b)[e][r][q][p]",
                   "exactly what sf_physderiv_* writes", "the ROW index a", "laid out like the w of",          # layout
                   "the layout of sf_iproduct_*'s",
                   "If df is NULL it is never read (nor validated): g_b = w * in_b",                           # NULL rules
                   "If w is NULL it is never read (nor validated)", "With both NULL the call is sum_b B^T D_b^T in_b",
                   "algebraic transpose of sf_physderiv_*",
                   "1. t_b = sum_a df_ab in_a, a ascending", "2. g_b = w * t_b",                                # order
                   "3. v = (D_0^T g_0 + D_1^T g_1) [+ D_2^T g_2]", "4. transposed sweeps k -> r, j -> q, i -> p",
                   "Only `out` needs 16-byte alignment for the wave route", "need only scalar alignment on every route",
                   "`out` overlapping any in_a, `df` or `w`", "NOT in-place safe",                              # overlap
                   "the inputs may overlap each other", "capture-safe", "(d*d + d + 1) nq^d + nm^d"):
        assert needle in text, needle
