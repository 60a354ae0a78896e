"""CPU-side checks of the diagonal of the fused Helmholtz operator (include/sumfact.h sf_diag_helmholtz_*,
sf_diag_tables_*): the exports and their Python binding, every step of the argument validation before any HIP call (w
ignored at lambda = 0, inputs overlapping each other accepted, `out` overlapping a table refused), the Python size and
dtype checks, the test reference (tests/diag_ref.py) against the diagonal of the dense operator of tests/helm_ref.py and
against the Gauss-Lobatto closed form, numpy evaluations inside the bound, positivity, and the register / scratch budget
of every wave instantiation (hipcc cross-compiles, no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from diag_ref import (diag_excess, diag_f64, diag_n, diag_np, gll_exact_diag, ref_diag, tables, tables_excess)
from helm_ref import COMPONENTS, U32, U64, dense_operator, gamma, gll_setup
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

NEW = ["sf_diag_tables_f64", "sf_diag_tables_f32", "sf_diag_helmholtz_hex_f64", "sf_diag_helmholtz_hex_f64_variant",
       "sf_diag_helmholtz_quad_f64", "sf_diag_helmholtz_quad_f64_variant", "sf_diag_helmholtz_hex_f32",
       "sf_diag_helmholtz_quad_f32"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def test_diag_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the header and the binding agree on every sf_diag_* name, and on the number of arguments of each
    declared = set(re.findall(r"\bint\s+(sf_diag_\w+)\s*\(", header))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_diag_")}
    for name in NEW:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]), name
    for name in ("diag_tables", "diag_helmholtz_hex", "diag_helmholtz_quad"):
        assert callable(getattr(pkg, name)), name
    assert lib.sf_version() == 100


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, extents, nelmt, (t0, t1, t2), g, w, lam, out))."""
    def hex64(v, e, n, t, g, w, lam, o):
        return lib.sf_diag_helmholtz_hex_f64_variant(v, *e, n, *t, g, w, lam, o, None)

    def quad64(v, e, n, t, g, w, lam, o):
        return lib.sf_diag_helmholtz_quad_f64_variant(v, *e[:2], n, *t[:2], g, w, lam, o, None)

    def hex32(v, e, n, t, g, w, lam, o):
        assert v == 0
        return lib.sf_diag_helmholtz_hex_f32(*e, n, *t, g, w, lam, o, None)

    def quad32(v, e, n, t, g, w, lam, o):
        assert v == 0
        return lib.sf_diag_helmholtz_quad_f32(*e[:2], n, *t[:2], g, w, lam, o, None)

    return [("hex64", 3, 8, hex64), ("quad64", 2, 8, quad64), ("hex32", 3, 4, hex32), ("quad32", 2, 4, quad32)]


def test_diag_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call, so it is testable on a machine without a GPU.  One block per step of
    the validation order of include/sumfact.h."""
    lib = pkg.capi.lib()
    # fake device addresses, far enough apart for 10 elements of 8^3 (g: 245 760 bytes) and a table triple (1344 bytes)
    T0, T1, T2 = 0x10000, 0x11000, 0x12000
    G, W, OUT = 0x100000, 0x200000, 0x400000
    TS = (T0, T1, T2)
    N = (None, None, None)
    for name, dim, size, f in _calls(lib):
        ok = (8, 8, 8)
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(0, bad, 10, TS, G, W, 1.0, OUT) == EINVAL, (name, bad)
            assert f(0, bad, 0, N, None, None, 1.0, None) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(0, ok, 0, N, None, None, 1.0, None) == 0, name
        # (3) each null pointer; w only with lambda != 0; a lambda that is not finite
        for d in range(dim):
            ts = tuple(None if x == d else TS[x] for x in range(3))
            assert f(0, ok, 10, ts, G, W, 1.0, OUT) == EINVAL, (name, d)
        assert f(0, ok, 10, TS, None, W, 1.0, OUT) == EINVAL, name
        assert f(0, ok, 10, TS, G, None, 1.0, OUT) == EINVAL, name
        assert f(0, ok, 10, TS, G, None, -1e-300, OUT) == EINVAL, name
        assert f(0, ok, 10, TS, G, W, 1.0, None) == EINVAL, name
        for lam in (math.inf, -math.inf, math.nan):
            assert f(0, ok, 10, TS, G, W, lam, OUT) == EINVAL, (name, lam)
            assert f(0, ok, 10, TS, G, None, lam, OUT) == EINVAL, (name, lam)
        # ... a null w with lambda == 0 passes (3): with an odd g the call reaches step (4)
        assert f(0, ok, 10, TS, G + 1, None, 0.0, OUT) == EALIGN, name
        assert f(0, ok, 10, TS, G + 1, None, -0.0, OUT) == EALIGN, name
        # (3) before (4)
        assert f(0, ok, 10, TS, G + 1, None, 1.0, OUT) == EINVAL, name
        # (4) each odd address; w only with lambda != 0
        for d in range(dim):
            ts = tuple(TS[x] + 1 if x == d else TS[x] for x in range(3))
            assert f(0, ok, 10, ts, G, W, 1.0, OUT) == EALIGN, (name, d)
        assert f(0, ok, 10, TS, G + 1, W, 1.0, OUT) == EALIGN, name
        assert f(0, ok, 10, TS, G, W + 1, 1.0, OUT) == EALIGN, name
        assert f(0, ok, 10, TS, G, W, 1.0, OUT + 1) == EALIGN, name
        # (5) overlap: out == g, out inside the last plane of g, out == w, out inside w, out straddling the ends of a
        #     table triple (3 * 7 * 8 scalars)
        modes = size * 10 * 7 ** dim
        points = size * 10 * 8 ** dim
        ncomp = len(COMPONENTS[dim])
        tab = size * 3 * 7 * 8
        assert f(0, ok, 10, TS, G, W, 1.0, G) == EINVAL, name
        assert f(0, ok, 10, TS, G, W, 1.0, G + ncomp * points - 16) == EINVAL, name
        assert f(0, ok, 10, TS, G, W, 1.0, W) == EINVAL, name
        assert f(0, ok, 10, TS, G, W, 1.0, W + 16) == EINVAL, name
        for d in range(dim):
            assert f(0, ok, 10, TS, G, W, 1.0, TS[d]) == EINVAL, (name, d)
            assert f(0, ok, 10, TS, G, W, 1.0, TS[d] + tab - 16) == EINVAL, (name, d)
            assert f(0, ok, 10, TS, G, W, 1.0, TS[d] - modes + 16) == EINVAL, (name, d)
        # ... and overlap is refused before the extent bounds and the variant are looked at
        big = 13 if dim == 3 else 33
        assert f(0, (big, 8, 8), 10, TS, G, W, 1.0, G) == EINVAL, name
        # (6) extents above the fallback's bounds
        for ext in ((big, 8, 8), (8, big, 8)) + (((8, 8, big),) if dim == 3 else ()):
            assert f(0, ext, 10, TS, G, W, 1.0, OUT) == ENOTBUILT, (name, ext)
    for name, dim, size, f in _calls(lib)[:2]:
        # (1) variant out of range
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, TS, G, W, 1.0, OUT) == EINVAL, (name, v)
        assert f(-1, (8, 8, 8), 0, N, None, None, 1.0, None) == EINVAL, name
        # (5) before (7)
        assert f(2, (8, 8, 8), 10, TS, G, W, 1.0, G) == EINVAL, name
        # (7) the variants that have no kernel here: thread, block-lds, block-glb, mfma, mfma4, wave-rt
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, (8, 8, 8), 10, TS, G, W, 1.0, OUT) == ENOTBUILT, (name, v)
        # WAVE off its table (anisotropic, or above nq 8 / 16) and WAVE on an 8-byte-aligned out
        assert f(1, (6, 6, 12) if dim == 3 else (4, 9, 0), 10, TS, G, W, 1.0, OUT) == ENOTBUILT, name
        assert f(1, (9, 9, 9) if dim == 3 else (17, 17, 17), 10, TS, G, W, 1.0, OUT) == ENOTBUILT, name
        assert f(1, (8, 8, 8), 10, TS, G, W, 1.0, OUT + 8) == EALIGN, name


def test_inputs_may_overlap_each_other_and_w_is_ignored_at_lambda_zero(pkg):
    """Inputs overlapping each other pass validation (all are only read): with an unsupported variant the call reaches
    step (7), SF_ENOTBUILT, and not the overlap refusal of step (5).  With lambda == 0, `w` is no argument at all: it may
    be null, odd, or overlap `out`.  `out` overlapping a table is refused."""
    lib = pkg.capi.lib()
    T, G, OUT = 0x10000, 0x100000, 0x400000
    h, q = lib.sf_diag_helmholtz_hex_f64_variant, lib.sf_diag_helmholtz_quad_f64_variant
    assert h(2, 8, 8, 8, 10, T, T, T, G, G, 1.0, OUT, None) == ENOTBUILT        # one table thrice, w == g
    assert h(2, 8, 8, 8, 10, T, T + 64, T, G, G + 64, 1.0, OUT, None) == ENOTBUILT
    assert h(2, 8, 8, 8, 10, G, G, G, G, G, 1.0, OUT, None) == ENOTBUILT        # the tables inside g
    assert q(2, 8, 8, 10, T, T, G, G, 1.0, OUT, None) == ENOTBUILT
    assert h(2, 8, 8, 8, 10, T, T, T, G, G, 1.0, G, None) == EINVAL
    assert h(2, 8, 8, 8, 10, T, T, OUT, G, G, 1.0, OUT, None) == EINVAL         # out == tab2
    assert h(2, 8, 8, 8, 10, T, T, OUT + 27440 - 8, G, G, 1.0, OUT, None) == EINVAL   # tab2 starts in out's last scalar
    assert h(2, 8, 8, 8, 10, T, T, OUT + 27440, G, G, 1.0, OUT, None) == ENOTBUILT    # ... and right behind it
    assert q(2, 8, 8, 10, OUT, T, G, G, 1.0, OUT, None) == EINVAL               # out == tab0
    assert h(2, 8, 8, 8, 10, T, T, T, G, OUT, 1.0, OUT, None) == EINVAL         # out == w, lambda != 0
    assert h(2, 8, 8, 8, 10, T, T, T, G, OUT, 0.0, OUT, None) == ENOTBUILT      # ... lambda == 0
    assert h(2, 8, 8, 8, 10, T, T, T, G, OUT + 1, 0.0, OUT, None) == ENOTBUILT
    assert h(2, 8, 8, 8, 10, T, T, T, G, None, 0.0, OUT, None) == ENOTBUILT


def test_diag_tables_argument_validation_without_gpu(pkg):
    lib = pkg.capi.lib()
    B, D, TAB = 0x10000, 0x20000, 0x30000
    for f, size in ((lib.sf_diag_tables_f64, 8), (lib.sf_diag_tables_f32, 4)):
        for nq in (0, 1, 1025):
            assert f(nq, B, D, TAB, None) == EINVAL, nq
        assert f(8, None, D, TAB, None) == EINVAL
        assert f(8, B, None, TAB, None) == EINVAL
        assert f(8, B, D, None, None) == EINVAL
        assert f(8, B + 1, D, TAB, None) == EALIGN
        assert f(8, B, D + 1, TAB, None) == EALIGN
        assert f(8, B, D, TAB + 1, None) == EALIGN
        assert f(8, B, D, B, None) == EINVAL                              # tab == basis
        assert f(8, B, D, D, None) == EINVAL                              # tab == deriv
        assert f(8, B, D, B - 3 * 56 * size + size, None) == EINVAL       # tab ends in basis's first scalar
        assert f(8, B, D, D + 64 * size - size, None) == EINVAL           # tab starts in deriv's last scalar


def test_diag_python_checks_sizes_without_gpu(pkg):
    import torch
    f64 = torch.float64
    b, d, t = torch.zeros(56, dtype=f64), torch.zeros(64, dtype=f64), torch.zeros(3 * 56, dtype=f64)
    w3, g3 = torch.zeros(2 * 512, dtype=f64), torch.zeros(2 * 6 * 512, dtype=f64)
    w2, g2 = torch.zeros(2 * 64, dtype=f64), torch.zeros(2 * 3 * 64, dtype=f64)
    hx, qd, tb = pkg.diag_helmholtz_hex, pkg.diag_helmholtz_quad, pkg.diag_tables
    t3, t2 = (t, t, t), (t, t)
    with pytest.raises(ValueError):      # g not a whole number of elements
        hx((8, 8, 8), b, b, b, d, d, d, g3[:-1], w3, 1.0, tabs=t3)
    with pytest.raises(ValueError):      # g with five planes: 10 planes are no multiple of six
        hx((8, 8, 8), b, b, b, d, d, d, g3[:2 * 5 * 512], w3, 1.0, tabs=t3)
    with pytest.raises(ValueError):      # w
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3[:-1], 1.0, tabs=t3)
    with pytest.raises(ValueError):      # w=None needs lam == 0
        hx((8, 8, 8), b, b, b, d, d, d, g3, None, 0.5, tabs=t3)
    with pytest.raises(ValueError):      # out
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3, 1.0, out=torch.zeros(2 * 343 + 1, dtype=f64), tabs=t3)
    with pytest.raises(ValueError):      # a table
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3, 1.0, tabs=(t, t[:-1], t))
    with pytest.raises(ValueError):      # two tables for three directions
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3, 1.0, tabs=t2)
    with pytest.raises(ValueError):      # dtype of w
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3.float(), 1.0, tabs=t3)
    with pytest.raises(ValueError):      # dtype of a table
        hx((8, 8, 8), b, b, b, d, d, d, g3, w3, 1.0, tabs=(t, t, t.float()))
    with pytest.raises(TypeError):       # g is no tensor
        hx((8, 8, 8), b, b, b, d, d, d, None, w3, 1.0, tabs=t3)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, g2[:100], w2, 1.0, tabs=t2)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, g2, w2[:100], 1.0, tabs=t2)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, g2, None, 1.0, tabs=t2)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d, d, g2, w2, 1.0, out=torch.zeros(97, dtype=f64), tabs=t2)
    with pytest.raises(ValueError):      # float32 has the AUTO route only
        qd((8, 8), b, b, d, d, g2.float(), w2.float(), 1.0, variant="wave", tabs=(t.float(), t.float()))
    # tabs=None builds the tables: the basis and the derivative matrix are checked there
    with pytest.raises(ValueError):
        qd((8, 8), b[:55], b, d, d, g2, w2, 1.0)
    with pytest.raises(ValueError):
        qd((8, 8), b, b, d[:63], d, g2, w2, 1.0)
    with pytest.raises(ValueError):
        tb(8, b, d[:63])
    with pytest.raises(ValueError):
        tb(8, b[:55], d)
    with pytest.raises(ValueError):      # dtype of the derivative matrix
        tb(8, b, d.float())
    with pytest.raises(TypeError):
        tb(8, b.long(), d)


def _data(nq, nelmt, seed=0):
    rng = np.random.default_rng(2000 + seed + 17 * sum(nq))
    nqt = int(np.prod(nq))
    bases = [rng.uniform(-1, 1, (q - 1) * q) for q in nq]
    derivs = [rng.uniform(-1, 1, q * q) for q in nq]
    g = rng.uniform(-1, 1, nelmt * len(COMPONENTS[len(nq)]) * nqt)
    w = rng.uniform(-1, 1, nelmt * nqt)
    return bases, derivs, g, w


_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


@pytest.mark.parametrize("nq,nelmt", [((4, 4, 4), 3), ((3, 5, 4), 4), ((5, 5), 5), ((4, 9), 3)], ids=_id)
def test_reference_is_the_diagonal_of_the_dense_operator(nq, nelmt):
    """The sweep-by-sweep reference against np.diag of the element matrix that tests/helm_ref.py assembles with einsum
    (long double both): agreement to long-double rounding, within 1e-2 of the fp64 bound."""
    bases, derivs, g, w = _data(nq, nelmt)
    for lam, ww in ((0.75, w), (0.0, None)):
        ref, absref = ref_diag(nq, nelmt, bases, derivs, g, ww, lam)
        dense = np.concatenate([np.diag(dense_operator(nq, bases, derivs, g.reshape(nelmt, -1)[e],
                                                       None if ww is None else w.reshape(nelmt, -1)[e], lam))
                                for e in range(nelmt)])
        q = diag_excess(dense, ref, absref, nq, U64)
        print(f"{nq} lam={lam}: max |diag(dense) - ref| / (gamma_N absref) = {q:.3g}")
        assert q <= 1e-2
        assert float(np.max(np.abs(ref))) > 0 and float(np.min(absref)) > 0


@pytest.mark.parametrize("dim,nq", [(3, 6), (2, 9)], ids=["3d-nq6", "2d-nq9"])
def test_gll_closed_form(dim, nq):
    """Legendre modes at the Gauss-Lobatto points, G = I * weight, w = weight: the diagonal is lam prod m[p_d] + sum_a
    s[p_a] prod_{d != a} m[p_d], m[p] = 2 / (2p + 1), s[p] = p (p + 1).  Relative to max |exact| within 1e-12 (the
    accuracy of gll()'s points and weights), with and without the mass term."""
    nelmt, ext = 2, (nq,) * dim
    bases, derivs, g, w = gll_setup(nq, dim, nelmt)
    for lam, ww in ((0.75, w), (0.0, None)):
        exact = np.tile(gll_exact_diag(nq, dim, lam), nelmt)
        ref, _ = ref_diag(ext, nelmt, bases, derivs, g, ww, lam)
        got, _ = diag_f64(ext, nelmt, bases, derivs, g, ww, lam)
        scale = float(np.max(np.abs(exact)))
        e_ref = float(np.max(np.abs(np.asarray(ref, dtype=np.float64) - exact))) / scale
        e_got = float(np.max(np.abs(got - exact))) / scale
        print(f"{ext} lam={lam}: max |exact| = {scale:.4g}, relative: reference {e_ref:.3g}, fp64 {e_got:.3g}")
        assert e_ref <= 1e-12 and e_got <= 1e-12


SHAPES = [((2, 2, 2), 5), ((4, 4, 4), 3), ((3, 5, 4), 4), ((8, 8, 8), 2), ((12, 12, 12), 1), ((16, 16), 3), ((4, 9), 5),
          ((32, 32), 2)]


@pytest.mark.parametrize("nq,nelmt", SHAPES, ids=_id)
def test_fp64_and_fp32_evaluations_sit_inside_the_bound(nq, nelmt):
    """numpy evaluations of the tables and the sweeps in fp64 and fp32 against the long-double reference of the same
    (rounded) data: inside the bound, with room."""
    bases, derivs, g, w = _data(nq, nelmt)
    for lam, on in ((0.75, True), (0.0, False)):
        ref, absref = ref_diag(nq, nelmt, bases, derivs, g, w if on else None, lam)
        o64, _ = diag_f64(nq, nelmt, bases, derivs, g, w if on else None, lam)
        q64 = diag_excess(o64, ref, absref, nq, U64)
        f = np.float32
        b32, d32, g32, w32 = [b.astype(f) for b in bases], [d.astype(f) for d in derivs], g.astype(f), w.astype(f)
        o32, _ = diag_np(nq, nelmt, b32, d32, g32, w32 if on else None, lam, f)
        r32, a32 = ref_diag(nq, nelmt, b32, d32, g32, w32 if on else None, lam)
        q32 = diag_excess(o32, r32, a32, nq, U32)
        print(f"{nq} lam={lam}: fp64 {q64:.3g}, fp32 {q32:.3g} of gamma_N absref (N = {diag_n(nq)})")
        assert q64 <= 1.0 and q32 <= 1.0
    # the tables alone, against gamma_{2 nq + 1}
    for q, b, d in zip(nq, bases, derivs):
        t64 = tables(q, b, d, np.float64)
        assert tables_excess(t64, tables(q, b, d), tables(q, b, d, absolute=True), q, U64) <= 1.0


@pytest.mark.parametrize("nq,nelmt", [((4, 4, 4), 3), ((3, 5, 4), 4), ((8, 8), 5), ((4, 9), 3)], ids=_id)
def test_diagonal_is_positive_for_spd_metric(nq, nelmt):
    """G = L L^T per point (L lower triangular from the planes of a random g) and lambda w >= 0: every diagonal entry is
    that of a positive semidefinite matrix, >= 0 up to the bound, and positive in sum."""
    bases, derivs, g, w = _data(nq, nelmt)
    dim, nc = len(nq), len(COMPONENTS[len(nq)])
    L = g.reshape(nelmt, nc, -1)
    tri = {(b, a): L[:, c] for c, (a, b) in enumerate(COMPONENTS[dim])}
    spd = np.empty_like(L)
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        spd[:, c] = sum(tri[(a, k)] * tri[(b, k)] for k in range(a + 1))
    ref, absref = ref_diag(nq, nelmt, bases, derivs, spd.reshape(-1), np.abs(w), 0.75)
    got, _ = diag_f64(nq, nelmt, bases, derivs, spd.reshape(-1), np.abs(w), 0.75)
    slack = gamma(diag_n(nq), U64) * np.asarray(absref, dtype=np.float64)
    assert np.all(np.asarray(ref, dtype=np.float64) >= 0) and np.all(got + slack >= 0) and float(np.sum(got)) > 0


def test_bound_constants():
    assert diag_n((8, 8, 8)) == 3 * 24 + 3 + 2 + 6 == 83
    assert diag_n((4, 9)) == 3 * 13 + 2 + 2 + 3 == 46
    assert gamma(83, U64) == 83 * U64 / (1 - 83 * U64)


NAME = re.compile(r"(hex|quad)_diag_wave_kernel<(\d+), .*(double|float)>")


def test_wave_instantiations_use_no_scratch():
    """Every wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D nq 2..16
    for double and float, each with and without the mass term (the documented table, no row left out).  Prints VGPRs /
    occupancy per kernel (the table of DESIGN.md s4.15)."""
    got = set()
    for src, r in kernel_resources(("diag.hip", "diag_f32.hip"), "diag_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, t, flag = 3 if m.group(1) == "hex" else 2, int(m.group(2)), m.group(3), ", true, " in r.name
        assert (t == "float") == (src == "diag_f32.hip"), (src, r.name)
        got.add((dim, nq, t, flag))
        print(f"{dim}D nq {nq:2d} {t:6s} {'helmholtz' if flag else 'laplacian'}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, "
              f"occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, h) for d, n in orders for t in ("double", "float") for h in (True, False)}
    assert got == want, sorted(want ^ got)


def test_header_documents_diag():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "#define SF_VERSION 100" in text
    for needle in ("tab[t][p][i]", "T^0 = B o B,  T^1 = E o B,  T^2 = E o E", "E[p][i] = sum_m deriv[i*nq + m] * basis[p*nq + m]",
                   "s_d = [d == a] + [d == b]", "f_c = 1 if a == b, else 2",                                    # tables, layout
                   "k -> r, j -> q, i -> p", "B^0 = (S_3 + S_4) + S_5", "are doubled", "A_5 = A_5 + sum_k (lambda w",  # order
                   "(sum_i B^0 T0^0[p][i] + sum_i B^1 T0^1[p][i]) + sum_i B^2 T0^2[p][i]",
                   "a null w with lambda != 0", "not finite", "or any of the tables", "may be NULL",           # validation
                   "capture-safe", "3D nq 9..12, all anisotropic shapes", "`tab` overlapping `basis` or `deriv`"):
        assert needle in text, needle
