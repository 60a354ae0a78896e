"""CPU-side checks of the fused Helmholtz operator on affine elements (include/sumfact.h sf_affine_helmholtz_*): the
exports and their Python binding, argument validation before any HIP call in the documented order (a null je with
lambda = 0, je ignored at lambda = 0, the overlap refusals, input / input overlap accepted), the Python size and dtype
checks, the test reference (tests/affine_ref.py) against the dense einsum restatement of tests/helm_ref.py on expanded
data, numpy evaluations of the documented order inside the bound, the affine energy identity, the header text, and the
register / scratch budget of every wave instantiation (hipcc cross-compiles, no GPU needed)."""
import math
import os
import re

import numpy as np
import pytest

from affine_ref import (affine_eval, affine_excess, affine_geometry, affine_n, exact_energy_affine, expand,
                        gll_affine_setup, ref_affine)
from helm_ref import (COMPONENTS, U32, U64, dense_operator, gamma, helm_n, helmholtz_f64, per_element_dots,
                      symmetry_bound)
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

NEW = ["sf_affine_helmholtz_hex_f64", "sf_affine_helmholtz_hex_f64_variant", "sf_affine_helmholtz_quad_f64",
       "sf_affine_helmholtz_quad_f64_variant", "sf_affine_helmholtz_hex_f32", "sf_affine_helmholtz_quad_f32"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def test_affine_exports(pkg):
    lib = pkg.capi.lib()
    header = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the header and the binding agree on every sf_affine_* name, and on the number of arguments of each
    declared = set(re.findall(r"\b(sf_affine_\w+)\s*\(", header))
    assert declared == set(NEW) == {n for n in pkg.capi.SYMBOLS if n.startswith("sf_affine_")}
    for name in NEW:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(args.split(",")) == len(pkg.capi.SYMBOLS[name][1]), name
    # 3D: 4 extents/count + 3 bases + 3 derivs + 3 weights + ge + je + lambda + in + out + stream
    assert len(pkg.capi.SYMBOLS["sf_affine_helmholtz_hex_f64"][1]) == 19
    assert len(pkg.capi.SYMBOLS["sf_affine_helmholtz_quad_f64_variant"][1]) == 16
    assert not any(n.startswith("sf_helmholtz_") for n in NEW)
    for name in ("affine_helmholtz_hex", "affine_helmholtz_quad"):
        assert callable(getattr(pkg, name)), name
    assert lib.sf_version() == 100


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, extents, nelmt, bases, derivs, qws, ge, je, lam, in, out))."""
    def hex64(v, e, n, b, d, q, ge, je, lam, i, o):
        return lib.sf_affine_helmholtz_hex_f64_variant(v, *e, n, *b, *d, *q, ge, je, lam, i, o, None)

    def quad64(v, e, n, b, d, q, ge, je, lam, i, o):
        return lib.sf_affine_helmholtz_quad_f64_variant(v, *e[:2], n, *b[:2], *d[:2], *q[:2], ge, je, lam, i, o, None)

    def hex32(v, e, n, b, d, q, ge, je, lam, i, o):
        assert v == 0
        return lib.sf_affine_helmholtz_hex_f32(*e, n, *b, *d, *q, ge, je, lam, i, o, None)

    def quad32(v, e, n, b, d, q, ge, je, lam, i, o):
        assert v == 0
        return lib.sf_affine_helmholtz_quad_f32(*e[:2], n, *b[:2], *d[:2], *q[:2], ge, je, lam, i, o, None)

    return [("hex64", 3, 8, hex64), ("quad64", 2, 8, quad64), ("hex32", 3, 4, hex32), ("quad32", 2, 4, quad32)]


def test_affine_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call, so it is testable on a machine without a GPU.  One block per step of
    the validation order of include/sumfact.h."""
    lib = pkg.capi.lib()
    # fake device addresses, far apart: never touched on these paths
    BS, DS, QS = (0x10000, 0x11000, 0x12000), (0x13000, 0x14000, 0x15000), (0x16000, 0x17000, 0x18000)
    GE, JE, IN, OUT = 0x100000, 0x200000, 0x300000, 0x400000
    N = (None, None, None)
    for name, dim, size, f in _calls(lib):
        ok = (8, 8, 8)
        ncomp = len(COMPONENTS[dim])
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(0, bad, 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == EINVAL, (name, bad)
            assert f(0, bad, 0, N, N, N, None, None, 1.0, None, None) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(0, ok, 0, N, N, N, None, None, 1.0, None, None) == 0, name
        # (3) each null pointer; je only with lambda != 0; a lambda that is not finite
        for d in range(dim):
            drop = lambda t: tuple(None if x == d else t[x] for x in range(3))      # noqa: E731
            assert f(0, ok, 10, drop(BS), DS, QS, GE, JE, 1.0, IN, OUT) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, drop(DS), QS, GE, JE, 1.0, IN, OUT) == EINVAL, (name, d)
            assert f(0, ok, 10, BS, DS, drop(QS), GE, JE, 1.0, IN, OUT) == EINVAL, (name, d)
        assert f(0, ok, 10, BS, DS, QS, None, JE, 1.0, IN, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, None, 1.0, IN, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, None, -1e-300, IN, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, None, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, None) == EINVAL, name
        for lam in (math.inf, -math.inf, math.nan):
            assert f(0, ok, 10, BS, DS, QS, GE, JE, lam, IN, OUT) == EINVAL, (name, lam)
            assert f(0, ok, 10, BS, DS, QS, GE, None, lam, IN, OUT) == EINVAL, (name, lam)
        # ... a null je with lambda == 0 passes (3): with an odd ge the call reaches step (4)
        assert f(0, ok, 10, BS, DS, QS, GE + 1, None, 0.0, IN, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, QS, GE + 1, None, -0.0, IN, OUT) == EALIGN, name
        # (3) before (4)
        assert f(0, ok, 10, BS, DS, QS, GE + 1, None, 1.0, IN, OUT) == EINVAL, name
        # (4) each odd address; je only with lambda != 0
        for d in range(dim):
            odd = lambda t: tuple(t[x] + 1 if x == d else t[x] for x in range(3))      # noqa: E731
            assert f(0, ok, 10, odd(BS), DS, QS, GE, JE, 1.0, IN, OUT) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, odd(DS), QS, GE, JE, 1.0, IN, OUT) == EALIGN, (name, d)
            assert f(0, ok, 10, BS, DS, odd(QS), GE, JE, 1.0, IN, OUT) == EALIGN, (name, d)
        assert f(0, ok, 10, BS, DS, QS, GE + 1, JE, 1.0, IN, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE + 1, 1.0, IN, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN + 1, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, OUT + 1) == EALIGN, name
        # (4) before (5)
        assert f(0, ok, 10, BS, DS, QS, GE + 1, JE, 1.0, IN, IN) == EALIGN, name
        # (5) overlap: out == in, out on ge, out ending inside / starting at the last scalar of ge, out on je, out
        # straddling the ends of in; one scalar past the end of ge or je is no overlap
        modes = size * 10 * 7 ** dim
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, IN) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, GE) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, GE + size * (10 * ncomp - 1)) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, GE - modes + size) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, JE) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, JE + size * 9) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, IN + modes - 16) == EINVAL, name
        assert f(0, ok, 10, BS, DS, QS, GE, JE, 1.0, IN, IN - modes + 16) == EINVAL, name
        # ... and overlap is refused before the extent bounds and the variant are looked at
        big = 13 if dim == 3 else 33
        assert f(0, (big, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, IN) == EINVAL, name
        # (6) extents above the fallback's bounds; the byte ranges end where ge / je end
        for ext in ((big, 8, 8), (8, big, 8)) + (((8, 8, big),) if dim == 3 else ()):
            assert f(0, ext, 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == ENOTBUILT, (name, ext)
        assert f(0, (big, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, GE + size * 10 * ncomp) == ENOTBUILT, name
        assert f(0, (big, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, JE + size * 10) == ENOTBUILT, name
    for name, dim, size, f in _calls(lib)[:2]:
        # (1) variant out of range
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == EINVAL, (name, v)
        assert f(-1, (8, 8, 8), 0, N, N, N, None, None, 1.0, None, None) == EINVAL, name
        # (5) before (7)
        assert f(2, (8, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, IN) == EINVAL, name
        # (6) before (7)
        assert f(2, (13, 8, 8) if dim == 3 else (33, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == ENOTBUILT, name
        # (7) the variants that have no fused kernel: thread, block-lds, block-glb, mfma, mfma4, wave-rt
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, (8, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == ENOTBUILT, (name, v)
        # WAVE off its table (anisotropic, or above nq 8 / 16) and WAVE on 8-byte-aligned in / out
        assert f(1, (6, 6, 12) if dim == 3 else (4, 9, 0), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == ENOTBUILT, name
        assert f(1, (9, 9, 9) if dim == 3 else (17, 17, 17), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT) == ENOTBUILT, name
        assert f(1, (8, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN + 8, OUT) == EALIGN, name
        assert f(1, (8, 8, 8), 10, BS, DS, QS, GE, JE, 1.0, IN, OUT + 8) == EALIGN, name


def test_inputs_may_overlap_each_other_and_je_is_ignored_at_lambda_zero(pkg):
    """Inputs overlapping each other pass validation (all are only read): with an unsupported variant the call reaches
    step (7), SF_ENOTBUILT, and not the overlap refusal of step (5).  With lambda == 0, `je` is no argument at all: it
    may be null, odd, or overlap `out`."""
    lib = pkg.capi.lib()
    B, G, OUT = 0x10000, 0x100000, 0x400000
    h, q = lib.sf_affine_helmholtz_hex_f64_variant, lib.sf_affine_helmholtz_quad_f64_variant
    nine = (B,) * 9
    assert h(2, 8, 8, 8, 10, *nine, G, G, 1.0, G, OUT, None) == ENOTBUILT       # in == ge == je, bases == derivs == qw
    assert h(2, 8, 8, 8, 10, *nine, G, G + 64, 1.0, G + 128, OUT, None) == ENOTBUILT
    assert q(2, 8, 8, 10, *(B,) * 6, G, G, 1.0, G, OUT, None) == ENOTBUILT
    assert h(2, 8, 8, 8, 10, *nine, G, G, 1.0, G, G, None) == EINVAL
    assert h(2, 8, 8, 8, 10, *nine, G, OUT, 1.0, 0x300000, OUT, None) == EINVAL      # out == je, lambda != 0
    assert h(2, 8, 8, 8, 10, *nine, G, OUT, 0.0, 0x300000, OUT, None) == ENOTBUILT   # ... lambda == 0
    assert h(2, 8, 8, 8, 10, *nine, G, OUT + 1, 0.0, 0x300000, OUT, None) == ENOTBUILT
    assert h(2, 8, 8, 8, 10, *nine, G, None, 0.0, 0x300000, OUT, None) == ENOTBUILT
    assert q(2, 8, 8, 10, *(B,) * 6, G, OUT + 1, 0.0, 0x300000, OUT, None) == ENOTBUILT
    assert q(2, 8, 8, 10, *(B,) * 6, G, OUT, 0.5, 0x300000, OUT, None) == EINVAL


def test_affine_python_checks_sizes_without_gpu(pkg):
    import torch
    f64 = torch.float64
    b, d, q = torch.zeros(56, dtype=f64), torch.zeros(64, dtype=f64), torch.zeros(8, dtype=f64)
    x3, j3, g3 = torch.zeros(2 * 343, dtype=f64), torch.zeros(2, dtype=f64), torch.zeros(2 * 6, dtype=f64)
    x2, j2, g2 = torch.zeros(2 * 49, dtype=f64), torch.zeros(2, dtype=f64), torch.zeros(2 * 3, dtype=f64)
    hx, qd = pkg.affine_helmholtz_hex, pkg.affine_helmholtz_quad
    e3, e2 = (8, 8, 8), (8, 8)
    with pytest.raises(ValueError):      # inp not a whole number of elements
        hx(e3, b, b, b, d, d, d, q, q, q, g3, j3, 1.0, torch.zeros(2 * 343 - 1, dtype=f64))
    with pytest.raises(ValueError):      # ge
        hx(e3, b, b, b, d, d, d, q, q, q, g3[:-1], j3, 1.0, x3)
    with pytest.raises(ValueError):      # ge with five components
        hx(e3, b, b, b, d, d, d, q, q, q, g3[:10], j3, 1.0, x3)
    with pytest.raises(ValueError):      # ge expanded to planes
        hx(e3, b, b, b, d, d, d, q, q, q, torch.zeros(2 * 6 * 512, dtype=f64), j3, 1.0, x3)
    with pytest.raises(ValueError):      # je
        hx(e3, b, b, b, d, d, d, q, q, q, g3, j3[:-1], 1.0, x3)
    with pytest.raises(ValueError):      # je=None needs lam == 0
        hx(e3, b, b, b, d, d, d, q, q, q, g3, None, 0.5, x3)
    with pytest.raises(ValueError):      # out
        hx(e3, b, b, b, d, d, d, q, q, q, g3, j3, 1.0, x3, out=torch.zeros(2 * 343 + 1, dtype=f64))
    with pytest.raises(ValueError):      # a basis
        hx(e3, b, b[:55], b, d, d, d, q, q, q, g3, j3, 1.0, x3)
    with pytest.raises(ValueError):      # a derivative matrix
        hx(e3, b, b, b, d, d[:56], d, q, q, q, g3, j3, 1.0, x3)
    with pytest.raises(ValueError):      # a weight array
        hx(e3, b, b, b, d, d, d, q, q[:7], q, g3, j3, 1.0, x3)
    with pytest.raises(ValueError):      # dtype of ge
        hx(e3, b, b, b, d, d, d, q, q, q, g3.float(), j3, 1.0, x3)
    with pytest.raises(ValueError):      # dtype of je
        hx(e3, b, b, b, d, d, d, q, q, q, g3, j3.float(), 1.0, x3)
    with pytest.raises(ValueError):      # dtype of a weight array
        hx(e3, b, b, b, d, d, d, q, q, q.float(), g3, j3, 1.0, x3)
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q, q, g2, j2, 1.0, torch.zeros(2 * 49 + 3, dtype=f64))
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q, q, g2[:5], j2, 1.0, x2)
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q, q, g2, j2[:1], 1.0, x2)
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q, q, g2, None, 1.0, x2)
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q, q, g2, j2, 1.0, x2, out=torch.zeros(97, dtype=f64))
    with pytest.raises(ValueError):
        qd(e2, b, b, d[:63], d, q, q, g2, j2, 1.0, x2)
    with pytest.raises(ValueError):
        qd(e2, b, b, d, d, q[:9 - 2], q, g2, j2, 1.0, x2)
    with pytest.raises(ValueError):      # dtype of a derivative matrix
        qd(e2, b, b, d, d.float(), q, q, g2, j2, 1.0, x2)
    with pytest.raises(ValueError):      # float32 has the AUTO route only
        qd(e2, b.float(), b.float(), d.float(), d.float(), q.float(), q.float(), g2.float(), j2.float(), 1.0, x2.float(),
           variant="wave")


CASES = [((8, 8, 8), 3), ((5, 5, 5), 4), ((3, 3, 3), 6), ((2, 2, 2), 5), ((6, 6, 12), 2), ((3, 5, 4), 5), ((8, 8), 7),
         ((16, 16), 3), ((4, 9), 9), ((2, 2), 4)]


def _data(nq, nelmt, seed=0):
    """All data uniform in (-1, 1), the signs of qw and ge included."""
    rng = np.random.default_rng(2000 + seed + 17 * sum(nq))
    nm = [q - 1 for q in nq]
    nmt = int(np.prod(nm))
    dim = len(nq)
    bases = [rng.uniform(-1, 1, nm[d] * nq[d]) for d in range(dim)]
    derivs = [rng.uniform(-1, 1, nq[d] * nq[d]) for d in range(dim)]
    qws = [rng.uniform(-1, 1, nq[d]) for d in range(dim)]
    ge = rng.uniform(-1, 1, nelmt * len(COMPONENTS[dim]))
    je = rng.uniform(-1, 1, nelmt)
    x = rng.uniform(-1, 1, nelmt * nmt)
    return bases, derivs, qws, ge, je, x


_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


def test_bound_constants():
    assert affine_n((8, 8, 8)) == helm_n((8, 8, 8)) + 3 == 76
    assert affine_n((4, 9)) == helm_n((4, 9)) + 2 == 53


def test_expansion_layout():
    """g[e][c][k][j][i] = ge[e][c] qw2[k] qw1[j] qw0[i], w[e][k][j][i] = je[e] qw2[k] qw1[j] qw0[i]."""
    nq, nelmt = (3, 5, 4), 2
    _, _, qws, ge, je, _ = _data(nq, nelmt)
    g, w = expand(nq, nelmt, qws, ge, je, np.float64)
    g, w = g.reshape(nelmt, 6, 4, 5, 3), w.reshape(nelmt, 4, 5, 3)
    for e, c, k, j, i in ((0, 0, 0, 0, 0), (1, 4, 3, 2, 1), (1, 5, 3, 4, 2), (0, 2, 1, 4, 0)):
        q = qws[2][k] * (qws[1][j] * qws[0][i])
        assert g[e, c, k, j, i] == ge[e * 6 + c] * q and w[e, k, j, i] == je[e] * q
    g2, w2 = expand((4, 9), 3, [qws[2], np.arange(9.0)], np.arange(9.0), None, np.float64)
    assert w2 is None and g2.reshape(3, 3, 9, 4)[2, 1, 5, 3] == 7.0 * (5.0 * qws[2][3])


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_reference_is_the_dense_operator_on_expanded_data(nq, nelmt):
    """The affine reference against the element matrix of helm_ref.dense_operator on the expanded planes."""
    bases, derivs, qws, ge, je, x = _data(nq, nelmt)
    nmt = int(np.prod([q - 1 for q in nq]))
    g, w = expand(nq, nelmt, qws, ge, je)
    for lam, jj in ((0.75, je), (0.0, None)):
        ref, absref = ref_affine(nq, nelmt, bases, derivs, qws, ge, jj, lam, x)
        dense = np.empty_like(ref)
        for e in range(nelmt):
            A = dense_operator(nq, bases, derivs, g.reshape(nelmt, -1)[e], None if jj is None else w.reshape(nelmt, -1)[e],
                               lam)
            assert np.max(np.abs(A - A.T)) <= 1e-15 * np.max(np.abs(A))
            dense[e * nmt:(e + 1) * nmt] = A @ x[e * nmt:(e + 1) * nmt].astype(np.longdouble)
        q = affine_excess(dense, ref, absref, nq, U64)
        print(f"{nq} lam={lam}: max |dense - ref| / (gamma_N' absref) = {q:.3g}")
        assert q <= 1e-2
        assert float(np.max(np.abs(ref))) > 0 and float(np.min(absref)) > 0


@pytest.mark.parametrize("nq,nelmt", CASES, ids=_id)
def test_fp64_and_fp32_evaluations_sit_inside_the_bound(nq, nelmt):
    """numpy evaluations of the documented order in fp64 and fp32, and sf_helmholtz semantics on planes expanded in
    working precision, against the long-double reference: inside gamma_N' absref, with room."""
    bases, derivs, qws, ge, je, x = _data(nq, nelmt)
    f = np.float32
    b32, d32, q32 = [b.astype(f) for b in bases], [d.astype(f) for d in derivs], [q.astype(f) for q in qws]
    ge32, je32, x32 = ge.astype(f), je.astype(f), x.astype(f)
    for lam, jj, jj32 in ((0.75, je, je32), (0.0, None, None)):
        ref, absref = ref_affine(nq, nelmt, bases, derivs, qws, ge, jj, lam, x)
        e64 = affine_excess(affine_eval(nq, nelmt, bases, derivs, qws, ge, jj, lam, x, np.float64), ref, absref, nq, U64)
        g64, w64 = expand(nq, nelmt, qws, ge, jj, np.float64)
        h64 = affine_excess(helmholtz_f64(nq, nelmt, bases, derivs, g64, w64, lam, x)[0], ref, absref, nq, U64)
        r32, a32 = ref_affine(nq, nelmt, b32, d32, q32, ge32, jj32, lam, x32)
        o32 = affine_eval(nq, nelmt, b32, d32, q32, ge32, jj32, lam, x32, f)
        assert o32.dtype == f
        e32 = affine_excess(o32, r32, a32, nq, U32)
        print(f"{nq} lam={lam}: fp64 {e64:.3g}, expanded fp64 {h64:.3g}, fp32 {e32:.3g} of gamma_N' absref")
        assert 0 < e64 <= 1.0 and h64 <= 1.0 and 0 < e32 <= 1.0


@pytest.mark.parametrize("dim,nq", [(3, 5), (3, 8), (2, 8), (2, 12)], ids=["3d-nq5", "3d-nq8", "2d-nq8", "2d-nq12"])
def test_affine_null_space_and_energy(dim, nq):
    """Legendre basis at the GLL points, GLL D and weights, J_e = I + 0.3 U(-1, 1), ge = |det J| J^-1 J^-T: a constant is in
    the null space of the Laplacian and x^T A x is the exact int |grad u|^2 over the physical element (mixed terms
    included), in fp64 numpy within the bounds the GPU tests use."""
    nelmt, ext = 3, (nq,) * dim
    nmt = (nq - 1) ** dim
    bases, derivs, qws = gll_affine_setup(nq, dim)
    J, ge, je = affine_geometry(dim, nelmt, 11 + nq)
    assert np.all(je > 0.1)
    const = np.zeros((nelmt, nmt))
    const[:, 0] = 1.0 + np.arange(nelmt)
    got = affine_eval(ext, nelmt, bases, derivs, qws, ge, None, 0.0, const.reshape(-1), np.float64)
    ref, absref = ref_affine(ext, nelmt, bases, derivs, qws, ge, None, 0.0, const.reshape(-1))
    assert affine_excess(got, ref, absref, ext, U64) <= 1.0
    assert float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))) <= gamma(affine_n(ext), U64) * float(np.max(absref))
    x = np.random.default_rng(5).uniform(-1, 1, nelmt * nmt)
    y = affine_eval(ext, nelmt, bases, derivs, qws, ge, None, 0.0, x, np.float64)
    _, yabs = ref_affine(ext, nelmt, bases, derivs, qws, ge, None, 0.0, x)
    got = per_element_dots(y, x, nelmt)
    slack = symmetry_bound(ext, U64) * per_element_dots(np.asarray(yabs, dtype=np.float64), np.abs(x), nelmt)
    for e in range(nelmt):
        exact = exact_energy_affine(nq, dim, x.reshape(nelmt, -1)[e], J[e])
        print(f"{ext} element {e}: relative {abs(got[e] - exact) / exact:.3e}, of the bound {abs(got[e] - exact) / slack[e]:.3g}")
        assert exact > 0 and abs(got[e] - exact) <= slack[e]
    # the mixed terms matter: with the off-diagonal components dropped the energy is off by far more than the slack
    nc = len(COMPONENTS[dim])
    diag = ge.reshape(nelmt, nc).copy()
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        if a != b:
            diag[:, c] = 0.0
    yd = affine_eval(ext, nelmt, bases, derivs, qws, diag.reshape(-1), None, 0.0, x, np.float64)
    gd = per_element_dots(yd, x, nelmt)
    assert all(abs(gd[e] - got[e]) > 1e3 * slack[e] for e in range(nelmt))


NAME = re.compile(r"(hex|quad)_affine_wave_kernel<(\d+), .*(double|float)>")


def test_wave_instantiations_use_no_scratch():
    """Every affine wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..8 and 2D
    nq 2..16 for double and float, each with and without the mass term (88 kernels).  Prints VGPRs / occupancy per kernel
    (the table of DESIGN.md s4.12)."""
    got = set()
    for src, r in kernel_resources(("affine.hip", "affine_f32.hip"), "_wave_kernel"):      # no wave kernel of another family
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, t, flag = 3 if m.group(1) == "hex" else 2, int(m.group(2)), m.group(3), ", true, " in r.name
        assert (t == "float") == (src == "affine_f32.hip"), (src, r.name)
        assert (dim, nq, t, flag) not in got, r.name
        got.add((dim, nq, t, flag))
        print(f"{dim}D nq {nq:2d} {t:6s} {'helmholtz' if flag else 'laplacian'}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, "
              f"occupancy {r.occ}")
    orders = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
    want = {(d, n, t, h) for d, n in orders for t in ("double", "float") for h in (True, False)}
    assert len(want) == 88 and got == want, sorted(want ^ got)


def test_header_documents_affine():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "#define SF_VERSION 100" in text
    block = text[text.index("The fused Helmholtz operator on AFFINE elements"):text.index("int sf_affine_helmholtz_hex_f64(")]
    for needle in ("G_ab,e[k][j][i] = ge[e][ab] * qw2[k] qw1[j] qw0[i]", "w_e[k][j][i] = je[e] * qw2[k] qw1[j] qw0[i]",
                   "(00, 01, 02, 11, 12, 22)", "(00, 01, 11)", "|det J_e| J_e^-1 J_e^-T", "one-dimensional quadrature",  # layout
                   "q = qw2[k] * (qw1[j] * qw0[i])", "f_a = q * (sum_b ge_ab du_b), b ascending",
                   "(((lambda je_e) * q) * u + D_0^T f_0) + D_1^T f_1", "k -> r', j -> q', i -> p'",                 # order
                   "a null je with lambda != 0", "not finite", "`out` overlapping", "may be NULL",                    # validation
                   "(je only if lambda != 0)", "2 nm^d + d(d+1)/2 + 1",
                   "capture-safe", "NOT in-place safe", "3D nq 9..11"):
        assert needle in block, needle
