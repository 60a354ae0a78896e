"""CPU-side checks of the tensor-product apply with independent input / output extents (include/sumfact.h sf_tensor_*):
the test reference (tests/tensor_ref.py) against a dense contraction, against deliberately wrong ones and against the
references of BwdTrans and IProductWRTBase; the adjoint identity; the exports and the validation table with dummy
pointers and no device; the run-time specialisation's compile half through bin/sf_rtc_check; and the scratch budget of
every kernel of the compiled table (hipcc cross-compiles, no GPU needed)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import bwd_ref
import iprod_ref
from resources_ref import RTC_ROW, kernel_resources
from tensor_ref import (U32, U64, adjoint_bound, dense_tensor, gamma, per_element_dots, ref_tensor, tensor_excess,
                        tensor_n)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")
CHECK = os.path.join(PKG, "bin", "sf_rtc_check")

EXPORTS = ["sf_tensor_hex_f64", "sf_tensor_hex_f64_variant", "sf_tensor_quad_f64", "sf_tensor_quad_f64_variant",
           "sf_tensor_hex_f32", "sf_tensor_hex_f32_variant", "sf_tensor_quad_f32", "sf_tensor_quad_f32_variant",
           "sf_specialise_tensor", "sf_tensor_specialisation_state"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3

# (ni, no): more outputs than inputs, fewer, equal, extents of 1, both dimensions
SHAPES = [((4, 4, 4), (7, 7, 7)), ((7, 7, 7), (4, 4, 4)), ((5, 3, 6), (8, 3, 4)), ((1, 2, 5), (4, 2, 1)),
          ((3, 3), (3, 3)), ((1, 9), (4, 3)), ((10, 6), (15, 9))]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not (os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")) and os.path.exists(CHECK)):
        ge.build()
    return ge.load_package()


def _data(ni, no, nelmt, seed):
    rng = np.random.default_rng(seed)
    mats = [rng.uniform(-1, 1, a * b) for a, b in zip(ni, no)]
    return mats, rng.uniform(-1, 1, nelmt * int(np.prod(ni)))


def _id(v):
    return ">".join("x".join(map(str, t)) for t in v) if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v)


# ---- the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_reference_equals_a_dense_contraction(shape, trans):
    ni, no = shape
    nelmt = 3
    mats, x = _data(ni, no, nelmt, 5)
    ref, absref = ref_tensor(ni, no, trans, nelmt, mats, x)
    dense = dense_tensor(ni, no, trans, nelmt, mats, x)
    assert ref.size == nelmt * int(np.prod(no))
    # both in long double: they differ by the order of summation only, far inside the fp64 bound
    assert tensor_excess(dense, ref, absref, ni, U64) <= 2.0 ** -8
    assert np.max(np.abs(np.asarray(ref, dtype=np.float64))) > 0


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != (3, 3)], ids=_id)
def test_reference_tells_wrong_contractions_apart(shape):
    """A transposed matrix and swapped directions are not within the bound of the reference."""
    ni, no = shape
    nelmt = 2
    mats, x = _data(ni, no, nelmt, 6)
    ref, absref = ref_tensor(ni, no, 0, nelmt, mats, x)
    # the matrix of the first direction with more than one row and column, stored in the other layout
    d = next(k for k in range(len(ni)) if ni[k] > 1 and no[k] > 1)
    wrong = list(mats)
    wrong[d] = mats[d].reshape(ni[d], no[d]).T.copy().reshape(-1)
    bad = dense_tensor(ni, no, 0, nelmt, wrong, x)
    assert tensor_excess(bad, ref, absref, ni, U64) > 1e6
    # directions 0 and 1 swapped, where their shapes allow it
    if ni[0] == ni[1] and no[0] == no[1]:
        swapped = [mats[1], mats[0]] + list(mats[2:])
        bad = dense_tensor(ni, no, 0, nelmt, swapped, x)
        assert tensor_excess(bad, ref, absref, ni, U64) > 1e6


def test_trans_reads_the_transposed_layout():
    ni, no, nelmt = (3, 5), (4, 2), 2
    mats, x = _data(ni, no, nelmt, 7)
    r0, _ = ref_tensor(ni, no, 0, nelmt, mats, x)
    flipped = [m.reshape(a, b).T.copy().reshape(-1) for m, a, b in zip(mats, ni, no)]
    r1, _ = ref_tensor(ni, no, 1, nelmt, flipped, x)
    assert np.array_equal(r0, r1)
    r2, a2 = ref_tensor(ni, no, 1, nelmt, mats, x)
    assert tensor_excess(r2, r0, a2, ni, U64) > 1e6


@pytest.mark.parametrize("nq", [(4, 4, 4), (3, 5, 4), (8, 8), (4, 9)], ids=lambda v: "x".join(map(str, v)))
def test_reference_equals_the_bwdtrans_and_iproduct_references(nq):
    nelmt = 3
    nm = tuple(q - 1 for q in nq)
    rng = np.random.default_rng(8)
    bases = [rng.uniform(-1, 1, a * b) for a, b in zip(nm, nq)]
    x = rng.uniform(-1, 1, nelmt * int(np.prod(nm)))
    y = rng.uniform(-1, 1, nelmt * int(np.prod(nq)))
    ref, absref = ref_tensor(nm, nq, 0, nelmt, bases, x)
    bref, babs = bwd_ref.ref_bwdtrans(nq, nelmt, bases, x)
    assert np.array_equal(ref, bref) and np.array_equal(absref, babs)
    assert tensor_n(nm) == bwd_ref.bwd_n(nq)
    ref, absref = ref_tensor(nq, nm, 1, nelmt, bases, y)
    iref, iabs = iprod_ref.ref_iprod(nq, nelmt, bases, y)
    assert np.array_equal(ref, iref) and np.array_equal(absref, iabs)
    assert tensor_n(nq) == sum(nq)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_adjoint_identity(shape):
    """<A x, y> == <x, A^T y> with A^T the same arrays, trans flipped and ni / no swapped, both applies rounded to fp64:
    within adjoint_bound * <|A||x|, |y|>."""
    ni, no = shape
    nelmt = 4
    mats, x = _data(ni, no, nelmt, 9)
    y = np.random.default_rng(10).uniform(-1, 1, nelmt * int(np.prod(no)))
    ax, aabs = ref_tensor(ni, no, 0, nelmt, mats, x)
    aty, _ = ref_tensor(no, ni, 1, nelmt, mats, y)
    lhs = math.fsum(per_element_dots(np.asarray(ax, dtype=np.float64), y, nelmt))
    rhs = math.fsum(per_element_dots(x, np.asarray(aty, dtype=np.float64), nelmt))
    scale = math.fsum(per_element_dots(np.asarray(aabs, dtype=np.float64), np.abs(y), nelmt))
    bound = adjoint_bound(ni, no, U64) * scale
    print(f"{ni}->{no}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0
    assert gamma(tensor_n(ni), U32) > gamma(tensor_n(ni), U64) > 0


# ---- exports and validation ----------------------------------------------------------------------------------------------
def test_tensor_exports(pkg):
    lib = pkg.capi.lib()
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
    for name in ("tensor_hex", "tensor_quad", "specialise_tensor", "tensor_specialisation_state", "tensor_autograd"):
        assert callable(getattr(pkg, name)), name


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, ni, no, trans, nelmt, m, in, out))"""
    def make(fn, dim):
        def call(v, ni, no, tr, n, m, i, o):
            return fn(v, *ni[:dim], *no[:dim], tr, n, *([m] * dim), i, o, None)
        return call
    return [("hex64", 3, 8, make(lib.sf_tensor_hex_f64_variant, 3)), ("quad64", 2, 8, make(lib.sf_tensor_quad_f64_variant, 2)),
            ("hex32", 3, 4, make(lib.sf_tensor_hex_f32_variant, 3)), ("quad32", 2, 4, make(lib.sf_tensor_quad_f32_variant, 2))]


def test_tensor_argument_validation_without_gpu(pkg):
    """The validation table of include/sumfact.h, in its order, before any HIP call: dummy pointers, no device."""
    lib = pkg.capi.lib()
    M, IN, OUT = 0x10000, 0x200000, 0x400000    # fake device addresses: never touched on these paths
    for name, dim, sb, f in _calls(lib):
        ni, no = (4, 4, 4), (6, 6, 6)
        # an extent of 0, on either side, wins over everything else
        for d in range(dim):
            z = tuple(0 if k == d else 4 for k in range(3))
            assert f(0, z, no, 0, 10, M, IN, OUT) == EINVAL, (name, z)
            assert f(0, ni, z, 0, 10, M, IN, OUT) == EINVAL, (name, z)
            assert f(0, z, no, 0, 0, None, None, None) == EINVAL, (name, z)
        # trans other than 0 / 1, a variant outside the enum
        for tr in (-1, 2, 7):
            assert f(0, ni, no, tr, 10, M, IN, OUT) == EINVAL, (name, tr)
        for v in (-1, 9, 99):
            assert f(v, ni, no, 0, 10, M, IN, OUT) == EINVAL, (name, v)
            assert f(v, ni, no, 0, 0, None, None, None) == EINVAL, (name, v)
        # nelmt == 0: nothing to do
        assert f(0, ni, no, 1, 0, None, None, None) == 0, name
        # null pointers with nelmt > 0
        assert f(0, ni, no, 0, 10, None, IN, OUT) == EINVAL, name
        assert f(0, ni, no, 0, 10, M, None, OUT) == EINVAL, name
        assert f(0, ni, no, 0, 10, M, IN, None) == EINVAL, name
        # a pointer not aligned to the scalar
        for off in (1, sb // 2):
            assert f(0, ni, no, 0, 10, M + off, IN, OUT) == EALIGN, (name, off)
            assert f(0, ni, no, 0, 10, M, IN + off, OUT) == EALIGN, (name, off)
            assert f(0, ni, no, 0, 10, M, IN, OUT + off) == EALIGN, (name, off)
        # out overlapping in: the same array, and the last byte of in
        nin = sb * 10 * 4 ** dim
        assert f(0, ni, no, 0, 10, M, IN, IN) == EINVAL, name
        assert f(0, ni, no, 0, 10, M, IN, IN + nin - sb) == EINVAL, name
        assert f(5, ni, no, 0, 10, M, IN, IN + nin - sb) == EINVAL, name
        # extents beyond the fallback's bounds, in or out
        big = 17 if dim == 3 else 33
        for d in range(dim):
            z = tuple(big if k == d else 4 for k in range(3))
            assert f(0, z, no, 0, 10, M, IN, OUT) == ENOTBUILT, (name, z)
            assert f(5, ni, z, 0, 10, M, IN, OUT) == ENOTBUILT, (name, z)
        # the variants the family does not take
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, ni, no, 0, 10, M, IN, OUT) == ENOTBUILT, (name, v)
        # WAVE off the table: an anisotropic shape, a pair the table lacks; WAVE on buffers aligned only to the scalar
        assert f(1, (5, 3, 6), (8, 3, 4), 0, 10, M, IN, OUT) == ENOTBUILT, name
        assert f(1, (4, 4, 4), (7, 7, 7), 0, 10, M, IN, OUT) == ENOTBUILT, name
        assert f(1, (4, 4, 4), (6, 6, 6), 0, 10, M, IN + sb, OUT) == EALIGN, name
        assert f(1, (4, 4, 4), (6, 6, 6), 1, 10, M, IN, OUT + sb) == EALIGN, name


def test_specialise_tensor_argument_validation_without_gpu(pkg):
    lib = pkg.capi.lib()
    n = ctypes.c_uint64(7)
    bad = [(1, 4, 4, 4, 7, 7, 7, 0, 8), (4, 4, 4, 4, 7, 7, 7, 0, 8), (3, 0, 4, 4, 7, 7, 7, 0, 8),
           (3, 4, 4, 4, 7, 7, 0, 0, 8), (3, 17, 4, 4, 7, 7, 7, 0, 8), (3, 4, 4, 4, 7, 17, 7, 0, 8),
           (2, 25, 4, 1, 7, 7, 1, 0, 8), (2, 4, 4, 1, 7, 25, 1, 1, 8), (2, 4, 0, 1, 7, 7, 1, 1, 8),
           (3, 4, 4, 4, 7, 7, 7, 2, 8), (3, 4, 4, 4, 7, 7, 7, -1, 8), (3, 4, 4, 4, 7, 7, 7, 0, 2),
           (2, 4, 4, 1, 7, 7, 1, 0, 16)]
    for args in bad:
        assert lib.sf_specialise_tensor(*args) == EINVAL, args
        assert lib.sf_tensor_specialisation_state(*args, None) == EINVAL, args
        assert lib.sf_tensor_specialisation_state(*args, ctypes.byref(n)) == EINVAL, args


def test_tensor_python_checks_sizes_without_gpu(pkg):
    import torch
    m = torch.zeros(28, dtype=torch.float64)
    with pytest.raises(ValueError):
        pkg.tensor_hex((4, 4, 4), (7, 7, 7), m, m, m, torch.zeros(63, dtype=torch.float64))
    with pytest.raises(ValueError):
        pkg.tensor_quad((4, 4), (7, 7), m[:27], m, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        pkg.tensor_quad((4, 4, 4), (7, 7), m, m, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(ValueError):
        pkg.tensor_autograd((4, 4), (7, 7), (m.clone().requires_grad_(True), m), torch.zeros(16, dtype=torch.float64))


# ---- the compile half of the run-time specialisation -----------------------------------------------------------------------
RTC_SHAPES = ["4>7x4>7x4>7", "7>4x7>4x7>4:t", "5>8x3>3x6>4", "1>4x9>3", "10>15x10>15", "7>8x7>8x7>8",
              "4>7x4>7x4>7:f32", "9>6x9>6:t:f32"]


def _run_check(*shapes):
    r = subprocess.run([CHECK, *shapes], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout.splitlines()


def test_rtc_check_compiles_tensor_shapes_without_scratch(pkg):
    rc, lines = _run_check(*RTC_SHAPES)
    assert rc == 0, "\n".join(lines)
    assert lines[0].startswith("source-hash ")
    rows = {}
    for ln in lines[1:]:
        m = RTC_ROW.match(ln)
        assert m, f"unparsed sf_rtc_check line: {ln!r}"
        rows[m.group(3) + (":f32" if m.group(1) == "fp32" else "")] = m
    assert sorted(rows) == sorted(RTC_SHAPES)
    for s, m in rows.items():
        assert int(m.group(7)) == 0 and int(m.group(8)) == 0 and int(m.group(9)) == 0 and m.group(15) == "ok", (s, m.string)
        assert 0 < int(m.group(4)) <= 256 and 0 < int(m.group(11)) <= 64 * 1024, (s, m.string)


def test_rtc_check_agrees_with_bwdtrans_on_its_shape(pkg):
    """(7 -> 8)^3 is the geometry of BwdTrans 8x8x8: the same chunk, workgroup and LDS."""
    _, lines = _run_check("7>8x7>8x7>8", "8x8x8")
    a, b = RTC_ROW.match(lines[1]), RTC_ROW.match(lines[2])
    assert a and b, lines
    assert [a.group(k) for k in (11, 12, 13)] == [b.group(k) for k in (11, 12, 13)], lines


def test_rtc_check_reports_a_shape_beyond_the_slab_limit_as_refused(pkg):
    """1 -> 16, 16 -> 1, 16 -> 1: the first intermediate of two elements, 2*16*16 pencils of stride 17, is 69632 bytes."""
    rc, lines = _run_check("1>16x16>1x16>1", "4>6x4>6")
    assert rc == 1, "\n".join(lines)
    assert re.match(r"^fp64 3D 1>16x16>1x16>1\s+REFUSED\b.*69632", lines[1]), lines
    assert RTC_ROW.match(lines[2]) and lines[2].rstrip().endswith("ok"), lines


def test_rtc_check_rejects_malformed_tensor_shapes(pkg):
    rc, lines = _run_check("4>7x4", "0>3x2>2", "4>7x4>7:q", "17>3x2>2x2>2")
    assert rc == 4 and all("invalid shape" in ln for ln in lines[1:]), lines


# ---- the compiled table ---------------------------------------------------------------------------------------------------
HEX_PAIRS = [(n, n) for n in range(2, 9)] + [(n, -(-3 * n // 2)) for n in range(2, 7)] + \
            [(-(-3 * n // 2), n) for n in range(2, 7)]
QUAD_PAIRS = [(n, n) for n in range(2, 17)] + [(n, -(-3 * n // 2)) for n in range(2, 11)] + \
             [(-(-3 * n // 2), n) for n in range(2, 11)]
NAME = re.compile(r"(hex|quad)_tensor_wave_kernel<(.*), (double|float)>")


@pytest.mark.parametrize("unit,dim,scalar", [("tensor.hip", 3, "double"), ("tensor_quad.hip", 2, "double"),
                                             ("tensor_f32.hip", 3, "float"), ("tensor_quad_f32.hip", 2, "float")])
def test_table_kernels_use_no_scratch(unit, dim, scalar):
    got = set()
    for _, r in kernel_resources((unit,), "tensor_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m and (3 if m.group(1) == "hex" else 2) == dim and m.group(3) == scalar, r.name
        args = [int(a) for a in m.group(2).split(", ")]
        got.add((args[0], args[1], args[6 if dim == 3 else 4]))     # I0, O0, TR
    want = {(i, o, tr) for i, o in (HEX_PAIRS if dim == 3 else QUAD_PAIRS) for tr in (0, 1)}
    assert got == want, sorted(want ^ got)


def test_generic_kernels_use_no_scratch():
    rows = kernel_resources(("tensor_generic.hip",), "tensor_generic_kernel")
    assert len(rows) == 8, rows     # double / float x 2D / 3D x two LDS classes


def test_header_documents_tensor():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in EXPORTS:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "SF_NUM_VARIANTS       = 9" in text
    for needle in ("m_d[a*no_d + b]", "m_d[b*ni_d + a]", "ascending summed index", "capture-safe"):
        assert needle in text, needle
