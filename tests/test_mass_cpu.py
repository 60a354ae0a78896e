"""CPU-side checks of the fused mass operator (include/sumfact.h sf_mass_*): the exports and their Python binding, argument
validation before any HIP call (the overlap refusal included), the test reference (tests/mass_ref.py) against the pinned
oracle and its symmetry, and the register / scratch budget of every wave instantiation (hipcc cross-compiles, no GPU
needed)."""
import math
import os
import re

import numpy as np
import pytest

from iprod_ref import ref_iprod
from mass_ref import U64, gamma, mass_excess, mass_n, per_element_dots, ref_mass, symmetry_bound
from resources_ref import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

NEW = ["sf_mass_hex_f64", "sf_mass_hex_f64_variant", "sf_mass_quad_f64", "sf_mass_quad_f64_variant",
       "sf_mass_hex_f32", "sf_mass_quad_f32"]
EINVAL, EALIGN, ENOTBUILT = -1, -2, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def test_mass_exports(pkg):
    lib = pkg.capi.lib()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in pkg.capi.SYMBOLS, name
    for name in ("mass_hex", "mass_quad"):
        assert callable(getattr(pkg, name)), name


def _calls(lib):
    """(name, dim, scalar bytes, callable(variant, extents, nelmt, (b0, b1, b2), w, in, out)) for every entry point."""
    def hex64(v, e, n, b, w, i, o):
        return lib.sf_mass_hex_f64_variant(v, *e, n, *b, w, i, o, None)

    def quad64(v, e, n, b, w, i, o):
        return lib.sf_mass_quad_f64_variant(v, *e[:2], n, *b[:2], w, i, o, None)

    def hex32(v, e, n, b, w, i, o):
        assert v == 0
        return lib.sf_mass_hex_f32(*e, n, *b, w, i, o, None)

    def quad32(v, e, n, b, w, i, o):
        assert v == 0
        return lib.sf_mass_quad_f32(*e[:2], n, *b[:2], w, i, o, None)

    return [("hex64", 3, 8, hex64), ("quad64", 2, 8, quad64), ("hex32", 3, 4, hex32), ("quad32", 2, 4, quad32)]


def test_mass_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call, so it is testable on a machine without a GPU.  One assertion per step
    of the validation order of include/sumfact.h."""
    lib = pkg.capi.lib()
    # fake device addresses, far enough apart for 10 elements of 8^3 (w: 40 960 bytes): never touched on these paths
    B0, B1, B2, W, IN, OUT = 0x10000, 0x11000, 0x12000, 0x100000, 0x200000, 0x400000
    BS = (B0, B1, B2)
    N = (None, None, None)
    for name, dim, size, f in _calls(lib):
        ok = (8, 8, 8)
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(0, bad, 10, BS, W, IN, OUT) == EINVAL, (name, bad)
            assert f(0, bad, 0, N, None, None, None) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(0, ok, 0, N, None, None, None) == 0, name
        # (3) each null pointer, w included
        for d in range(dim):
            bs = tuple(None if x == d else BS[x] for x in range(3))
            assert f(0, ok, 10, bs, W, IN, OUT) == EINVAL, (name, d)
        assert f(0, ok, 10, BS, None, IN, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, W, None, OUT) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, None) == EINVAL, name
        # (4) each odd address
        for d in range(dim):
            bs = tuple(BS[x] + 1 if x == d else BS[x] for x in range(3))
            assert f(0, ok, 10, bs, W, IN, OUT) == EALIGN, (name, d)
        assert f(0, ok, 10, BS, W + 1, IN, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, W, IN + 1, OUT) == EALIGN, name
        assert f(0, ok, 10, BS, W, IN, OUT + 1) == EALIGN, name
        # (5) overlap: out == in, out == w, out starting inside in, out ending inside in, out inside w
        modes = size * 10 * 7 ** dim
        assert f(0, ok, 10, BS, W, IN, IN) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, W) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, IN + 16) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, IN + modes - 16) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, IN - modes + 16) == EINVAL, name
        assert f(0, ok, 10, BS, W, IN, W + 16) == EINVAL, name
        # ... and overlap is refused before the extent bounds and the variant are looked at
        big = 17 if dim == 3 else 33
        assert f(0, (big, 8, 8), 10, BS, W, IN, IN) == EINVAL, name
        # (6) extents above the fallback's bounds
        for ext in ((big, 8, 8), (8, big, 8)) + (((8, 8, big),) if dim == 3 else ()):
            assert f(0, ext, 10, BS, W, IN, OUT) == ENOTBUILT, (name, ext)
    for name, dim, size, f in _calls(lib)[:2]:
        # (1) variant out of range
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, BS, W, IN, OUT) == EINVAL, (name, v)
        assert f(-1, (8, 8, 8), 0, N, None, None, None) == EINVAL, name
        # (5) before (7)
        assert f(2, (8, 8, 8), 10, BS, W, IN, IN) == EINVAL, name
        # (7) the variants that have no fused kernel: thread, block-lds, block-glb, mfma, mfma4, wave-rt
        for v in (2, 3, 4, 6, 7, 8):
            assert f(v, (8, 8, 8), 10, BS, W, IN, OUT) == ENOTBUILT, (name, v)
        # WAVE off its table (anisotropic, or above nq 11 / 16) and WAVE on 8-byte-aligned in / out
        assert f(1, (6, 6, 12) if dim == 3 else (4, 9, 0), 10, BS, W, IN, OUT) == ENOTBUILT, name
        assert f(1, (12, 12, 12) if dim == 3 else (17, 17, 17), 10, BS, W, IN, OUT) == ENOTBUILT, name
        assert f(1, (8, 8, 8), 10, BS, W, IN + 8, OUT) == EALIGN, name
        assert f(1, (8, 8, 8), 10, BS, W, IN, OUT + 8) == EALIGN, name


def test_in_may_overlap_w(pkg):
    """`in` overlapping `w` passes validation (both are only read): with an unsupported variant the call then reaches
    step (7), SF_ENOTBUILT, and not the overlap refusal of step (5)."""
    lib = pkg.capi.lib()
    B, W, OUT = 0x10000, 0x100000, 0x400000
    assert lib.sf_mass_hex_f64_variant(2, 8, 8, 8, 10, B, B, B, W, W, OUT, None) == ENOTBUILT
    assert lib.sf_mass_hex_f64_variant(2, 8, 8, 8, 10, B, B, B, W, W + 64, OUT, None) == ENOTBUILT
    assert lib.sf_mass_quad_f64_variant(2, 8, 8, 10, B, B, W, W, OUT, None) == ENOTBUILT
    assert lib.sf_mass_hex_f64_variant(2, 8, 8, 8, 10, B, B, B, W, W, W, None) == EINVAL


def test_mass_python_checks_sizes_without_gpu(pkg):
    import torch
    f64 = torch.float64
    b = torch.zeros(56, dtype=f64)
    x3, w3 = torch.zeros(2 * 343, dtype=f64), torch.zeros(2 * 512, dtype=f64)
    x2, w2 = torch.zeros(2 * 49, dtype=f64), torch.zeros(2 * 64, dtype=f64)
    with pytest.raises(ValueError):      # inp not a whole number of elements
        pkg.mass_hex((8, 8, 8), b, b, b, w3, torch.zeros(2 * 343 - 1, dtype=f64))
    with pytest.raises(ValueError):      # w
        pkg.mass_hex((8, 8, 8), b, b, b, w3[:-1], x3)
    with pytest.raises(ValueError):      # out
        pkg.mass_hex((8, 8, 8), b, b, b, w3, x3, out=torch.zeros(2 * 343 + 1, dtype=f64))
    with pytest.raises(ValueError):      # a basis
        pkg.mass_hex((8, 8, 8), b, b[:55], b, w3, x3)
    with pytest.raises(ValueError):
        pkg.mass_quad((8, 8), b, b, w2, torch.zeros(2 * 49 + 3, dtype=f64))
    with pytest.raises(ValueError):
        pkg.mass_quad((8, 8), b, b, w2[:100], x2)
    with pytest.raises(ValueError):
        pkg.mass_quad((8, 8), b, b, w2, x2, out=torch.zeros(97, dtype=f64))
    with pytest.raises(ValueError):
        pkg.mass_quad((8, 8), b[:55], b, w2, x2)
    with pytest.raises(ValueError):      # float32 has the AUTO route only
        b32 = b.float()
        pkg.mass_quad((8, 8), b32, b32, w2.float(), x2.float(), variant="wave")


CASES = [((8, 8, 8), 5), ((3, 5, 4), 7), ((8, 8), 9), ((4, 9), 11)]     # tests/test_iproduct_cpu.py


def _data(oracle, nq, nelmt):
    nm = [q - 1 for q in nq]
    nmt, nqt = int(np.prod(nm)), int(np.prod(nq))
    bases = [oracle.fill_random(nm[d] * nq[d], 900 + d) for d in range(len(nq))]
    x = oracle.fill_random(nelmt * nmt, 31)
    y = oracle.fill_random(nelmt * nmt, 33)
    w = 0.25 + np.abs(oracle.fill_random(nelmt * nqt, 32))
    return bases, w, x, y


@pytest.mark.parametrize("nq,nelmt", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_reference_is_the_chain_through_the_oracle(oracle, nq, nelmt):
    """ref_mass(x) == ref_iprod(w * oracle.bwdtrans(x)) within gamma_N * absref: the fp64 oracle's forward error and the
    fp64 multiply are n + 1 of the N roundings the bound allows, the long-double halves add nothing visible."""
    bases, w, x, _ = _data(oracle, nq, nelmt)
    bwd = oracle.bwdtrans_hex if len(nq) == 3 else oracle.bwdtrans_quad
    chain, _ = ref_iprod(nq, nelmt, bases, w * bwd(tuple(nq), nelmt, *bases, x))
    ref, absref = ref_mass(nq, nelmt, bases, w, x)
    q = mass_excess(chain, ref, absref, nq, U64)
    print(f"{nq}: max |chain - ref| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0
    assert float(np.max(np.abs(ref))) > 0 and float(np.min(absref)) > 0


@pytest.mark.parametrize("nq,nelmt", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_reference_is_symmetric(oracle, nq, nelmt):
    """|<M x, y> - <x, M y>| <= 2 (gamma_N + gamma_m) sum_e <|M||x|, |y|>_e for the long-double reference."""
    bases, w, x, y = _data(oracle, nq, nelmt)
    mx, mabs = ref_mass(nq, nelmt, bases, w, x)
    my, _ = ref_mass(nq, nelmt, bases, w, y)
    lhs = math.fsum(per_element_dots(np.asarray(mx, dtype=np.float64), y, nelmt))
    rhs = math.fsum(per_element_dots(x, np.asarray(my, dtype=np.float64), nelmt))
    scale = math.fsum(per_element_dots(np.asarray(mabs, dtype=np.float64), np.abs(y), nelmt))
    bound = symmetry_bound(nq, U64) * scale
    print(f"{nq}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    assert abs(lhs) > 0
    # positive definite for w > 0
    assert math.fsum(per_element_dots(np.asarray(mx, dtype=np.float64), x, nelmt)) > 0


def test_bound_constants():
    assert mass_n((8, 8, 8)) == 49 and mass_n((4, 9)) == 27
    assert gamma(49, U64) == 49 * U64 / (1 - 49 * U64)


NAME = re.compile(r"(hex|quad)_mass_wave_kernel<(\d+), .*(double|float)>")


def test_wave_instantiations_use_no_scratch():
    """Every fused wave instantiation: no scratch, no spills, at most 256 VGPRs; the set is exactly 3D nq 2..11 and 2D
    nq 2..16 for double and float.  Prints VGPRs / occupancy per order (the table of DESIGN.md s4.10)."""
    got = set()
    for src, r in kernel_resources(("mass.hip", "mass_f32.hip"), "mass_wave_kernel"):
        m = NAME.fullmatch(r.name)
        assert m, r.name
        dim, nq, t = 3 if m.group(1) == "hex" else 2, int(m.group(2)), m.group(3)
        assert (t == "float") == (src == "mass_f32.hip"), (src, r.name)
        got.add((dim, nq, t))
        print(f"{dim}D nq {nq:2d} {t:6s}: {r.vgpr:3d} VGPRs, {r.sgpr:3d} SGPRs, occupancy {r.occ}")
    want = {(3, n, t) for n in range(2, 12) for t in ("double", "float")} | \
           {(2, n, t) for n in range(2, 17) for t in ("double", "float")}
    assert got == want, sorted(want ^ got)


def test_header_documents_mass():
    text = open(os.path.join(ROOT, "include", "sumfact.h")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
    assert "#define SF_VERSION 100" in text
    assert "SF_NUM_VARIANTS       = 9" in text
    for needle in ("capture-safe", "NOT in-place safe", "k -> r', j -> q', i -> p'", "overlapping", "sf_mass_*"):
        assert needle in text, needle
