"""CPU-side checks of the BwdTrans entry points (include/sumfact.h sf_bwdtrans_*): the return code of every path that
ends before a HIP call -- the validation order, the variant range, and what each explicit variant answers for extents
off its table or for 8-byte-aligned buffers -- the Python wrappers' size checks, and the binding's signatures."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-benchmarking_amd")

OK, EINVAL, EALIGN, ENOTBUILT = 0, -1, -2, -3
AUTO, WAVE, MFMA, MFMA4, WAVE_RT = 0, 1, 6, 7, 8


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(PKG, "lib", "libsumfact.so")):
        ge.build()
    return ge.load_package()


def _calls(lib):
    """(name, dim, takes a variant, callable(variant, extents, nelmt, (b0, b1, b2), in, wsp, out)): the six entry points."""
    def hex64v(v, e, n, b, i, w, o):
        return lib.sf_bwdtrans_hex_f64_variant(v, *e, n, *b, i, w, o, None)

    def quad64v(v, e, n, b, i, w, o):
        return lib.sf_bwdtrans_quad_f64_variant(v, *e[:2], n, *b[:2], i, w, o, None)

    def hex64(v, e, n, b, i, w, o):
        assert v == AUTO and w is None
        return lib.sf_bwdtrans_hex_f64(*e, n, *b, i, o, None)

    def quad64(v, e, n, b, i, w, o):
        assert v == AUTO and w is None
        return lib.sf_bwdtrans_quad_f64(*e[:2], n, *b[:2], i, o, None)

    def hex32(v, e, n, b, i, w, o):
        assert v == AUTO and w is None
        return lib.sf_bwdtrans_hex_f32(*e, n, *b, i, o, None)

    def quad32(v, e, n, b, i, w, o):
        assert v == AUTO and w is None
        return lib.sf_bwdtrans_quad_f32(*e[:2], n, *b[:2], i, o, None)

    return [("hex64", 3, True, hex64v), ("quad64", 2, True, quad64v), ("hex64-auto", 3, False, hex64),
            ("quad64-auto", 2, False, quad64), ("hex32", 3, False, hex32), ("quad32", 2, False, quad32)]


# fake device addresses, far enough apart for 10 elements of 17^3: never touched on these paths
B0, B1, B2, IN, WSP, OUT = 0x10000, 0x11000, 0x12000, 0x300000, 0x500000, 0x700000
BS, N = (B0, B1, B2), (None, None, None)


def test_bwdtrans_argument_validation_without_gpu(pkg):
    """Every refusal happens before any HIP call.  One block per step of the validation order of include/sumfact.h, for
    both dimensions and both scalar types."""
    for name, dim, has_variant, f in _calls(pkg.capi.lib()):
        ok = (8, 8, 8)
        # (1) an extent < 2, in every direction -- before the nelmt == 0 shortcut
        for bad in ((1, 8, 8), (8, 1, 8), (0, 8, 8)) + (((8, 8, 1),) if dim == 3 else ()):
            assert f(AUTO, bad, 10, BS, IN, None, OUT) == EINVAL, (name, bad)
            assert f(AUTO, bad, 0, N, None, None, None) == EINVAL, (name, bad)
        # (2) nelmt == 0 with null pointers: nothing to do
        assert f(AUTO, ok, 0, N, None, None, None) == OK, name
        # (3) each null pointer; the workspace may be null
        for d in range(dim):
            bs = tuple(None if x == d else BS[x] for x in range(3))
            assert f(AUTO, ok, 10, bs, IN, None, OUT) == EINVAL, (name, d)
        assert f(AUTO, ok, 10, BS, None, None, OUT) == EINVAL, name
        assert f(AUTO, ok, 10, BS, IN, None, None) == EINVAL, name
        if has_variant:
            assert f(AUTO, ok, 10, BS, None, WSP, OUT) == EINVAL, name
        # (4) each odd address, looked at after the nulls; a null workspace is not an argument of these steps
        for d in range(dim):
            bs = tuple(BS[x] + 1 if x == d else BS[x] for x in range(3))
            assert f(AUTO, ok, 10, bs, IN, None, OUT) == EALIGN, (name, d)
            assert f(AUTO, ok, 10, bs, None, None, OUT) == EINVAL, (name, d)
            assert f(AUTO, ok, 10, bs, IN, None, None) == EINVAL, (name, d)
        assert f(AUTO, ok, 10, BS, IN + 1, None, OUT) == EALIGN, name
        assert f(AUTO, ok, 10, BS, IN, None, OUT + 1) == EALIGN, name
        assert f(AUTO, ok, 10, (None, B1, B2), IN + 1, None, OUT) == EINVAL, name
        if has_variant:
            assert f(AUTO, ok, 10, BS, IN + 1, WSP, OUT) == EALIGN, name


def test_bwdtrans_variant_routing_without_gpu(pkg):
    """What the explicit variants answer without launching: out of range, off their table, anisotropic, or in / out
    that are only 8-byte aligned.  3D WAVE looks at the alignment first (its anisotropic table answers at launch); every
    other matrix-core / wave variant refuses anisotropic extents before it looks at the alignment."""
    calls = {name: f for name, _, _, f in _calls(pkg.capi.lib())}
    h, q = calls["hex64"], calls["quad64"]
    for f in (h, q):
        for v in (-1, 9, 99):
            assert f(v, (8, 8, 8), 10, BS, IN, None, OUT) == EINVAL, v
            assert f(v, (8, 8, 8), 0, N, None, None, None) == EINVAL, v
    # 3D WAVE
    assert h(WAVE, (8, 8, 8), 10, BS, IN + 8, None, OUT) == EALIGN
    assert h(WAVE, (8, 8, 8), 10, BS, IN, None, OUT + 8) == EALIGN
    assert h(WAVE, (5, 9, 13), 10, BS, IN + 8, None, OUT) == EALIGN
    assert h(WAVE, (5, 9, 13), 10, BS, IN, None, OUT) == ENOTBUILT
    assert h(WAVE, (12, 12, 12), 10, BS, IN, None, OUT) == ENOTBUILT
    # 3D MFMA / MFMA4
    assert h(MFMA, (8, 8, 4), 10, BS, IN + 8, None, OUT) == ENOTBUILT
    assert h(MFMA, (8, 8, 8), 10, BS, IN + 8, None, OUT) == EALIGN
    assert h(MFMA, (3, 3, 3), 10, BS, IN, None, OUT) == ENOTBUILT
    assert h(MFMA, (17, 17, 17), 10, BS, IN, None, OUT) == ENOTBUILT
    assert h(MFMA4, (8, 8, 8), 10, BS, IN, None, OUT) == ENOTBUILT
    # 2D WAVE / MFMA / MFMA4 / WAVE_RT
    assert q(WAVE, (4, 9), 10, BS, IN + 8, None, OUT) == ENOTBUILT
    assert q(WAVE, (8, 8), 10, BS, IN + 8, None, OUT) == EALIGN
    assert q(WAVE, (25, 25), 10, BS, IN, None, OUT) == ENOTBUILT
    assert q(MFMA, (8, 8), 10, BS, IN, None, OUT) == ENOTBUILT
    assert q(MFMA4, (7, 7), 10, BS, IN, None, OUT) == ENOTBUILT
    assert q(WAVE_RT, (8, 8), 10, BS, IN, None, OUT) == ENOTBUILT
    assert q(WAVE_RT, (4, 9), 10, BS, IN, None, OUT) == ENOTBUILT


def test_bwdtrans_python_checks_sizes_without_gpu(pkg):
    """The wrappers refuse wrong sizes with ValueError before they touch the library: CPU tensors, nothing launched."""
    import torch
    f64 = torch.float64
    b = torch.zeros(56, dtype=f64)
    x3, o3 = torch.zeros(2 * 343, dtype=f64), torch.zeros(2 * 512, dtype=f64)
    x2, o2 = torch.zeros(2 * 49, dtype=f64), torch.zeros(2 * 64, dtype=f64)
    hx, qd, ip, sp = pkg.bwdtrans_hex, pkg.bwdtrans_quad, pkg.iproduct_hex, pkg.bwdtrans_specialised
    with pytest.raises(ValueError):      # inp not a whole number of elements
        hx((8, 8, 8), b, b, b, x3[:-1])
    with pytest.raises(ValueError):
        qd((8, 8), b, b, x2[:-1])
    with pytest.raises(ValueError):
        ip((8, 8, 8), b, b, b, o3[:-1])
    with pytest.raises(ValueError):
        sp((8, 8, 8), b, b, b, inp=x3[:-1])
    with pytest.raises(ValueError):      # out of the wrong size
        hx((8, 8, 8), b, b, b, x3, out=o3[:-1])
    with pytest.raises(ValueError):
        qd((8, 8), b, b, x2, out=torch.zeros(2 * 64 + 1, dtype=f64))
    with pytest.raises(ValueError):
        ip((8, 8, 8), b, b, b, o3, out=x3[:-1])
    with pytest.raises(ValueError):
        sp((8, 8, 8), b, b, b, inp=x3, out=o3[:-1])
    with pytest.raises(ValueError):      # a short basis
        hx((8, 8, 8), b, b[:55], b, x3)
    with pytest.raises(ValueError):
        qd((8, 8), b[:55], b, x2)
    with pytest.raises(ValueError):
        ip((8, 8, 8), b, b, b[:55], o3)
    with pytest.raises(ValueError):
        sp((8, 8, 8), b[:55], b, b, inp=x3)
    with pytest.raises(ValueError):      # a short workspace for block-glb
        hx((8, 8, 8), b, b, b, x3, variant="block-glb", wsp=torch.zeros(pkg.hex_wsp_doubles((8, 8, 8), 2) - 1, dtype=f64))
    with pytest.raises(ValueError):
        qd((8, 8), b, b, x2, variant="block-glb", wsp=torch.zeros(pkg.quad_wsp_doubles((8, 8), 2) - 1, dtype=f64))


def test_bwdtrans_binding_signatures(pkg):
    vp, sz, u, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_int
    want = {
        "sf_bwdtrans_hex_f64": (i, [u, u, u, sz, vp, vp, vp, vp, vp, vp]),
        "sf_bwdtrans_hex_f64_variant": (i, [i, u, u, u, sz, vp, vp, vp, vp, vp, vp, vp]),
        "sf_bwdtrans_quad_f64": (i, [u, u, sz, vp, vp, vp, vp, vp]),
        "sf_bwdtrans_quad_f64_variant": (i, [i, u, u, sz, vp, vp, vp, vp, vp, vp]),
        "sf_bwdtrans_hex_f32": (i, [u, u, u, sz, vp, vp, vp, vp, vp, vp]),
        "sf_bwdtrans_quad_f32": (i, [u, u, sz, vp, vp, vp, vp, vp]),
    }
    for name, sig in want.items():
        assert pkg.capi.SYMBOLS[name] == sig, name
