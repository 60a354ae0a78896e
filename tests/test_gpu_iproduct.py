"""GPU tests of IProductWRTBase (include/sumfact.h sf_iproduct_*), the transpose of BwdTrans: every wave order through
AUTO, ragged counts, the any-extent fallback, explicit variants, 8-byte-aligned views, guard values around `out`, the
full 1 048 576-element batch, stream capture, two streams in flight and the autograd binding.

Reference and bounds: tests/iprod_ref.py.  Elementwise |gpu - ref| <= gamma_n * absref against a long-double reference,
gamma_n = n u / (1 - n u), n = nq0 + nq1 (+ nq2), u = 2^-53 (fp64) or 2^-24 (fp32); where long double would be too
slow, 2 gamma_n (1 + gamma_n) * absref64 against fp64 CPU sweeps, and the adjointness bound with the GPU BwdTrans."""
import math

import numpy as np
import pytest

from iprod_ref import (U64, adjoint_bound, elementwise_excess, iprod_f64, ref_iprod,
                       unit_roundoff)

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 3, 5, 13, 14, 15, 63, 64, 65, 127, 257, 1000, 4099]   # tests/test_gpu_specialise.py
WAVE_ORDERS = [(3, n) for n in range(2, 12)] + [(2, n) for n in range(2, 17)]
FALLBACK = [(6, 6, 12), (3, 5, 4), (16, 12, 14), (2, 3, 2), (13, 13, 13), (4, 9), (16, 3), (32, 32), (23, 5)]


@pytest.fixture(scope="module")
def sf():
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available(), "the GPU tests need a GPU"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _bases(sf, torch_mod, nq, dtype_name, seed):
    dtype = getattr(torch_mod, dtype_name)
    return [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]


def _iprod(sf, nq, bs, x, **kw):
    return (sf.iproduct_hex if len(nq) == 3 else sf.iproduct_quad)(tuple(nq), *bs, x, **kw)


def _check(nq, nelmt, bs, x, got, dtype_name, what):
    ref, absref = ref_iprod(nq, nelmt, [_np(b) for b in bs], _np(x))
    q = elementwise_excess(_np(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"{what}: {nq} {dtype_name} nelmt={nelmt}: max |err| / (gamma_n absref) = {q:.3g}")
    assert q <= 1.0, (what, nq, dtype_name, nelmt, q)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("dim,nq", WAVE_ORDERS, ids=[f"{d}d-nq{n}" for d, n in WAVE_ORDERS])
def test_auto_every_wave_order(sf, torch_mod, dim, nq, dtype_name):
    ext = (nq,) * dim
    nelmt = 1003
    bs = _bases(sf, torch_mod, ext, dtype_name, nq)
    x = sf.fill_random(nelmt * nq ** dim, 10 + nq, dtype=getattr(torch_mod, dtype_name))
    got = _iprod(sf, ext, bs, x)
    torch_mod.cuda.synchronize()
    _check(ext, nelmt, bs, x, got, dtype_name, "auto")
    if dtype_name == "float64":
        # AUTO runs the wave kernel here: the same bits as the explicit variant
        wave = _iprod(sf, ext, bs, x, variant="wave")
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(got, wave)


RAGGED_SHAPES = [((2, 2, 2), "float64"), ((3, 3, 3), "float64"), ((8, 8, 8), "float64"), ((11, 11, 11), "float64"),
                 ((3, 3), "float64"), ((7, 7), "float64"), ((16, 16), "float64"),
                 ((3, 3, 3), "float32"), ((9, 9, 9), "float32"), ((7, 7), "float32"), ((13, 13), "float32")]


@pytest.mark.parametrize("nq,dtype_name", RAGGED_SHAPES, ids=[_ids(s) + "-" + d for s, d in RAGGED_SHAPES])
def test_ragged_counts(sf, torch_mod, nq, dtype_name):
    bs = _bases(sf, torch_mod, nq, dtype_name, 3)
    for nelmt in RAGGED:
        x = sf.fill_random(nelmt * int(np.prod(nq)), nelmt, dtype=getattr(torch_mod, dtype_name))
        got = _iprod(sf, nq, bs, x)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, x, got, dtype_name, "ragged")


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("nq", FALLBACK, ids=_ids)
def test_fallback_shapes(sf, torch_mod, nq, dtype_name):
    for nelmt in (1, 37, 300):
        bs = _bases(sf, torch_mod, nq, dtype_name, nelmt)
        x = sf.fill_random(nelmt * int(np.prod(nq)), 70 + nelmt, dtype=getattr(torch_mod, dtype_name))
        got = _iprod(sf, nq, bs, x)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, x, got, dtype_name, "fallback")
        if dtype_name == "float64":
            gen = _iprod(sf, nq, bs, x, variant="generic")
            torch_mod.cuda.synchronize()
            assert torch_mod.equal(got, gen)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (9, 9)], ids=_ids)
def test_explicit_wave_and_generic(sf, torch_mod, nq):
    nelmt = 777
    bs = _bases(sf, torch_mod, nq, "float64", 9)
    x = sf.fill_random(nelmt * int(np.prod(nq)), 99)
    for variant in ("wave", "generic"):
        got = _iprod(sf, nq, bs, x, variant=variant)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, x, got, "float64", variant)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=_ids)
def test_eight_byte_aligned_views_take_the_fallback(sf, torch_mod, nq):
    nelmt = 333
    nqt, nmt = int(np.prod(nq)), int(np.prod([q - 1 for q in nq]))
    for dtype_name, offsets in (("float64", ((1, 0), (0, 1), (1, 3))), ("float32", ((2, 0), (0, 2), (1, 3)))):
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 4)
        for off_in, off_out in offsets:
            xbuf = sf.fill_random(nelmt * nqt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nqt]
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            _iprod(sf, nq, bs, x, out=o)
            torch_mod.cuda.synchronize()
            _check(nq, nelmt, bs, x, o, dtype_name, f"view {off_in}/{off_out}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                with pytest.raises(sf.capi.SumfactError) as ei:
                    _iprod(sf, nq, bs, x, out=o, variant="wave")
                assert ei.value.rc == sf.capi.SF_EALIGN


GUARD = [((3, 3, 3), 1001), ((7, 7, 7), 257), ((8, 8, 8), 65), ((9, 9, 9), 63), ((11, 11, 11), 15), ((5, 5), 4099),
         ((13, 13), 1000), ((16, 16), 127), ((6, 6, 12), 13), ((23, 5), 14)]


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=[_ids(s) for s, _ in GUARD])
def test_guard_values_around_out(sf, torch_mod, nq, nelmt):
    """`out` sits between two guard bands (16-byte aligned, so the wave kernels run): only its own values change."""
    nqt, nmt = int(np.prod(nq)), int(np.prod([q - 1 for q in nq]))
    for dtype_name, pad in (("float64", 64), ("float32", 128)):
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 5)
        x = sf.fill_random(nelmt * nqt, 5, dtype=dtype)
        obuf = torch_mod.full((nelmt * nmt + 2 * pad,), -3.5, dtype=dtype, device="cuda")
        o = obuf[pad:pad + nelmt * nmt]
        _iprod(sf, nq, bs, x, out=o)
        torch_mod.cuda.synchronize()
        assert bool((obuf[:pad] == -3.5).all()) and bool((obuf[pad + nelmt * nmt:] == -3.5).all()), dtype_name
        _check(nq, nelmt, bs, x, o, dtype_name, "guard")


def test_full_batch_hex8(sf, torch_mod):
    """1 048 576 elements at 3D nq = 8: elementwise against fp64 CPU sweeps (bound 2 gamma_n (1 + gamma_n) absref64),
    then adjointness with the GPU BwdTrans."""
    nq, nelmt = (8, 8, 8), 1 << 20
    nqt, nmt = 512, 343
    bs = _bases(sf, torch_mod, nq, "float64", 8)
    bh = [_np(b) for b in bs]
    v = sf.fill_random(nelmt * nqt, 1234)
    w = sf.iproduct_hex(nq, *bs, v)
    torch_mod.cuda.synchronize()
    step, worst = 1 << 15, 0.0
    for lo in range(0, nelmt, step):
        vv = _np(v[lo * nqt:(lo + step) * nqt])
        out64, abs64 = iprod_f64(nq, step, bh, vv)
        g = sum(nq) * U64 / (1 - sum(nq) * U64)
        worst = max(worst, elementwise_excess(_np(w[lo * nmt:(lo + step) * nmt]), out64, abs64, nq, U64,
                                              factor=2 * (1 + g)))
    print(f"full batch: max |err| / (2 gamma_n (1 + gamma_n) absref64) = {worst:.3g}")
    assert worst <= 1.0
    del v
    # adjointness: sum_e <B x, y>_e against sum_e <x, I y>_e
    x = sf.fill_random(nelmt * nmt, 4321)
    y = sf.fill_random(nelmt * nqt, 8765)
    bx = sf.bwdtrans_hex(nq, *bs, x)
    iy = sf.iproduct_hex(nq, *bs, y)
    babs = sf.bwdtrans_hex(nq, *[b.abs() for b in bs], x.abs())
    torch_mod.cuda.synchronize()

    def dots(a, b):
        return (a.view(nelmt, -1) * b.view(nelmt, -1)).sum(dim=1).cpu().numpy()

    lhs = math.fsum(dots(bx, y))
    rhs = math.fsum(dots(x, iy))
    scale = math.fsum(dots(babs, y.abs()))
    bound = adjoint_bound(nq, U64) * scale
    print(f"adjointness: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("nq,nelmt", [((8, 8, 8), 20011), ((9, 9), 5003), ((6, 6, 12), 1001)], ids=lambda v: _ids(v))
def test_captured_graph_replay_matches_eager(sf, torch_mod, nq, nelmt):
    bs = _bases(sf, torch_mod, nq, "float64", 11)
    x = sf.fill_random(nelmt * int(np.prod(nq)), 11)
    nmt = int(np.prod([q - 1 for q in nq]))
    eager = _iprod(sf, nq, bs, x)
    o = torch_mod.zeros(nelmt * nmt, dtype=torch_mod.float64, device="cuda")
    torch_mod.cuda.synchronize()
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            _iprod(sf, nq, bs, x, out=o, stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    g.replay()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(o, eager)
    _check(nq, nelmt, bs, x, o, "float64", "graph")


FIRST_CALL_CAPTURED = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
sf = ge.load_package()
for nq, nelmt in (((8, 8, 8), 5001), ((6, 6, 12), 301), ((9, 9), 2001)):
    f = sf.iproduct_hex if len(nq) == 3 else sf.iproduct_quad
    nm = [q - 1 for q in nq]
    bs = [sf.fill_random(nm[d] * nq[d], 40 + d) for d in range(len(nq))]
    npt, nmo = 1, 1
    for q in nq:
        npt, nmo = npt * q, nmo * (q - 1)
    x = sf.fill_random(nelmt * npt, 41)
    o = torch.zeros(nelmt * nmo, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            f(nq, *bs, x, out=o, stream=side)     # the process's first call of this shape
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    eager = f(nq, *bs, x)
    torch.cuda.synchronize()
    assert torch.equal(o, eager), nq
print("first calls captured")
"""


def test_first_call_inside_a_capture():
    """Capture-safe from the first call: a fresh process whose first IProductWRTBase call of each route (wave, fallback)
    is inside a stream capture; the replay equals an eager call made afterwards."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", FIRST_CALL_CAPTURED, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_two_streams_in_flight(sf, torch_mod):
    """Two problems enqueued on two streams before either is waited for; each against fp64 CPU sweeps."""
    jobs = [((7, 7, 7), 100003), ((12, 12), 200009)]
    streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
    data = []
    for (nq, nelmt), st in zip(jobs, streams):
        bs = _bases(sf, torch_mod, nq, "float64", nelmt % 97)
        x = sf.fill_random(nelmt * int(np.prod(nq)), nelmt)
        data.append((bs, x))
    torch_mod.cuda.synchronize()
    outs = []
    for (nq, _), st, (bs, x) in zip(jobs, streams, data):
        with torch_mod.cuda.stream(st):
            outs.append(_iprod(sf, nq, bs, x, stream=st))
    torch_mod.cuda.synchronize()
    for (nq, nelmt), (bs, x), o in zip(jobs, data, outs):
        out64, abs64 = iprod_f64(nq, nelmt, [_np(b) for b in bs], _np(x))
        g = sum(nq) * U64 / (1 - sum(nq) * U64)
        q = elementwise_excess(_np(o), out64, abs64, nq, U64, factor=2 * (1 + g))
        print(f"stream job {nq}: {q:.3g}")
        assert q <= 1.0, nq


@pytest.mark.parametrize("nq,nelmt", [((4, 4, 4), 3), ((5, 5), 4)], ids=lambda v: _ids(v))
def test_bwdtrans_autograd_gradcheck(sf, torch_mod, nq, nelmt):
    bs = _bases(sf, torch_mod, nq, "float64", 2)
    nmt = int(np.prod([q - 1 for q in nq]))
    x = sf.fill_random(nelmt * nmt, 17).requires_grad_(True)
    assert torch_mod.autograd.gradcheck(lambda t: sf.bwdtrans_autograd(nq, bs, t), (x,))
    # the backward pass is IProductWRTBase of the output gradient
    y = sf.bwdtrans_autograd(nq, bs, x)
    gy = sf.fill_random(y.numel(), 18)
    (gx,) = torch_mod.autograd.grad(y, x, gy)
    assert torch_mod.equal(gx, _iprod(sf, nq, bs, gy))
    with pytest.raises(ValueError):
        sf.bwdtrans_autograd(nq, [bs[0].clone().requires_grad_(True)] + bs[1:], x)

