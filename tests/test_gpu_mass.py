"""GPU tests of the fused mass operator (include/sumfact.h sf_mass_*), y_e = B^T diag(w_e) B x_e in one kernel: every
wave order through AUTO, ragged counts, the any-extent fallback, 8-byte-aligned views, guard values around `out` with
`w` between NaN bands, composition with the two existing operators, symmetry and positivity, the full 1 048 576-element
batch, stream capture and two streams in flight.

Reference and bounds: tests/mass_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double reference,
gamma_N = N u / (1 - N u), N = 2 (nq0 + nq1 [+ nq2]) + 1, u = 2^-53 (fp64) or 2^-24 (fp32); where long double would be
too slow, 2 gamma_N (1 + gamma_N) * absref64 against fp64 CPU sweeps.

That lanes without a point of the batch issue no weight load at all is a property of the code (load_weights() in
csrc/mass_wave.h: the loads sit inside `t < NP && e < evalid`) and of the ISA (the loads are under an exec mask); no test
can show it without provoking a fault, and none tries.
"""
import math

import numpy as np
import pytest

from mass_ref import U64, gamma, mass_excess, mass_f64, mass_n, ref_mass, symmetry_bound, unit_roundoff
from test_gpu_iproduct import FALLBACK, GUARD, RAGGED

pytestmark = pytest.mark.gpu

WAVE_ORDERS = [(3, n) for n in range(2, 12)] + [(2, n) for n in range(2, 17)]


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


def _sizes(nq):
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def _bases(sf, torch_mod, nq, dtype_name, seed):
    dtype = getattr(torch_mod, dtype_name)
    return [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]


def _weights(sf, torch_mod, n, seed, dtype_name):
    return 0.25 + sf.fill_random(n, 7000 + seed, dtype=getattr(torch_mod, dtype_name)).abs()


def _mass(sf, nq, bs, w, x, **kw):
    return (sf.mass_hex if len(nq) == 3 else sf.mass_quad)(tuple(nq), *bs, w, x, **kw)


def _check(nq, nelmt, bs, w, x, got, dtype_name, what):
    ref, absref = ref_mass(nq, nelmt, [_np(b) for b in bs], _np(w), _np(x))
    q = mass_excess(_np(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"{what}: {nq} {dtype_name} nelmt={nelmt}: max |err| / (gamma_N absref) = {q:.3g}")
    assert q <= 1.0, (what, nq, dtype_name, nelmt, q)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("dim,nq", WAVE_ORDERS, ids=[f"{d}d-nq{n}" for d, n in WAVE_ORDERS])
def test_auto_every_wave_order(sf, torch_mod, dim, nq, dtype_name):
    ext = (nq,) * dim
    nelmt = 1003
    nmt, nqt = _sizes(ext)
    bs = _bases(sf, torch_mod, ext, dtype_name, nq)
    x = sf.fill_random(nelmt * nmt, 10 + nq, dtype=getattr(torch_mod, dtype_name))
    w = _weights(sf, torch_mod, nelmt * nqt, nq, dtype_name)
    got = _mass(sf, ext, bs, w, x)
    torch_mod.cuda.synchronize()
    _check(ext, nelmt, bs, w, x, got, dtype_name, "auto")
    if dtype_name == "float64":
        # AUTO runs the wave kernel here: the same bits as the explicit variant
        wave = _mass(sf, ext, bs, w, x, variant="wave")
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(got, wave)


# EC > 1 rows (3D nq 2..6, every 2D row), EC = 1 rows (3D nq 7..11), word-grid input rows (one element with an odd number
# of modes: 3D nq 8 / 10 in fp64) and fp32
RAGGED_SHAPES = [((2, 2, 2), "float64"), ((3, 3, 3), "float64"), ((4, 4, 4), "float64"), ((6, 6, 6), "float64"),
                 ((7, 7, 7), "float64"), ((8, 8, 8), "float64"), ((10, 10, 10), "float64"), ((11, 11, 11), "float64"),
                 ((3, 3), "float64"), ((7, 7), "float64"), ((8, 8), "float64"), ((12, 12), "float64"),
                 ((16, 16), "float64"),
                 ((3, 3, 3), "float32"), ((8, 8, 8), "float32"), ((9, 9, 9), "float32"), ((7, 7), "float32"),
                 ((13, 13), "float32")]


@pytest.mark.parametrize("nq,dtype_name", RAGGED_SHAPES, ids=[_ids(s) + "-" + d for s, d in RAGGED_SHAPES])
def test_ragged_counts(sf, torch_mod, nq, dtype_name):
    """The last chunk is ragged and `w` ends where the batch ends: the guarded weight loads."""
    nmt, nqt = _sizes(nq)
    bs = _bases(sf, torch_mod, nq, dtype_name, 3)
    for nelmt in RAGGED:
        x = sf.fill_random(nelmt * nmt, nelmt, dtype=getattr(torch_mod, dtype_name))
        w = _weights(sf, torch_mod, nelmt * nqt, nelmt, dtype_name)
        got = _mass(sf, nq, bs, w, x)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, w, x, got, dtype_name, "ragged")


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("nq", FALLBACK, ids=_ids)
def test_fallback_shapes(sf, torch_mod, nq, dtype_name):
    nmt, nqt = _sizes(nq)
    for nelmt in (1, 37, 300):
        bs = _bases(sf, torch_mod, nq, dtype_name, nelmt)
        x = sf.fill_random(nelmt * nmt, 70 + nelmt, dtype=getattr(torch_mod, dtype_name))
        w = _weights(sf, torch_mod, nelmt * nqt, 70 + nelmt, dtype_name)
        got = _mass(sf, nq, bs, w, x)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, w, x, got, dtype_name, "fallback")
        if dtype_name == "float64":
            gen = _mass(sf, nq, bs, w, x, variant="generic")
            torch_mod.cuda.synchronize()
            assert torch_mod.equal(got, gen)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (9, 9)], ids=_ids)
def test_explicit_wave_and_generic(sf, torch_mod, nq):
    nelmt = 777
    nmt, nqt = _sizes(nq)
    bs = _bases(sf, torch_mod, nq, "float64", 9)
    x = sf.fill_random(nelmt * nmt, 99)
    w = _weights(sf, torch_mod, nelmt * nqt, 99, "float64")
    for variant in ("wave", "generic"):
        got = _mass(sf, nq, bs, w, x, variant=variant)
        torch_mod.cuda.synchronize()
        _check(nq, nelmt, bs, w, x, got, "float64", variant)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=_ids)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """8-byte-aligned (fp32: 4-byte-aligned) views of in, out and w.  AUTO is correct through the fallback when in or out
    lacks 16-byte alignment, and through the wave kernel when only w does; guards on both sides of out are untouched;
    variant "wave" refuses in / out with SF_EALIGN."""
    nelmt = 333
    nmt, nqt = _sizes(nq)
    cases = (("float64", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 1))), ("float32", ((2, 0, 0), (0, 2, 0), (0, 0, 1), (1, 3, 3))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 4)
        for off_in, off_out, off_w in offsets:
            xbuf = sf.fill_random(nelmt * nmt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nmt]
            wbuf = _weights(sf, torch_mod, nelmt * nqt + 8, off_w, dtype_name)
            w = wbuf[off_w:off_w + nelmt * nqt]
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            _mass(sf, nq, bs, w, x, out=o)
            torch_mod.cuda.synchronize()
            _check(nq, nelmt, bs, w, x, o, dtype_name, f"view {off_in}/{off_out}/{off_w}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                if off_in or off_out:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        _mass(sf, nq, bs, w, x, out=o, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                else:
                    # w needs only scalar alignment on the wave route
                    wave = _mass(sf, nq, bs, w, x, variant="wave")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(wave, o)


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=[_ids(s) for s, _ in GUARD])
def test_guard_values_around_out_and_nan_around_w(sf, torch_mod, nq, nelmt):
    """`out` sits between two guard bands (16-byte aligned, so the wave kernels run): only its own values change.  `w` is
    a view inside a larger buffer filled with NaN on both sides: a weight read from outside the batch that reached a
    result would show as a NaN in `out`."""
    nmt, nqt = _sizes(nq)
    for dtype_name, pad in (("float64", 64), ("float32", 128)):
        dtype = getattr(torch_mod, dtype_name)
        bs = _bases(sf, torch_mod, nq, dtype_name, 5)
        x = sf.fill_random(nelmt * nmt, 5, dtype=dtype)
        wbuf = torch_mod.full((nelmt * nqt + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        wbuf[pad:pad + nelmt * nqt] = _weights(sf, torch_mod, nelmt * nqt, 5, dtype_name)
        w = wbuf[pad:pad + nelmt * nqt]
        obuf = torch_mod.full((nelmt * nmt + 2 * pad,), -3.5, dtype=dtype, device="cuda")
        o = obuf[pad:pad + nelmt * nmt]
        _mass(sf, nq, bs, w, x, out=o)
        torch_mod.cuda.synchronize()
        assert bool((obuf[:pad] == -3.5).all()) and bool((obuf[pad + nelmt * nmt:] == -3.5).all()), dtype_name
        assert not bool(torch_mod.isnan(o).any()), dtype_name
        _check(nq, nelmt, bs, w, x, o, dtype_name, "guard")


COMPOSE = [((8, 8, 8), 1003, "float64"), ((5, 5, 5), 1003, "float64"), ((11, 11, 11), 257, "float64"),
           ((12, 12), 1003, "float64"), ((7, 7), 1003, "float64"), ((6, 6, 12), 300, "float64"), ((23, 5), 300, "float64"),
           ((8, 8, 8), 1003, "float32"), ((16, 16), 1003, "float32")]


@pytest.mark.parametrize("nq,nelmt,dtype_name", COMPOSE, ids=[_ids(s) + "-" + d for s, _, d in COMPOSE])
def test_composition_with_bwdtrans_and_iproduct(sf, torch_mod, nq, nelmt, dtype_name):
    """The fused result against the three-launch chain iproduct(w * bwdtrans(x)) on the GPU, within
    2 gamma_N (1 + gamma_N) * absref, absref from the fused operator on absolute values.  The two orders of summation
    differ, so bit identity is not expected."""
    nmt, nqt = _sizes(nq)
    bs = _bases(sf, torch_mod, nq, dtype_name, 6)
    x = sf.fill_random(nelmt * nmt, 61, dtype=getattr(torch_mod, dtype_name))
    w = _weights(sf, torch_mod, nelmt * nqt, 62, dtype_name)
    bwd, ipr = (sf.bwdtrans_hex, sf.iproduct_hex) if len(nq) == 3 else (sf.bwdtrans_quad, sf.iproduct_quad)
    fused = _mass(sf, nq, bs, w, x)
    chain = ipr(tuple(nq), *bs, w * bwd(tuple(nq), *bs, x))
    absref = _mass(sf, nq, [b.abs() for b in bs], w, x.abs())
    torch_mod.cuda.synchronize()
    u = unit_roundoff(dtype_name)
    g = gamma(mass_n(nq), u)
    q = mass_excess(_np(fused), _np(chain), _np(absref), nq, u, factor=2 * (1 + g))
    print(f"composition {nq} {dtype_name}: max |fused - chain| / (2 gamma_N (1 + gamma_N) absref) = {q:.3g}")
    assert q <= 1.0
    assert float(absref.min()) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12)], ids=_ids)
def test_symmetry_and_positivity(sf, torch_mod, nq):
    """|<M x, y> - <x, M y>| <= 2 (gamma_N + gamma_m) sum_e <|M||x|, |y|>_e, m = nm^d, |M| the fused operator on absolute
    values, the sums with math.fsum per element; and <M x, x> > 0 for w > 0."""
    nelmt = 1003
    nmt, nqt = _sizes(nq)
    bs = _bases(sf, torch_mod, nq, "float64", 12)
    x = sf.fill_random(nelmt * nmt, 121)
    y = sf.fill_random(nelmt * nmt, 122)
    w = _weights(sf, torch_mod, nelmt * nqt, 123, "float64")
    mx = _mass(sf, nq, bs, w, x)
    my = _mass(sf, nq, bs, w, y)
    mabs = _mass(sf, nq, [b.abs() for b in bs], w, x.abs())
    torch_mod.cuda.synchronize()

    def dots(a, b):
        a, b = _np(a).reshape(nelmt, -1), _np(b).reshape(nelmt, -1)
        return [math.fsum(a[e] * b[e]) for e in range(nelmt)]

    lhs, rhs = math.fsum(dots(mx, y)), math.fsum(dots(x, my))
    scale = math.fsum(dots(mabs, y.abs()))
    bound = symmetry_bound(nq, U64) * scale
    print(f"symmetry {nq}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound
    energy = dots(mx, x)
    assert min(energy) > 0 and math.fsum(energy) > 0


def test_full_batch_hex8(sf, torch_mod):
    """1 048 576 elements at 3D nq = 8: elementwise against fp64 CPU sweeps in slices (bound 2 gamma_N (1 + gamma_N)
    absref64); a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 1 << 20
    nmt, nqt = 343, 512
    bs = _bases(sf, torch_mod, nq, "float64", 8)
    bh = [_np(b) for b in bs]
    x = sf.fill_random(nelmt * nmt, 1234)
    w = _weights(sf, torch_mod, nelmt * nqt, 1235, "float64")
    y = sf.mass_hex(nq, *bs, w, x)
    torch_mod.cuda.synchronize()
    g = gamma(mass_n(nq), U64)
    step, worst = 1 << 15, 0.0
    for lo in range(0, nelmt, step):
        out64, abs64 = mass_f64(nq, step, bh, _np(w[lo * nqt:(lo + step) * nqt]), _np(x[lo * nmt:(lo + step) * nmt]))
        worst = max(worst, mass_excess(_np(y[lo * nmt:(lo + step) * nmt]), out64, abs64, nq, U64, factor=2 * (1 + g)))
    print(f"full batch: max |err| / (2 gamma_N (1 + gamma_N) absref64) = {worst:.3g}")
    assert worst <= 1.0
    again = sf.mass_hex(nq, *bs, w, x)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


@pytest.mark.parametrize("nq,nelmt", [((8, 8, 8), 20011), ((9, 9), 5003), ((6, 6, 12), 1001)], ids=lambda v: _ids(v))
def test_captured_graph_replay_matches_eager(sf, torch_mod, nq, nelmt):
    nmt, nqt = _sizes(nq)
    bs = _bases(sf, torch_mod, nq, "float64", 11)
    x = sf.fill_random(nelmt * nmt, 11)
    w = _weights(sf, torch_mod, nelmt * nqt, 11, "float64")
    eager = _mass(sf, nq, bs, w, x)
    o = torch_mod.zeros(nelmt * nmt, dtype=torch_mod.float64, device="cuda")
    torch_mod.cuda.synchronize()
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            _mass(sf, nq, bs, w, x, out=o, stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    g.replay()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(o, eager)
    _check(nq, nelmt, bs, w, x, o, "float64", "graph")


FIRST_CALL_CAPTURED = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
sf = ge.load_package()
for nq, nelmt in (((8, 8, 8), 5001), ((6, 6, 12), 301), ((9, 9), 2001), ((23, 5), 301)):
    f = sf.mass_hex if len(nq) == 3 else sf.mass_quad
    nm = [q - 1 for q in nq]
    bs = [sf.fill_random(nm[d] * nq[d], 40 + d) for d in range(len(nq))]
    npt, nmo = 1, 1
    for q in nq:
        npt, nmo = npt * q, nmo * (q - 1)
    x = sf.fill_random(nelmt * nmo, 41)
    w = 0.25 + sf.fill_random(nelmt * npt, 42).abs()
    o = torch.zeros(nelmt * nmo, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            f(nq, *bs, w, x, out=o, stream=side)     # the process's first call of this route
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    eager = f(nq, *bs, w, x)
    torch.cuda.synchronize()
    assert torch.equal(o, eager), nq
    assert float(o.abs().max()) > 0, nq
print("first calls captured")
"""


def test_first_call_inside_a_capture():
    """Capture-safe from the first call: a fresh child process whose first fused call of each route (3D wave, 3D
    fallback, 2D wave, 2D fallback) is inside a stream capture; the replay equals an eager call made afterwards."""
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
    for nq, nelmt in jobs:
        nmt, nqt = _sizes(nq)
        bs = _bases(sf, torch_mod, nq, "float64", nelmt % 97)
        x = sf.fill_random(nelmt * nmt, nelmt)
        w = _weights(sf, torch_mod, nelmt * nqt, nelmt % 89, "float64")
        data.append((bs, w, x))
    torch_mod.cuda.synchronize()
    outs = []
    for (nq, _), st, (bs, w, x) in zip(jobs, streams, data):
        with torch_mod.cuda.stream(st):
            outs.append(_mass(sf, nq, bs, w, x, stream=st))
    torch_mod.cuda.synchronize()
    for (nq, nelmt), (bs, w, x), o in zip(jobs, data, outs):
        out64, abs64 = mass_f64(nq, nelmt, [_np(b) for b in bs], _np(w), _np(x))
        g = gamma(mass_n(nq), U64)
        q = mass_excess(_np(o), out64, abs64, nq, U64, factor=2 * (1 + g))
        print(f"stream job {nq}: {q:.3g}")
        assert q <= 1.0, nq


def test_overlap_is_refused(sf, torch_mod):
    """out == in and out inside w: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    bs = _bases(sf, torch_mod, nq, "float64", 1)
    x = sf.fill_random(nelmt * 343, 1)
    w = _weights(sf, torch_mod, nelmt * 512, 1, "float64")
    keep = x.clone()
    for o in (x, w[:nelmt * 343]):
        with pytest.raises(sf.capi.SumfactError) as ei:
            sf.mass_hex(nq, *bs, w, x, out=o)
        assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(x, keep)
