"""GPU tests of the run-time specialisation (include/sumfact.h sf_specialise): the wave-per-chunk kernels compiled with
hiprtc for shapes outside the compiled tables, against the CPU oracle -- through the specialised entry point and through
AUTO (which must actually route to them), plus the fallbacks, the spill guard, concurrency, stream capture and the
per-device state."""
import re
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12
TOL32 = 2e-5   # the suite's fp32 bar (tests/test_gpu_parity.py)
RAGGED = [1, 2, 3, 5, 13, 14, 15, 63, 64, 65, 127, 257, 1000, 4099]
SHAPES = [(6, 6, 12), (12, 10, 8), (5, 9, 7), (3, 5, 4), (2, 3, 2), (4, 9), (16, 3), (12, 20), (23, 5), (2, 24)]
# fp32 2x24: ROCm 7.0's compiler (the hiprtc a PyTorch process loads) gives it scratch, so the spill guard refuses it
F32_SHAPES = [s for s in SHAPES if s != (2, 24)]
CASES = [(s, "float64") for s in SHAPES] + [(s, "float32") for s in F32_SHAPES]


@pytest.fixture(scope="module")
def sf():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    return ge.load_package()


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(sf, nq, nelmt, dtype, seed, x=None):
    nm = [q - 1 for q in nq]
    bs = [sf.fill_random(nm[d] * nq[d], 400 + d + seed, dtype=dtype) for d in range(len(nq))]
    if x is None:
        x = sf.fill_random(nelmt * int(np.prod(nm)), seed, dtype=dtype)
    return bs, x


def _auto(sf, nq, bs, x, out=None, stream=None):
    if len(nq) == 3:
        return sf.bwdtrans_hex(nq, *bs, x, out=out, stream=stream)
    return sf.bwdtrans_quad(nq, *bs, x, out=out, stream=stream)


def _ref(oracle, nq, nelmt, bs, x):
    b = [_np(t).astype(np.float64) for t in bs]
    xs = _np(x).astype(np.float64)
    if len(nq) == 3:
        return oracle.bwdtrans_hex(tuple(nq), nelmt, *b, xs)
    return oracle.bwdtrans_quad(tuple(nq), nelmt, *b, xs)


def _log_compile(sf):
    m = re.search(r"compile #(\d+), ([\d.]+) s", sf.specialise_log())
    assert m, sf.specialise_log()
    return int(m.group(1)), float(m.group(2))


@pytest.mark.parametrize("nq,dtype_name", CASES, ids=["x".join(map(str, s)) + "-" + d for s, d in CASES])
def test_specialised_parity_direct_and_through_auto(sf, oracle, torch_mod, nq, dtype_name):
    dtype = getattr(torch_mod, dtype_name)
    tol = TOL if dtype == torch_mod.float64 else TOL32
    assert sf.specialisation_state(nq, dtype) == (0, 0)
    assert sf.specialise(nq, dtype) == sf.capi.SF_OK, sf.specialise_log()
    assert sf.specialisation_state(nq, dtype) == (1, 0)
    for nelmt in RAGGED:
        bs, x = _inputs(sf, nq, nelmt, dtype, nelmt)
        ref = _ref(oracle, nq, nelmt, bs, x)
        out = sf.bwdtrans_specialised(nq, *bs, inp=x)
        torch_mod.cuda.synchronize()
        assert oracle.rel_err(_np(out).astype(np.float64), ref) <= tol, ("specialised", nq, nelmt)
        _, before = sf.specialisation_state(nq, dtype)
        out = _auto(sf, nq, bs, x)
        torch_mod.cuda.synchronize()
        assert sf.specialisation_state(nq, dtype) == (1, before + 1), ("AUTO did not take the specialisation", nelmt)
        assert oracle.rel_err(_np(out).astype(np.float64), ref) <= tol, ("auto", nq, nelmt)
    assert sf.specialisation_state(nq, dtype) == (1, 2 * len(RAGGED))


def test_specialised_is_bit_identical_to_the_aot_instantiation(sf, torch_mod):
    """8x8x4 is a compile-time triple: hiprtc's code object of the same template must give the same bits as hipcc's."""
    nq = (8, 8, 4)
    assert sf.specialise(nq) == sf.capi.SF_OK, sf.specialise_log()
    for nelmt in (1, 3, 257, 4099, 100003):
        bs, x = _inputs(sf, nq, nelmt, torch_mod.float64, nelmt)
        wave = sf.bwdtrans_hex(nq, *bs, x, variant="wave")
        spec = sf.bwdtrans_specialised(nq, *bs, inp=x)
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(wave, spec), nelmt
    # AUTO keeps preferring the table for a shape it holds
    _, n = sf.specialisation_state(nq)
    sf.bwdtrans_hex(nq, *bs, x)
    torch_mod.cuda.synchronize()
    assert sf.specialisation_state(nq) == (1, n)


@pytest.mark.parametrize("nq", [(6, 6, 12), (4, 9)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_views_take_todays_route(sf, oracle, torch_mod, nq):
    """in / out only 8-byte (fp64) or 4-byte (fp32) aligned: AUTO leaves the specialisation alone; guard words stay."""
    for dtype, tol in ((torch_mod.float64, TOL), (torch_mod.float32, TOL32)):
        assert sf.specialise(nq, dtype) == sf.capi.SF_OK
        nmt, nqt = int(np.prod([q - 1 for q in nq])), int(np.prod(nq))
        nelmt = 333
        for off_in, off_out in ((1, 0), (0, 1), (1, 3)):
            xbuf = sf.fill_random(nelmt * nmt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nmt]
            bs, _ = _inputs(sf, nq, nelmt, dtype, 3, x=x)
            obuf = torch_mod.full((nelmt * nqt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nqt]
            state = sf.specialisation_state(nq, dtype)
            _auto(sf, nq, bs, x, out=o)
            torch_mod.cuda.synchronize()
            assert sf.specialisation_state(nq, dtype) == state, (off_in, off_out)
            assert oracle.rel_err(_np(o).astype(np.float64), _ref(oracle, nq, nelmt, bs, x)) <= tol
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nqt:] == 7.25).all())
            with pytest.raises(sf.capi.SumfactError) as ei:
                sf.bwdtrans_specialised(nq, *bs, inp=x, out=o)
            assert ei.value.rc == sf.capi.SF_EALIGN


def test_spilling_shape_is_refused_and_auto_stays_right(sf, oracle, torch_mod):
    nq = (16, 16, 14)
    assert sf.specialise(nq) == sf.capi.SF_ECOMPILE
    assert "spills" in sf.specialise_log()
    assert sf.specialisation_state(nq) == (sf.capi.SF_ECOMPILE, 0)
    assert sf.specialise(nq) == sf.capi.SF_ECOMPILE          # remembered: no second compile
    bs, x = _inputs(sf, nq, 37, torch_mod.float64, 7)
    out = sf.bwdtrans_hex(nq, *bs, x)
    torch_mod.cuda.synchronize()
    assert oracle.rel_err(_np(out), _ref(oracle, nq, 37, bs, x)) <= TOL
    with pytest.raises(sf.capi.SumfactError) as ei:
        sf.bwdtrans_specialised(nq, *bs, inp=x)
    assert ei.value.rc == sf.capi.SF_ENOTBUILT


def test_concurrent_requests_compile_once(sf, torch_mod):
    """Four threads ask for one new shape at once: all succeed, and they share one compile (same compile number)."""
    nq = (7, 5, 3)
    assert sf.specialisation_state(nq) == (0, 0)
    barrier = threading.Barrier(4)
    got = {}

    def worker(i):
        torch_mod.cuda.set_device(0)
        barrier.wait()
        rc = sf.specialise(nq)
        got[i] = (rc, _log_compile(sf))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert sorted(got) == [0, 1, 2, 3]
    assert all(rc == sf.capi.SF_OK for rc, _ in got.values()), got
    assert len({c for _, c in got.values()}) == 1, got     # one compile record: same number, same seconds
    serial = next(iter(got.values()))[1][0]
    assert sf.specialise((7, 5, 4)) == sf.capi.SF_OK
    assert _log_compile(sf)[0] == serial + 1                # the next new shape is the next compile


def test_auto_call_on_a_specialised_shape_is_captured(sf, oracle, torch_mod):
    nq, nelmt = (5, 9, 7), 20011
    assert sf.specialise(nq) == sf.capi.SF_OK
    bs, x = _inputs(sf, nq, nelmt, torch_mod.float64, 11)
    ref = _ref(oracle, nq, nelmt, bs, x)
    o = torch_mod.zeros(nelmt * int(np.prod(nq)), dtype=torch_mod.float64, device="cuda")
    torch_mod.cuda.synchronize()
    _, n0 = sf.specialisation_state(nq)
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            sf.bwdtrans_hex(nq, *bs, x, out=o, stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    assert sf.specialisation_state(nq) == (1, n0 + 1)       # the captured launch was the specialisation
    g.replay()
    torch_mod.cuda.synchronize()
    assert oracle.rel_err(_np(o), ref) <= TOL


def test_state_is_per_device(sf, oracle, torch_mod):
    if torch_mod.cuda.device_count() < 2:
        pytest.skip("one device visible")
    nq = (9, 4, 11)
    assert sf.specialise(nq, device=1) == sf.capi.SF_OK
    serial = _log_compile(sf)[0]
    assert sf.specialisation_state(nq, device=1) == (1, 0)
    assert sf.specialisation_state(nq, device=0) == (0, 0)
    assert sf.specialise(nq, device=0) == sf.capi.SF_OK
    assert _log_compile(sf)[0] == serial                    # loaded on device 0, compiled once
    dev = torch_mod.device("cuda:1")
    nm = [q - 1 for q in nq]
    bs = [sf.fill_random(nm[d] * nq[d], 70 + d, device=dev) for d in range(3)]
    x = sf.fill_random(101 * int(np.prod(nm)), 3, device=dev)
    out = sf.bwdtrans_hex(nq, *bs, x)
    torch_mod.cuda.synchronize(dev)
    assert sf.specialisation_state(nq, device=1) == (1, 1)
    assert sf.specialisation_state(nq, device=0) == (1, 0)
    assert oracle.rel_err(_np(out), _ref(oracle, nq, 101, bs, x)) <= TOL
