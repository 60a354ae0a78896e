"""GPU tests of the tensor-product apply with independent input / output extents (include/sumfact.h sf_tensor_*): every
entry of the compiled table inside the derived bound of tests/tensor_ref.py on ragged counts, through AUTO, the explicit
wave variant and the any-extent kernel (all three bit for bit the same); equality by value with sf_bwdtrans_* and
sf_iproduct_* on their shapes; shapes only the fallback or a run-time specialisation can run; guard words, NaN bands and
every scalar offset inside a 128-byte line; the specialisation's state, routing, refusals and concurrency; stream capture
as a process's first call, two streams in flight, batches over several XCD windows and the autograd wrapper.

Data is drawn in float32 and widened, so that one long-double reference per (shape, trans) serves both scalar types; the
ragged counts are prefixes of one batch of 4099 elements."""
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

from fused_common import Banded
from fused_families import sf, torch_mod  # noqa: F401  (fixtures)
from tensor_ref import ref_tensor, tensor_excess, unit_roundoff

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 3, 5, 13, 63, 64, 65, 127, 128, 129, 257, 1000, 4099]
DTYPES = ["float64", "float32"]


def _up(n):
    return -(-3 * n // 2)


HEX_PAIRS = [(n, n) for n in range(2, 9)] + [(n, _up(n)) for n in range(2, 7)] + [(_up(n), n) for n in range(2, 7)]
QUAD_PAIRS = [(n, n) for n in range(2, 17)] + [(n, _up(n)) for n in range(2, 11)] + [(_up(n), n) for n in range(2, 11)]
TABLE = [(3, i, o) for i, o in HEX_PAIRS] + [(2, i, o) for i, o in QUAD_PAIRS]


def tensor_cfg(dim, ni, no, sbytes):
    """(ec, wpb) of csrc/rtc_config.h tensor_cfg, restated."""
    vw = 16 // sbytes
    i2, o2 = (ni[2], no[2]) if dim == 3 else (1, 1)
    big = max(int(np.prod(ni[:dim])), int(np.prod(no[:dim])))
    if dim == 3:
        ec = min(max(512 // big, 1), 8)
    else:
        ec = min(max(256 // big, -(-48 // max(ni[1], no[0])), 1), 16)
    ec *= 2 if sbytes == 4 else 1
    p0, p1, p2 = ec * i2 * ni[1], ec * no[0] * i2, ec * no[1] * no[0]
    slab0 = max(p0 * (ni[0] | 1), p1 * (ni[1] | 1), p2 * (i2 | 1) if dim == 3 else 0)
    slab = (max(slab0, ec * no[0] * no[1] * o2) + vw - 1) // vw * vw
    wpb = 4
    while wpb > 1 and sbytes * wpb * slab > 64 * 1024:
        wpb //= 2
    return ec, wpb


class Case:
    """One shape and `trans` with data for `nelmt` elements, its long-double reference, and the device copies per dtype."""

    def __init__(self, torch, ni, no, trans, nelmt, seed, reference=True):
        self.torch, self.ni, self.no, self.trans, self.nelmt = torch, tuple(ni), tuple(no), int(trans), nelmt
        self.nin, self.nout = int(np.prod(ni)), int(np.prod(no))
        rng = np.random.default_rng(seed)
        f32 = lambda n: rng.uniform(-1, 1, n).astype(np.float32).astype(np.float64)  # noqa: E731
        self.mats = [f32(a * b) for a, b in zip(ni, no)]
        self.x = f32(nelmt * self.nin)
        if reference:
            self.ref, self.absref = ref_tensor(ni, no, trans, nelmt, self.mats, self.x)
        self.dev = {}

    def on(self, dtype_name):
        if dtype_name not in self.dev:
            dt = getattr(self.torch, dtype_name)
            put = lambda a: self.torch.from_numpy(a).to(device="cuda", dtype=dt)  # noqa: E731
            self.dev[dtype_name] = ([put(m) for m in self.mats], put(self.x))
        return self.dev[dtype_name]

    def run(self, sf, dtype_name, n=None, variant="auto", out=None, stream=None, x=None, mats=None):
        m, xd = self.on(dtype_name)
        n = self.nelmt if n is None else n
        x = xd[:n * self.nin] if x is None else x
        fn = sf.tensor_hex if len(self.ni) == 3 else sf.tensor_quad
        return fn(self.ni, self.no, *(mats or m), x, trans=self.trans, out=out, variant=variant, stream=stream)

    def excess(self, got, dtype_name, n=None):
        n = self.nelmt if n is None else n
        k = n * self.nout
        assert got.numel() == k
        return tensor_excess(got.detach().cpu().numpy(), self.ref[:k], self.absref[:k], self.ni, unit_roundoff(dtype_name))


def _label(ni, no, trans=0):
    return "x".join(f"{a}>{b}" for a, b in zip(ni, no)) + (":t" if trans else "")


# ---- the compiled table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,i,o", TABLE, ids=[f"{d}d-{i}>{o}" for d, i, o in TABLE])
def test_table_entry_bounds_and_routes(sf, torch_mod, dim, i, o):
    """Every output of AUTO within gamma_N absref on ragged counts that straddle a workgroup's EC * WPB elements; AUTO,
    SF_VARIANT_WAVE and the any-extent kernel give the same bits."""
    ni, no = (i,) * dim, (o,) * dim
    for dtype_name in DTYPES:
        ec, wpb = tensor_cfg(dim, ni, no, 8 if dtype_name == "float64" else 4)
        per = ec * wpb
        assert min(RAGGED) < per < max(RAGGED) and any(per < n and n % per for n in RAGGED), (ni, no, dtype_name, per)
        assert any(n % ec for n in RAGGED) or ec == 1
    worst = 0.0
    for trans in (0, 1):
        c = Case(torch_mod, ni, no, trans, max(RAGGED), 100 * i + o + trans)
        for dtype_name in DTYPES:
            for n in RAGGED:
                auto = c.run(sf, dtype_name, n)
                wave = c.run(sf, dtype_name, n, variant="wave")
                generic = c.run(sf, dtype_name, n, variant="generic")
                torch_mod.cuda.synchronize()
                ex = c.excess(auto, dtype_name, n)
                worst = max(worst, ex)
                assert ex <= 1.0, (_label(ni, no, trans), dtype_name, n, ex)
                assert torch_mod.equal(auto, wave), (_label(ni, no, trans), dtype_name, n)
                assert torch_mod.equal(wave, generic), (_label(ni, no, trans), dtype_name, n)
    print(f"{dim}D {i}>{o}: worst |err| / (gamma_N absref) = {worst:.3f}")


# ---- equality with the existing kernels ----------------------------------------------------------------------------------
def _same_values(torch, a, b):
    return a.shape == b.shape and bool((a == b).all())        # by value: +0 == -0


@pytest.mark.parametrize("dim,nq", [(3, 4), (3, 8), (2, 8), (2, 16)], ids=lambda v: str(v))
def test_equals_bwdtrans_and_iproduct(sf, torch_mod, dim, nq):
    """(nq-1 -> nq)^d with trans = 0 is sf_bwdtrans_*, (nq -> nq-1)^d with trans = 1 is sf_iproduct_*: the same values,
    through a specialised tensor kernel (AUTO, counted) and through the fallback."""
    nm_, nq_ = (nq - 1,) * dim, (nq,) * dim
    bwd = sf.bwdtrans_hex if dim == 3 else sf.bwdtrans_quad
    ipr = sf.iproduct_hex if dim == 3 else sf.iproduct_quad
    for ni, no, trans, old in ((nm_, nq_, 0, bwd), (nq_, nm_, 1, ipr)):
        assert sf.specialise_tensor(ni, no, trans) == sf.capi.SF_OK, sf.specialise_log()
        for nelmt in (1, 5, 129, 1000):
            c = Case(torch_mod, ni, no, trans, nelmt, nq + nelmt, reference=False)
            # the basis array is the same for both: row-major nm x nq
            m, x = c.on("float64")
            want = old(nq_, *m, x)
            _, before = sf.tensor_specialisation_state(ni, no, trans)
            spec = c.run(sf, "float64")
            generic = c.run(sf, "float64", variant="generic")
            torch_mod.cuda.synchronize()
            assert sf.tensor_specialisation_state(ni, no, trans) == (1, before + 1), "AUTO did not take the specialisation"
            diff = float((spec - want).abs().max())
            print(f"{dim}D nq {nq} {_label(ni, no, trans)} n={nelmt}: max |tensor - existing| = {diff:.3e}")
            assert _same_values(torch_mod, spec, want), (_label(ni, no, trans), nelmt, "specialised", diff)
            assert _same_values(torch_mod, generic, want), (_label(ni, no, trans), nelmt, "generic")


# ---- shapes only the fallback or a specialisation can run ------------------------------------------------------------------
OFF_TABLE = [((3, 4, 6), (5, 4, 2)), ((1, 2, 5), (4, 2, 1)), ((16, 2, 1), (16, 3, 1)), ((1, 9), (4, 3)), ((32, 7), (20, 32))]


@pytest.mark.parametrize("ni,no", OFF_TABLE, ids=[_label(a, b) for a, b in OFF_TABLE])
def test_shapes_off_the_table(sf, torch_mod, ni, no):
    dim = len(ni)
    can_specialise = max(ni + no) <= (16 if dim == 3 else 24)
    counts = [1, 5, 65, 259]
    for trans in (0, 1):
        c = Case(torch_mod, ni, no, trans, max(counts), 31 + trans)
        for dtype_name in DTYPES:
            dt = getattr(torch_mod, dtype_name)
            with pytest.raises(sf.capi.SumfactError) as ei:
                c.run(sf, dtype_name, 5, variant="wave")
            assert ei.value.rc == sf.capi.SF_ENOTBUILT
            fall = {}
            for n in counts:
                fall[n] = c.run(sf, dtype_name, n, variant="generic")
                torch_mod.cuda.synchronize()
                ex = c.excess(fall[n], dtype_name, n)
                print(f"{_label(ni, no, trans)} {dtype_name} n={n}: fallback {ex:.3f}")
                assert ex <= 1.0, (_label(ni, no, trans), dtype_name, n, ex)
            if can_specialise:
                assert sf.specialise_tensor(ni, no, trans, dt) == sf.capi.SF_OK, sf.specialise_log()
                for n in counts:
                    _, before = sf.tensor_specialisation_state(ni, no, trans, dt)
                    got = c.run(sf, dtype_name, n)
                    torch_mod.cuda.synchronize()
                    assert sf.tensor_specialisation_state(ni, no, trans, dt) == (1, before + 1)
                    assert c.excess(got, dtype_name, n) <= 1.0, (_label(ni, no, trans), dtype_name, n)
                    assert torch_mod.equal(got, fall[n]), (_label(ni, no, trans), dtype_name, n)
            else:
                with pytest.raises(sf.capi.SumfactError) as ei:
                    sf.specialise_tensor(ni, no, trans, dt)
                assert ei.value.rc == sf.capi.SF_EINVAL


def test_beyond_the_fallback_is_not_built(sf, torch_mod):
    m = torch_mod.zeros(17 * 4, dtype=torch_mod.float64, device="cuda")
    x = torch_mod.zeros(17 * 16, dtype=torch_mod.float64, device="cuda")
    for variant in ("auto", "generic", "wave"):
        with pytest.raises(sf.capi.SumfactError) as ei:
            sf.tensor_hex((17, 4, 4), (4, 4, 4), m, m[:16], m[:16], x, variant=variant)
        assert ei.value.rc == sf.capi.SF_ENOTBUILT


# ---- guard words, NaN bands, offsets ---------------------------------------------------------------------------------------
GUARD = [((4, 4, 4), (6, 6, 6), 0), ((5, 5), (8, 8), 1), ((9, 9, 9), (6, 6, 6), 1), ((3, 4, 6), (5, 4, 2), 0)]


@pytest.mark.parametrize("ni,no,trans", GUARD, ids=[_label(a, b, t) for a, b, t in GUARD])
def test_guard_words_and_nan_bands(sf, torch_mod, ni, no, trans):
    """`out` between guard words, `in` and every matrix between NaN bands: nothing outside `out` is written, nothing from
    outside an input reaches a result.  Then one element of `in` poisoned with NaN: only its own outputs change."""
    for dtype_name in DTYPES:
        for nelmt in (1, 7, 131):
            c = Case(torch_mod, ni, no, trans, nelmt, 17)
            m, x = c.on(dtype_name)
            xin = Banded.of(torch_mod, x)
            mats = [Banded.of(torch_mod, t) for t in m]
            out = Banded.of(torch_mod, torch_mod.zeros(nelmt * c.nout, dtype=x.dtype, device="cuda"), -3.5)
            for variant in ("auto", "generic"):
                out.reset()
                c.run(sf, dtype_name, variant=variant, out=out.view, x=xin.view, mats=[b.view for b in mats])
                torch_mod.cuda.synchronize()
                what = (_label(ni, no, trans), dtype_name, nelmt, variant)
                assert out.bands_intact(torch_mod), ("written outside out",) + what
                assert xin.bands_intact(torch_mod) and all(b.bands_intact(torch_mod) for b in mats), what
                assert bool(torch_mod.isfinite(out.view).all()), ("not finite",) + what
                assert c.excess(out.view, dtype_name) <= 1.0, what
            clean = out.view.clone()
            e = nelmt // 2
            xin.view[e * c.nin:(e + 1) * c.nin] = float("nan")
            for variant in ("auto", "generic"):
                out.reset()
                c.run(sf, dtype_name, variant=variant, out=out.view, x=xin.view, mats=[b.view for b in mats])
                torch_mod.cuda.synchronize()
                got = out.view.reshape(nelmt, c.nout)
                assert bool(torch_mod.isnan(got[e]).all()), (variant, "the poisoned element")
                keep = [k for k in range(nelmt) if k != e]
                assert torch_mod.equal(got[keep], clean.reshape(nelmt, c.nout)[keep]), (variant, "a NaN left its element")


@pytest.mark.parametrize("ni,no,trans", GUARD[:2], ids=[_label(a, b, t) for a, b, t in GUARD[:2]])
def test_every_scalar_offset_inside_a_line(sf, torch_mod, ni, no, trans):
    """`in` / `out` at every scalar offset of a 128-byte line: 16-byte-aligned pairs run the wave kernel, the others the
    any-extent kernel (SF_VARIANT_WAVE refuses them); the same bits either way, the guard words untouched."""
    nelmt = 37
    for dtype_name in DTYPES:
        c = Case(torch_mod, ni, no, trans, nelmt, 23, reference=False)
        m, x = c.on(dtype_name)
        want = c.run(sf, dtype_name, variant="generic")
        torch_mod.cuda.synchronize()
        line, vw = 128 // x.element_size(), 16 // x.element_size()
        for off in range(line):
            for off_in, off_out in ((off, 0), (0, off), (off, (off + vw + 1) % line)):
                xin = Banded(torch_mod, x.dtype, x.numel(), off_in, float("nan"))
                xin.view.copy_(x)
                out = Banded(torch_mod, x.dtype, nelmt * c.nout, off_out, -3.5)
                c.run(sf, dtype_name, out=out.view, x=xin.view)
                torch_mod.cuda.synchronize()
                assert out.bands_intact(torch_mod) and xin.bands_intact(torch_mod), (dtype_name, off_in, off_out)
                assert torch_mod.equal(out.view, want), (dtype_name, off_in, off_out)
                if off_in % vw or off_out % vw:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        c.run(sf, dtype_name, out=out.view, x=xin.view, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN


def test_overlap_is_refused(sf, torch_mod):
    c = Case(torch_mod, (4, 4), (6, 6), 0, 10, 3, reference=False)
    m, x = c.on("float64")
    buf = torch_mod.zeros(10 * 36 + 10 * 16, dtype=torch_mod.float64, device="cuda")
    with pytest.raises(sf.capi.SumfactError) as ei:
        sf.tensor_quad((4, 4), (6, 6), *m, buf[:160], out=buf[152:152 + 360])
    assert ei.value.rc == sf.capi.SF_EINVAL


# ---- run-time specialisation ------------------------------------------------------------------------------------------------
SPEC = [((4, 4, 4), (7, 7, 7), 0), ((7, 7, 7), (4, 4, 4), 1), ((5, 3, 6), (8, 3, 4), 0), ((10, 6), (15, 9), 0)]


def _compile_serial(sf):
    m = re.search(r"compile #(\d+), ([\d.]+) s", sf.specialise_log())
    assert m, sf.specialise_log()
    return int(m.group(1))


@pytest.mark.parametrize("ni,no,trans", SPEC, ids=[_label(a, b, t) for a, b, t in SPEC])
def test_specialisation_state_routing_and_parity(sf, torch_mod, ni, no, trans):
    for dtype_name in DTYPES:
        dt = getattr(torch_mod, dtype_name)
        c = Case(torch_mod, ni, no, trans, max(RAGGED), 41)
        before = c.run(sf, dtype_name, 13)                                   # no module yet: the fallback
        assert sf.tensor_specialisation_state(ni, no, trans, dt) == (0, 0)
        assert sf.specialise_tensor(ni, no, trans, dt) == sf.capi.SF_OK, sf.specialise_log()
        assert "tensor_wave_kernel<" in sf.specialise_log()
        print(sf.specialise_log().splitlines()[0])
        assert sf.tensor_specialisation_state(ni, no, trans, dt) == (1, 0)
        assert sf.tensor_specialisation_state(ni, no, 1 - trans, dt) == (0, 0)  # a key of its own
        for k, n in enumerate(RAGGED):
            got = c.run(sf, dtype_name, n)
            generic = c.run(sf, dtype_name, n, variant="generic")
            torch_mod.cuda.synchronize()
            assert sf.tensor_specialisation_state(ni, no, trans, dt) == (1, k + 1), ("AUTO did not take the module", n)
            assert c.excess(got, dtype_name, n) <= 1.0, (dtype_name, n)
            assert torch_mod.equal(got, generic), (dtype_name, n)
        assert torch_mod.equal(before, c.run(sf, dtype_name, 13, variant="generic"))
        # buffers aligned only to the scalar leave the module alone
        x = c.on(dtype_name)[1]
        xb = Banded(torch_mod, x.dtype, 5 * c.nin, 1, float("nan"))
        xb.view.copy_(x[:5 * c.nin])
        state = sf.tensor_specialisation_state(ni, no, trans, dt)
        got = c.run(sf, dtype_name, 5, x=xb.view)
        torch_mod.cuda.synchronize()
        assert sf.tensor_specialisation_state(ni, no, trans, dt) == state
        assert c.excess(got, dtype_name, 5) <= 1.0


def test_refused_shape_falls_back_and_stays_correct(sf, torch_mod):
    """1 -> 16, 16 -> 1, 16 -> 1: the first intermediate of one wave's chunk exceeds the slab limit."""
    ni, no = (1, 16, 16), (16, 1, 1)
    assert sf.specialise_tensor(ni, no) == sf.capi.SF_ECOMPILE
    assert "exceeds 64 KiB" in sf.specialise_log()
    assert sf.tensor_specialisation_state(ni, no) == (sf.capi.SF_ECOMPILE, 0)
    assert sf.specialise_tensor(ni, no) == sf.capi.SF_ECOMPILE             # remembered
    c = Case(torch_mod, ni, no, 0, 37, 7)
    got = c.run(sf, "float64")
    torch_mod.cuda.synchronize()
    assert c.excess(got, "float64") <= 1.0
    assert sf.tensor_specialisation_state(ni, no) == (sf.capi.SF_ECOMPILE, 0)


def test_request_inside_a_capture_is_refused_without_compiling(sf, torch_mod):
    ni, no = (3, 6, 5), (4, 4, 7)
    assert sf.specialise_tensor((2, 6, 5), (4, 4, 7)) == sf.capi.SF_OK
    serial = _compile_serial(sf)
    c = Case(torch_mod, ni, no, 0, 9, 5)
    m, x = c.on("float64")
    out = torch_mod.zeros(9 * c.nout, dtype=torch_mod.float64, device="cuda")
    torch_mod.cuda.synchronize()
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            rc = sf.specialise_tensor(ni, no)
            c.run(sf, "float64", out=out, stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    assert rc == sf.capi.SF_ECOMPILE
    assert sf.tensor_specialisation_state(ni, no) == (0, 0)                 # nothing recorded, nothing compiled
    g.replay()
    torch_mod.cuda.synchronize()
    assert c.excess(out, "float64") <= 1.0
    assert sf.specialise_tensor(ni, no) == sf.capi.SF_OK                    # outside the capture it compiles
    assert _compile_serial(sf) == serial + 1


def test_two_threads_request_one_shape(sf, torch_mod):
    ni, no = (6, 2, 3), (3, 5, 4)
    assert sf.tensor_specialisation_state(ni, no, True) == (0, 0)
    barrier, got = threading.Barrier(2), {}

    def worker(k):
        torch_mod.cuda.set_device(0)
        barrier.wait()
        got[k] = (sf.specialise_tensor(ni, no, True), _compile_serial(sf))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert sorted(got) == [0, 1] and all(rc == sf.capi.SF_OK for rc, _ in got.values()), got
    assert got[0][1] == got[1][1], got                                        # one compile
    assert sf.tensor_specialisation_state(ni, no, True) == (1, 0)


# ---- streams, capture, long batches, autograd -------------------------------------------------------------------------------
def test_first_call_inside_a_capture():
    """A fresh child process whose first call into the library is an AUTO sf_tensor_* call inside a stream capture."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tensor_first_call.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_two_streams_in_flight(sf, torch_mod):
    streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
    cases = [Case(torch_mod, (4, 4, 4), (6, 6, 6), 0, 3001, 1), Case(torch_mod, (12, 12), (8, 8), 1, 4003, 2)]
    for c in cases:
        c.on("float64")
    torch_mod.cuda.synchronize()
    outs = []
    for _ in range(3):
        outs = [c.run(sf, "float64", stream=s) for c, s in zip(cases, streams)]
    for s in streams:
        s.synchronize()
    for c, o in zip(cases, outs):
        assert c.excess(o, "float64") <= 1.0


@pytest.mark.parametrize("ni,no,nelmt", [((4, 4, 4), (6, 6, 6), 20011), ((8, 8), (12, 12), 40009)],
                         ids=["3d-4>6", "2d-8>12"])
def test_batch_over_several_xcd_windows(sf, torch_mod, ni, no, nelmt):
    """More than three windows of 8 * 64 workgroups and a partial tail window: the wave kernel equals the any-extent
    kernel on every element, and a long-double reference on the first, the last and a middle stretch."""
    for dtype_name in DTYPES:
        ec, wpb = tensor_cfg(len(ni), ni + (1,), no + (1,), 8 if dtype_name == "float64" else 4)
        blocks = -(-nelmt // (ec * wpb))
        assert blocks > 2 * 512 and blocks % 512, (dtype_name, blocks)
        c = Case(torch_mod, ni, no, 0, nelmt, 77, reference=False)
        wave = c.run(sf, dtype_name, variant="wave")
        generic = c.run(sf, dtype_name, variant="generic")
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(wave, generic), dtype_name
        for first in (0, nelmt // 2 - 50, nelmt - 100):
            x = c.x[first * c.nin:(first + 100) * c.nin]
            ref, absref = ref_tensor(ni, no, 0, 100, c.mats, x)
            got = wave[first * c.nout:(first + 100) * c.nout].cpu().numpy()
            assert tensor_excess(got, ref, absref, ni, unit_roundoff(dtype_name)) <= 1.0, (dtype_name, first)


@pytest.mark.parametrize("ni,no,trans", [((4, 4, 4), (6, 6, 6), 0), ((9, 5), (3, 7), 1)], ids=["3d", "2d"])
def test_autograd_is_the_transposed_call(sf, torch_mod, ni, no, trans):
    c = Case(torch_mod, ni, no, trans, 33, 3, reference=False)
    m, x = c.on("float64")
    xg = x.clone().requires_grad_(True)
    y = sf.tensor_autograd(ni, no, m, xg, trans=bool(trans))
    assert torch_mod.equal(y.detach(), c.run(sf, "float64"))
    g = torch_mod.from_numpy(np.random.default_rng(4).uniform(-1, 1, y.numel())).cuda()
    y.backward(g)
    fn = sf.tensor_hex if len(ni) == 3 else sf.tensor_quad
    want = fn(no, ni, *m, g, trans=not trans)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(xg.grad, want) and float(want.abs().max()) > 0
