"""GPU tests of the diagonal of the fused Helmholtz operator (include/sumfact.h sf_diag_helmholtz_*, sf_diag_tables_*)
that are the family's own: scalar-aligned views of out, g, w and the tables, the Laplacian that never reads `w`, the
operator itself as the witness (sf_helmholtz_* applied to every unit vector), the Gauss-Lobatto closed form, the tables
alone, several XCD windows, `g` past 2^32 scalars, four host threads on one stream and refused overlaps.  install() adds
the family's cases of the parametrised tests the fused families share (tests/fused_common.py: every wave order through
AUTO, ragged counts, the fallback, explicit variants, guard bands); refusals, stream capture and two streams in flight
are tests/test_gpu_fused_common.py.

Reference and bound: tests/diag_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double reference,
gamma_N = N u / (1 - N u), N = 3 sum nq_d + d + 2 + (6 | 3), u = 2^-53 (fp64) or 2^-24 (fp32); where long double would be
too slow, (gamma_N(u) + gamma_N(2^-53)) (1 + gamma_N(2^-53)) * absref64 against the fp64 numpy form (each side within its
gamma_N of the truth; for an fp64 result that is the 2 gamma_N (1 + gamma_N) of the other families).
Data: sf.fill_random, seeded, per-value distinct; g uniform in (-1, 1) and so not definite.
"""
import ctypes
import gc
import threading

import numpy as np
import pytest

from diag_ref import diag_excess, diag_f64, diag_n, gll_exact_diag, ref_diag, tables, tables_excess
from fused_common import install
from fused_families import BY_NAME, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from helm_ref import COMPONENTS, U64, gamma, gll_setup, helm_n, ref_helmholtz, unit_roundoff

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["diag"])

LAM = 0.75


def _ncomp(nq):
    return len(COMPONENTS[len(nq)])


class Problem:
    """Seeded data of one case, on the device; the tables are built once, by the library."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.nq, self.nelmt, self.dtype_name = tuple(nq), nelmt, dtype_name
        _, nqt = sizes(nq)
        self.bs = [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ds = [sf.fill_random(q * q, 600 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.g = sf.fill_random(nelmt * _ncomp(nq) * nqt, 8000 + seed, dtype=dtype)
        self.w = sf.fill_random(nelmt * nqt, 7000 + seed, dtype=dtype)
        self.tabs = [sf.diag_tables(q, b, d) for q, b, d in zip(nq, self.bs, self.ds)]
        self.host = ([to_host(b) for b in self.bs], [to_host(d) for d in self.ds])

    def run(self, sf, lam=LAM, **kw):
        g = kw.pop("g", self.g)
        w = kw.pop("w", self.w)
        tabs = kw.pop("tabs", self.tabs)
        f = sf.diag_helmholtz_hex if len(self.nq) == 3 else sf.diag_helmholtz_quad
        return f(self.nq, *self.bs, *self.ds, g, w, lam, tabs=tabs, **kw)

    def excess(self, got, lam=LAM, g=None, w="self"):
        g = self.g if g is None else g
        w = self.w if isinstance(w, str) else w
        nelmt = g.numel() // (_ncomp(self.nq) * sizes(self.nq)[1])
        ref, absref = ref_diag(self.nq, nelmt, *self.host, to_host(g), to_host(w), lam)
        assert float(np.max(np.abs(ref))) > 0
        return diag_excess(to_host(got), ref, absref, self.nq, unit_roundoff(self.dtype_name))

    def check(self, got, what, lam=LAM, g=None, w="self"):
        q = self.excess(got, lam, g, w)
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt} lam={lam}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, self.nelmt, q)


def f64_excess(p, got, lam=LAM, lo=0, n=None):
    """max |got - fp64 numpy| / ((gamma_N(u) + gamma_N(u64)) (1 + gamma_N(u64)) absref64) over elements lo .. lo + n."""
    n = p.nelmt if n is None else n
    nmt, nqt = sizes(p.nq)
    nc = _ncomp(p.nq)
    g = to_host(p.g[lo * nc * nqt:(lo + n) * nc * nqt]).astype(np.float64)
    w = to_host(p.w[lo * nqt:(lo + n) * nqt]).astype(np.float64) if lam != 0 else None
    out64, abs64 = diag_f64(p.nq, n, [b.astype(np.float64) for b in p.host[0]], [d.astype(np.float64) for d in p.host[1]],
                            g, w, lam)
    gu, g64 = gamma(diag_n(p.nq), unit_roundoff(p.dtype_name)), gamma(diag_n(p.nq), U64)
    return diag_excess(to_host(got[lo * nmt:(lo + n) * nmt]), out64, abs64, p.nq, unit_roundoff(p.dtype_name),
                       factor=(gu + g64) * (1 + g64) / gu)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """Scalar-aligned views of out, g, w and the tables.  AUTO is correct through the fallback when out lacks 16-byte
    alignment (guards on both sides of out untouched, variant "wave" refuses with SF_EALIGN), and stays on the wave
    kernel, bit for bit, when only g / w / the tables do."""
    nelmt = 133
    nmt, nqt = sizes(nq)
    nc = _ncomp(nq)
    cases = (("float64", ((1, 0, 0, 0), (0, 1, 1, 1), (3, 1, 3, 1))), ("float32", ((2, 0, 0, 0), (0, 1, 3, 1), (1, 3, 1, 3))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 4)
        aligned = p.run(sf)
        torch_mod.cuda.synchronize()
        for off_out, off_g, off_w, off_t in offsets:
            gbuf = torch_mod.zeros(nelmt * nc * nqt + 8, dtype=dtype, device="cuda")
            g = gbuf[off_g:off_g + nelmt * nc * nqt]
            g.copy_(p.g)
            wbuf = torch_mod.zeros(nelmt * nqt + 8, dtype=dtype, device="cuda")
            w = wbuf[off_w:off_w + nelmt * nqt]
            w.copy_(p.w)
            tabs = []
            for t in p.tabs:
                tbuf = torch_mod.zeros(t.numel() + 8, dtype=dtype, device="cuda")
                tabs.append(tbuf[off_t:off_t + t.numel()])
                tabs[-1].copy_(t)
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            p.run(sf, g=g, w=w, tabs=tabs, out=o)
            torch_mod.cuda.synchronize()
            p.check(o, f"view {off_out}/{off_g}/{off_w}/{off_t}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                if off_out:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        p.run(sf, g=g, w=w, tabs=tabs, out=o, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                    gen = p.run(sf, g=g, w=w, tabs=tabs, variant="generic")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(gen, o)      # AUTO took the fallback
                else:
                    wave = p.run(sf, g=g, w=w, tabs=tabs, variant="wave")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(wave, o)     # g, w and the tables need only scalar alignment on the wave route
            if not off_out:
                assert torch_mod.equal(o, aligned)      # the same kernel, the same bits, wherever the inputs sit


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (3, 3), (6, 6, 12), (23, 5)], ids=case_id)
def test_laplacian_never_reads_w(sf, torch_mod, nq):
    """lambda == 0 with w=None equals lambda == 0 with a NaN-filled w, bit for bit, in both precisions."""
    for dtype_name in ("float64", "float32"):
        p = Problem(sf, torch_mod, nq, 301, dtype_name, 21)
        none = p.run(sf, lam=0.0, w=None)
        nan = p.run(sf, lam=0.0, w=torch_mod.full_like(p.w, float("nan")))
        torch_mod.cuda.synchronize()
        assert not bool(torch_mod.isnan(none).any())
        assert torch_mod.equal(none, nan), (nq, dtype_name)
        p.check(none, "laplacian", lam=0.0, w=None)


@pytest.mark.parametrize("nq,nelmt", [((4, 4, 4), 67), ((6, 6), 131)], ids=lambda v: case_id(v))
def test_the_operator_itself_is_the_witness(sf, torch_mod, nq, nelmt):
    """sf_helmholtz_* applied to the unit vector e_m in every element, entry m collected: the diagonal, within the sum of
    the two families' bounds (each result is within its own gamma_N absref of the same exact number)."""
    nmt, _ = sizes(nq)
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 3)
    helm = sf.helmholtz_hex if len(nq) == 3 else sf.helmholtz_quad
    for lam, w in ((LAM, p.w), (0.0, None)):
        diag = p.run(sf, lam=lam, w=w)
        torch_mod.cuda.synchronize()
        col = torch_mod.empty_like(diag).view(nelmt, nmt)
        habs = np.empty((nelmt, nmt), dtype=np.longdouble)
        for m in range(nmt):
            x = torch_mod.zeros(nelmt, nmt, dtype=torch_mod.float64, device="cuda")
            x[:, m] = 1.0
            y = helm(nq, *p.bs, *p.ds, p.g, w, lam, x.reshape(-1))
            col[:, m] = y.view(nelmt, nmt)[:, m]
            _, ha = ref_helmholtz(nq, nelmt, *p.host, to_host(p.g), to_host(w), lam, to_host(x.reshape(-1)))
            habs[:, m] = np.asarray(ha).reshape(nelmt, nmt)[:, m]
        torch_mod.cuda.synchronize()
        _, dabs = ref_diag(nq, nelmt, *p.host, to_host(p.g), to_host(w), lam)
        bound = gamma(diag_n(nq), U64) * np.asarray(dabs).reshape(-1) + gamma(helm_n(nq), U64) * habs.reshape(-1)
        err = np.abs(to_host(diag).astype(np.longdouble) - to_host(col.reshape(-1)).astype(np.longdouble))
        worst = float(np.max(err / bound))
        print(f"witness {nq} lam={lam}: max |diag - (A e_m)_m| / (sum of the bounds) = {worst:.3g}")
        assert worst <= 1.0 and float(diag.abs().max()) > 0
        p.check(diag, "witness", lam=lam, w=w)


@pytest.mark.parametrize("dim,nq", [(3, 8), (2, 12)], ids=["3d-nq8", "2d-nq12"])
def test_gll_closed_form(sf, torch_mod, dim, nq):
    """Legendre modes at the Gauss-Lobatto points, G = I * weight, w = weight, on the device: within the bound around
    ref_diag of the same data, which is the closed form lam prod m[p_d] + sum_a s[p_a] prod_{d != a} m[p_d] to 1e-12 of its
    largest entry."""
    nelmt, ext = 67, (nq,) * dim
    bases, derivs, g, w = gll_setup(nq, dim, nelmt)
    dev = lambda a: torch_mod.tensor(np.asarray(a), device="cuda")      # noqa: E731
    tb, td, tg, tw = [dev(b) for b in bases], [dev(d) for d in derivs], dev(g), dev(w)
    f = sf.diag_helmholtz_hex if dim == 3 else sf.diag_helmholtz_quad
    for lam, ww, hw in ((LAM, tw, w), (0.0, None, None)):
        got = f(ext, *tb, *td, tg, ww, lam)                              # tabs=None: the tables are built on the way
        torch_mod.cuda.synchronize()
        ref, absref = ref_diag(ext, nelmt, bases, derivs, g, hw, lam)
        q = diag_excess(to_host(got), ref, absref, ext, U64)
        exact = np.tile(gll_exact_diag(nq, dim, lam), nelmt)
        scale = float(np.max(np.abs(exact)))
        e_ref = float(np.max(np.abs(np.asarray(ref, dtype=np.float64) - exact))) / scale
        slack = gamma(diag_n(ext), U64) * np.asarray(absref, dtype=np.float64) + 1e-12 * scale
        print(f"gll {ext} lam={lam}: excess {q:.3g}; reference against the closed form {e_ref:.3g} of max |exact| = {scale:.4g}")
        assert q <= 1.0 and e_ref <= 1e-12
        assert bool(np.all(np.abs(to_host(got) - exact) <= slack))


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_diag_tables(sf, torch_mod, dtype_name):
    """sf_diag_tables_* against long-double tables of the same (rounded) inputs: within gamma_{2 nq + 1} of the tables of
    absolute values."""
    dtype = getattr(torch_mod, dtype_name)
    for nq in (2, 3, 5, 8, 12, 16, 17, 32, 100):
        b = sf.fill_random((nq - 1) * nq, 900 + nq, dtype=dtype)
        d = sf.fill_random(nq * nq, 950 + nq, dtype=dtype)
        tab = sf.diag_tables(nq, b, d)
        torch_mod.cuda.synchronize()
        assert tab.numel() == 3 * (nq - 1) * nq
        q = tables_excess(to_host(tab), tables(nq, to_host(b), to_host(d)), tables(nq, to_host(b), to_host(d), absolute=True), nq,
                          unit_roundoff(dtype_name))
        print(f"tables nq {nq} {dtype_name}: max |err| / (gamma_{2 * nq + 1} abstab) = {q:.3g}")
        assert q <= 1.0 and float(tab.abs().max()) > 0


# (extents, {dtype: (EC, WPB)}): the rows of csrc/helmholtz_launch.h that the kernels run on
WINDOWS = [((8, 8, 8), {"float64": (1, 8), "float32": (2, 8)}), ((16, 16), {"float64": (4, 4), "float32": (4, 4)})]


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("nq,rows", WINDOWS, ids=[case_id(s) for s, _ in WINDOWS])
def test_several_xcd_windows(sf, torch_mod, nq, rows, dtype_name):
    """Workgroups are renumbered in windows of 8 * 64 = 512: four full windows' worth of elements plus 3, so that the grid
    ends in a partial window and a ragged chunk.  The whole output against the fp64 numpy form, in slices."""
    ec, wpb = rows[dtype_name]
    nelmt = 4 * 512 * wpb * ec + 3
    p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 17)
    got = p.run(sf)
    torch_mod.cuda.synchronize()
    assert bool(torch_mod.isfinite(got).all())
    step = 4096
    worst = max(f64_excess(p, got, lo=lo, n=min(step, nelmt - lo)) for lo in range(0, nelmt, step))
    print(f"windows {nq} {dtype_name} nelmt={nelmt}: max |err| / bound against fp64 numpy = {worst:.3g}")
    assert worst <= 1.0
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(got, again)


def test_streams_past_2_to_the_32_scalars(sf, torch_mod):
    """fp32 3D nq 8 with g just past 2^32 scalars (the index arithmetic is in scalars): windows of 300 elements against
    the long-double reference at the head, across the elements that hold scalar 2^31 and 2^32 of g, and at the tail."""
    nq, win = (8, 8, 8), 300
    nmt, nqt = sizes(nq)
    per_g = 6 * nqt
    nelmt = (1 << 32) // per_g + 1 + 333
    nelmt += 1 - nelmt % 2                                    # odd: a ragged last chunk (EC = 2) in a partial workgroup
    assert nelmt * per_g > 1 << 32
    need = 4 * nelmt * (per_g + nqt + nmt) + (2 << 30)
    free, _ = torch_mod.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"not enough device memory: {need >> 30} GiB")
    held = []
    try:
        p = Problem(sf, torch_mod, nq, nelmt, "float32", 8)
        out = torch_mod.full((nelmt * nmt,), float("nan"), dtype=torch_mod.float32, device="cuda")
        held += [p.g, p.w, out]
        assert p.g.numel() > 1 << 32
        p.run(sf, out=out)
        torch_mod.cuda.synchronize()
        assert all(bool(torch_mod.isfinite(out[a:a + (1 << 28)]).all()) for a in range(0, out.numel(), 1 << 28))
        e31, e32 = (1 << 31) // per_g, (1 << 32) // per_g
        worst = 0.0
        for lo in (0, e31 - win // 2, e32 - win // 2, nelmt - win):
            assert 0 <= lo and lo + win <= nelmt
            ref, absref = ref_diag(nq, win, *p.host, to_host(p.g[lo * per_g:(lo + win) * per_g]),
                                   to_host(p.w[lo * nqt:(lo + win) * nqt]), LAM)
            q = diag_excess(to_host(out[lo * nmt:(lo + win) * nmt]), ref, absref, nq, unit_roundoff("float32"))
            print(f"past 2^32: elements {lo} .. {lo + win}: max |err| / (gamma_N absref) = {q:.3g}")
            worst = max(worst, q)
        assert worst <= 1.0
    finally:
        for t in held:
            t.untyped_storage().resize_(0)
        gc.collect()
        torch_mod.cuda.empty_cache()


def test_four_host_threads_on_one_stream(sf, torch_mod):
    """Four threads call the raw C entry points on ONE stream, arguments marshalled beforehand (the calls release the GIL,
    so the threads are inside the library together), each thread its own problem (3D wave, 3D fallback, 2D wave, 2D
    fallback) and one output per launch: every output equals the thread's serial result, bit for bit."""
    torch = torch_mod
    shapes = [((8, 8, 8), 1501), ((6, 6, 12), 151), ((12, 12), 4001), ((23, 5), 301)]
    launches, timeout = 12, 120
    st = torch.cuda.Stream()
    lib = sf.capi.lib()
    probs = [Problem(sf, torch, nq, nelmt, "float64", 60 + i) for i, (nq, nelmt) in enumerate(shapes)]
    torch.cuda.synchronize()
    want = [p.run(sf, stream=st) for p in probs]
    st.synchronize()
    for p, o in zip(probs, want):
        p.check(o, "serial")
    handle = ctypes.c_void_p(st.cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    outs, calls = [], []
    for p in probs:
        n = p.nelmt * sizes(p.nq)[0]
        stride = (n + 31) // 32 * 32                     # rows start 256-byte aligned, as fresh allocations would
        o = torch.full((launches, stride), float("nan"), dtype=torch.float64, device="cuda")
        outs.append(o[:, :n])
        fn = lib.sf_diag_helmholtz_hex_f64_variant if len(p.nq) == 3 else lib.sf_diag_helmholtz_quad_f64_variant
        calls.append([(fn, (0, *p.nq, p.nelmt, *[ptr(t) for t in p.tabs], ptr(p.g), ptr(p.w), ctypes.c_double(LAM),
                            ptr(o[k]), handle)) for k in range(launches)])
    torch.cuda.synchronize()
    barrier = threading.Barrier(len(probs))
    errors = [None] * len(probs)

    def body(i):
        try:
            barrier.wait(timeout=timeout)
            for fn, args in calls[i]:
                sf.capi.check(fn(*args), "sf_diag_helmholtz")
        except BaseException as e:      # noqa: B036 -- handed to the main thread below
            errors[i] = e

    threads = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(probs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not [i for i, t in enumerate(threads) if t.is_alive()]
    for e in errors:
        if e is not None:
            raise e
    torch.cuda.synchronize()
    for p, o, w in zip(probs, outs, want):
        assert torch.equal(o, w[None, :].expand(launches, w.numel())), p.nq


def test_overlap_is_refused(sf, torch_mod):
    """out inside g, out inside w, out == a table: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    keep = p.g.clone()
    for o in (p.g[512:512 + nelmt * 343], p.w[:nelmt * 343]):
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, out=o)
        assert ei.value.rc == sf.capi.SF_EINVAL
    # a table triple (3 * 2 * 3 scalars at nq 3) at the head of the buffer that `out` (21 * 8 modes) covers
    small = Problem(sf, torch_mod, (3, 3, 3), 21, "float64", 1)
    t = torch_mod.zeros(21 * 8, dtype=torch_mod.float64, device="cuda")
    t[:18] = small.tabs[2]
    with pytest.raises(sf.capi.SumfactError) as ei:
        small.run(sf, tabs=[small.tabs[0], small.tabs[1], t[:18]], out=t)
    assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(p.g, keep)
