"""GPU tests of the fused Helmholtz operator (include/sumfact.h sf_helmholtz_*),
y_e = B^T [lambda diag(w_e) + sum_ab D_a^T diag(G_ab,e) D_b] B x_e in one kernel: every wave order through AUTO, ragged
counts, the any-extent fallback, scalar-aligned views, guard values around `out` with `g` and `w` between NaN bands, the
Laplacian without `w`, the mass limit, every metric component on its own, symmetry and semidefiniteness, the
Gauss-Lobatto null-space and energy identities, a 262 144-element batch, stream capture and two streams in flight.

Reference and bound: tests/helm_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double reference,
gamma_N = N u / (1 - N u), N = 2 sum nq_d + 2 max nq_d + 2 d + 3, u = 2^-53 (fp64) or 2^-24 (fp32); where long double
would be too slow, 2 gamma_N (1 + gamma_N) * absref64 against fp64 CPU sweeps (both sides within gamma_N of the truth).
Data: seeded, per-value distinct; g uniform in (-1, 1) and so not definite -- every component and sign is exercised.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helm_ref import (COMPONENTS, U64, exact_energy, gamma, gll_setup, helm_excess, helm_n, helmholtz_f64, ref_helmholtz,
                      symmetry_bound, unit_roundoff)
from mass_ref import mass_excess, mass_n, ref_mass

pytestmark = pytest.mark.gpu

WAVE_ORDERS = [(3, n) for n in range(2, 9)] + [(2, n) for n in range(2, 17)]
RAGGED = [1, 2, 3, 5, 13, 15, 63, 65, 127, 257, 1001]
FALLBACK = [(6, 6, 12), (3, 5, 4), (12, 10, 11), (2, 3, 2), (9, 9, 9), (11, 11, 11), (12, 12, 12), (4, 9), (16, 3),
            (32, 32), (23, 5)]
LAM = 0.75


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
    return None if t is None else t.detach().cpu().numpy()


def _sizes(nq):
    return int(np.prod([q - 1 for q in nq])), int(np.prod(nq))


def _ncomp(nq):
    return len(COMPONENTS[len(nq)])


class Problem:
    """Seeded data of one case, on the device."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.nq, self.nelmt, self.dtype_name = tuple(nq), nelmt, dtype_name
        nmt, nqt = _sizes(nq)
        self.bs = [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ds = [sf.fill_random(q * q, 600 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.g = sf.fill_random(nelmt * _ncomp(nq) * nqt, 8000 + seed, dtype=dtype)
        self.w = sf.fill_random(nelmt * nqt, 7000 + seed, dtype=dtype)
        self.x = sf.fill_random(nelmt * nmt, 10 + seed, dtype=dtype)

    def run(self, sf, lam=LAM, **kw):
        x = kw.pop("x", self.x)
        g = kw.pop("g", self.g)
        w = kw.pop("w", self.w)
        bs = kw.pop("bs", self.bs)
        ds = kw.pop("ds", self.ds)
        f = sf.helmholtz_hex if len(self.nq) == 3 else sf.helmholtz_quad
        return f(self.nq, *bs, *ds, g, w, lam, x, **kw)

    def check(self, got, what, lam=LAM, x=None, g=None, w="self"):
        x = self.x if x is None else x
        g = self.g if g is None else g
        w = self.w if isinstance(w, str) else w
        ref, absref = ref_helmholtz(self.nq, self.nelmt, [_np(b) for b in self.bs], [_np(d) for d in self.ds], _np(g),
                                    _np(w), lam, _np(x))
        q = helm_excess(_np(got), ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt} lam={lam}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, self.nelmt, q)
        assert float(np.max(np.abs(ref))) > 0


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("dim,nq", WAVE_ORDERS, ids=[f"{d}d-nq{n}" for d, n in WAVE_ORDERS])
def test_auto_every_wave_order(sf, torch_mod, dim, nq, dtype_name):
    p = Problem(sf, torch_mod, (nq,) * dim, 403, dtype_name, nq)
    got = p.run(sf)
    torch_mod.cuda.synchronize()
    p.check(got, "auto")
    lap = p.run(sf, lam=0.0, w=None)
    torch_mod.cuda.synchronize()
    p.check(lap, "auto laplacian", lam=0.0, w=None)
    if dtype_name == "float64":
        # AUTO runs the wave kernel here: the same bits as the explicit variant
        wave = p.run(sf, variant="wave")
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(got, wave)


RAGGED_SHAPES = [((2, 2, 2), "float64"), ((3, 3, 3), "float64"), ((4, 4, 4), "float64"), ((6, 6, 6), "float64"),
                 ((7, 7, 7), "float64"), ((8, 8, 8), "float64"),
                 ((3, 3), "float64"), ((7, 7), "float64"), ((8, 8), "float64"), ((12, 12), "float64"),
                 ((16, 16), "float64"),
                 ((3, 3, 3), "float32"), ((6, 6, 6), "float32"), ((8, 8, 8), "float32"), ((7, 7), "float32"),
                 ((13, 13), "float32")]


@pytest.mark.parametrize("nq,dtype_name", RAGGED_SHAPES, ids=[_ids(s) + "-" + d for s, d in RAGGED_SHAPES])
def test_ragged_counts(sf, torch_mod, nq, dtype_name):
    """The last chunk is partial, or the whole batch is smaller than one chunk; g and w end where the batch ends."""
    for nelmt in RAGGED:
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, nelmt % 101)
        got = p.run(sf)
        torch_mod.cuda.synchronize()
        p.check(got, "ragged")


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("nq", FALLBACK, ids=_ids)
def test_fallback_shapes(sf, torch_mod, nq, dtype_name):
    for nelmt in (1, 37, 150):
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 70 + nelmt)
        got = p.run(sf)
        torch_mod.cuda.synchronize()
        p.check(got, "fallback")
        if dtype_name == "float64":
            gen = p.run(sf, variant="generic")
            torch_mod.cuda.synchronize()
            assert torch_mod.equal(got, gen)
    lap = p.run(sf, lam=0.0, w=None)
    torch_mod.cuda.synchronize()
    p.check(lap, "fallback laplacian", lam=0.0, w=None)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (9, 9)], ids=_ids)
def test_explicit_wave_and_generic(sf, torch_mod, nq):
    p = Problem(sf, torch_mod, nq, 777, "float64", 9)
    for variant in ("wave", "generic"):
        got = p.run(sf, variant=variant)
        torch_mod.cuda.synchronize()
        p.check(got, variant)


def test_variants_off_the_table(sf, torch_mod):
    p = Problem(sf, torch_mod, (9, 9, 9), 5, "float64", 2)
    with pytest.raises(sf.capi.SumfactError) as ei:
        p.run(sf, variant="wave")
    assert ei.value.rc == sf.capi.SF_ENOTBUILT
    with pytest.raises(sf.capi.SumfactError) as ei:
        p.run(sf, variant="mfma")
    assert ei.value.rc == sf.capi.SF_ENOTBUILT
    big = Problem(sf, torch_mod, (13, 4, 4), 2, "float64", 2)
    with pytest.raises(sf.capi.SumfactError) as ei:
        big.run(sf)
    assert ei.value.rc == sf.capi.SF_ENOTBUILT


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=_ids)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """Scalar-aligned views of in, out, g and w.  AUTO is correct through the fallback when in or out lacks 16-byte
    alignment, and through the wave kernel when only g / w do; guards on both sides of out are untouched; variant "wave"
    refuses in / out with SF_EALIGN."""
    nelmt = 133
    nmt, nqt = _sizes(nq)
    nc = _ncomp(nq)
    cases = (("float64", ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (1, 3, 1, 3))),
             ("float32", ((2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 3), (1, 3, 3, 1))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 4)
        for off_in, off_out, off_g, off_w in offsets:
            xbuf = sf.fill_random(nelmt * nmt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nmt]
            gbuf = sf.fill_random(nelmt * nc * nqt + 8, 60 + off_g, dtype=dtype)
            g = gbuf[off_g:off_g + nelmt * nc * nqt]
            wbuf = sf.fill_random(nelmt * nqt + 8, 70 + off_w, dtype=dtype)
            w = wbuf[off_w:off_w + nelmt * nqt]
            obuf = torch_mod.full((nelmt * nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * nmt]
            p.run(sf, x=x, g=g, w=w, out=o)
            torch_mod.cuda.synchronize()
            p.check(o, f"view {off_in}/{off_out}/{off_g}/{off_w}", x=x, g=g, w=w)
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * nmt:] == 7.25).all())
            if dtype_name == "float64":
                if off_in or off_out:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        p.run(sf, x=x, g=g, w=w, out=o, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                    gen = p.run(sf, x=x, g=g, w=w, variant="generic")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(gen, o)      # AUTO took the fallback
                else:
                    wave = p.run(sf, x=x, g=g, w=w, variant="wave")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(wave, o)     # g and w need only scalar alignment on the wave route


GUARD = [((3, 3, 3), 1001), ((6, 6, 6), 129), ((7, 7, 7), 257), ((8, 8, 8), 65), ((2, 2, 2), 33), ((5, 5), 4099),
         ((13, 13), 1000), ((16, 16), 127), ((6, 6, 12), 13), ((23, 5), 14), ((9, 9, 9), 15)]


@pytest.mark.parametrize("nq,nelmt", GUARD, ids=[_ids(s) for s, _ in GUARD])
def test_guard_values_around_out_and_nan_around_g_and_w(sf, torch_mod, nq, nelmt):
    """`out` sits between two guard bands (16-byte aligned, so the wave kernels run): only its own values change.  `g` and
    `w` are views inside larger buffers filled with NaN on both sides: a value read from outside that reached a result
    would show as a NaN in `out`."""
    nmt, nqt = _sizes(nq)
    nc = _ncomp(nq)
    for dtype_name, pad in (("float64", 64), ("float32", 128)):
        dtype = getattr(torch_mod, dtype_name)
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 5)
        gbuf = torch_mod.full((nelmt * nc * nqt + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        gbuf[pad:pad + nelmt * nc * nqt] = p.g
        g = gbuf[pad:pad + nelmt * nc * nqt]
        wbuf = torch_mod.full((nelmt * nqt + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
        wbuf[pad:pad + nelmt * nqt] = p.w
        w = wbuf[pad:pad + nelmt * nqt]
        obuf = torch_mod.full((nelmt * nmt + 2 * pad,), -3.5, dtype=dtype, device="cuda")
        o = obuf[pad:pad + nelmt * nmt]
        p.run(sf, g=g, w=w, out=o)
        torch_mod.cuda.synchronize()
        assert bool((obuf[:pad] == -3.5).all()) and bool((obuf[pad + nelmt * nmt:] == -3.5).all()), dtype_name
        assert not bool(torch_mod.isnan(o).any()), dtype_name
        p.check(o, "guard")


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (3, 3), (6, 6, 12), (23, 5)], ids=_ids)
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


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((4, 4, 4), "float32"), ((12, 12), "float64"),
                                           ((7, 7), "float32"), ((6, 6, 12), "float64"), ((4, 9), "float64")],
                         ids=lambda v: _ids(v))
def test_mass_limit(sf, torch_mod, nq, dtype_name):
    """g = 0, lambda = 1 is the mass operator: against tests/mass_ref.py with ITS bound (N = 2 sum nq + 1 roundings; the
    zero fluxes add exact zeros)."""
    p = Problem(sf, torch_mod, nq, 257, dtype_name, 31)
    got = p.run(sf, lam=1.0, g=torch_mod.zeros_like(p.g))
    torch_mod.cuda.synchronize()
    ref, absref = ref_mass(nq, p.nelmt, [_np(b) for b in p.bs], _np(p.w), _np(p.x))
    q = mass_excess(_np(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"mass limit {nq} {dtype_name}: max |err| / (gamma_{mass_n(nq)} absref) = {q:.3g}")
    assert q <= 1.0


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (7, 7), (4, 9)], ids=_ids)
def test_each_metric_component_alone(sf, torch_mod, nq):
    """One-hot component planes: pins the component order and that an off-diagonal plane enters both (a,b) and (b,a)."""
    nmt, nqt = _sizes(nq)
    nc = _ncomp(nq)
    p = Problem(sf, torch_mod, nq, 131, "float64", 41)
    for c in range(nc):
        g = torch_mod.zeros_like(p.g).view(p.nelmt, nc, nqt)
        g[:, c] = p.g.view(p.nelmt, nc, nqt)[:, c]
        g = g.reshape(-1)
        got = p.run(sf, lam=0.0, w=None, g=g)
        torch_mod.cuda.synchronize()
        p.check(got, f"component {COMPONENTS[len(nq)][c]}", lam=0.0, w=None, g=g)
        assert float(got.abs().max()) > 0


def _dots(a, b, nelmt):
    a, b = _np(a).reshape(nelmt, -1), _np(b).reshape(nelmt, -1)
    return [math.fsum(a[e] * b[e]) for e in range(nelmt)]


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12), (5, 5, 5), (6, 6, 12)], ids=_ids)
def test_symmetry_and_semidefiniteness(sf, torch_mod, nq):
    """|<A x, y> - <x, A y>| <= 2 (gamma_N + gamma_m) sum_e <|A||x|, |y|>_e for an indefinite g; and <A x, x> >= -bound
    per element for G = L L^T per point with lambda w >= 0."""
    nelmt = 503
    dim = len(nq)
    nmt, nqt = _sizes(nq)
    nc = _ncomp(nq)
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 12)
    y = sf.fill_random(nelmt * nmt, 122)
    ax, ay = p.run(sf), p.run(sf, x=y)
    aabs = p.run(sf, bs=[b.abs() for b in p.bs], ds=[d.abs() for d in p.ds], g=p.g.abs(), w=p.w.abs(), x=p.x.abs())
    torch_mod.cuda.synchronize()
    lhs, rhs = math.fsum(_dots(ax, y, nelmt)), math.fsum(_dots(p.x, ay, nelmt))
    scale = math.fsum(_dots(aabs, y.abs(), nelmt))
    bound = symmetry_bound(nq, U64) * scale
    print(f"symmetry {nq}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0
    # G = L L^T from a lower-triangular L of the seeded planes
    L = p.g.view(nelmt, nc, nqt)
    tri = {}
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        tri[(b, a)] = L[:, c]                                    # L[b][a], b >= a
    spd = torch_mod.empty_like(L)
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        spd[:, c] = sum(tri[(a, k)] * tri[(b, k)] for k in range(a + 1))
    spd = spd.reshape(-1)
    w = p.w.abs()
    e1 = p.run(sf, g=spd, w=w)
    eabs = p.run(sf, bs=[b.abs() for b in p.bs], ds=[d.abs() for d in p.ds], g=spd.abs(), w=w, x=p.x.abs())
    torch_mod.cuda.synchronize()
    energy, slack = _dots(e1, p.x, nelmt), _dots(eabs, p.x.abs(), nelmt)
    f = symmetry_bound(nq, U64)
    worst = min(en + f * sl for en, sl in zip(energy, slack))
    print(f"semidefinite {nq}: min energy {min(energy):.3e}, min (energy + bound) {worst:.3e}")
    assert worst >= 0 and math.fsum(energy) > 0


@pytest.mark.parametrize("dim,nq", [(3, 8), (2, 12)], ids=["3d-nq8", "2d-nq12"])
def test_gll_null_space_and_energy(sf, torch_mod, dim, nq):
    """Legendre modal basis at the Gauss-Lobatto points, the GLL differentiation matrix, G = I * (tensor GLL weight): a
    constant field is in the null space of the Laplacian (within gamma_N absref), and x^T A x equals the exact
    int |grad u|^2 within 2 (gamma_N + gamma_m) sum |x| |A| |x| (the rule of symmetry_bound())."""
    nelmt = 67
    ext = (nq,) * dim
    nmt, nqt = _sizes(ext)
    bases, derivs, g, w = gll_setup(nq, dim, nelmt)
    tb = [torch_mod.tensor(b, device="cuda") for b in bases]
    td = [torch_mod.tensor(d, device="cuda") for d in derivs]
    tg, tw = torch_mod.tensor(g, device="cuda"), torch_mod.tensor(w, device="cuda")
    f = sf.helmholtz_hex if dim == 3 else sf.helmholtz_quad
    const = np.zeros((nelmt, nmt))
    const[:, 0] = 1.0 + np.arange(nelmt)                        # mode (0,0,0) is the constant P_0
    xc = torch_mod.tensor(const.reshape(-1), device="cuda")
    yc = f(ext, *tb, *td, tg, None, 0.0, xc)
    torch_mod.cuda.synchronize()
    ref, absref = ref_helmholtz(ext, nelmt, bases, derivs, g, None, 0.0, const.reshape(-1))
    q = helm_excess(_np(yc), ref, absref, ext, U64)
    print(f"null space {ext}: max |A 1| = {float(yc.abs().max()):.3e}, excess {q:.3g}")
    assert q <= 1.0
    assert float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))) <= gamma(helm_n(ext), U64) * float(np.max(absref))
    x = sf.fill_random(nelmt * nmt, 77)
    y = f(ext, *tb, *td, tg, None, 0.0, x)
    yabs = f(ext, *[b.abs() for b in tb], *[d.abs() for d in td], tg, None, 0.0, x.abs())
    torch_mod.cuda.synchronize()
    got, slack = _dots(y, x, nelmt), _dots(yabs, x.abs(), nelmt)
    xs = _np(x).reshape(nelmt, -1)
    fac = symmetry_bound(ext, U64)
    worst = 0.0
    for e in range(nelmt):
        exact = exact_energy(nq, dim, xs[e])
        worst = max(worst, abs(got[e] - exact) / (fac * slack[e]))
        assert exact > 0
    print(f"energy {ext}: max |x^T A x - exact| / bound = {worst:.3g}")
    assert worst <= 1.0


def test_large_batch_hex8(sf, torch_mod):
    """262 144 elements at 3D nq = 8: a fixed seeded sample of elements against helm_ref's fp64 sweeps (bound
    2 gamma_N (1 + gamma_N) absref64); a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 1 << 18
    nmt, nqt = 343, 512
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 8)
    y = p.run(sf)
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(20240611)
    sample = np.unique(np.concatenate(([0, 1, 7, 8, nelmt - 9, nelmt - 8, nelmt - 1], rng.integers(0, nelmt, 4096))))
    idx = torch_mod.tensor(sample, device="cuda")
    pick = lambda t, n: _np(t.view(nelmt, n)[idx].reshape(-1))      # noqa: E731
    out64, abs64 = helmholtz_f64(nq, len(sample), [_np(b) for b in p.bs], [_np(d) for d in p.ds], pick(p.g, 6 * nqt),
                                 pick(p.w, nqt), LAM, pick(p.x, nmt))
    gN = gamma(helm_n(nq), U64)
    worst = helm_excess(pick(y, nmt), out64, abs64, nq, U64, factor=2 * (1 + gN))
    print(f"large batch ({len(sample)} sampled elements): max |err| / (2 gamma_N (1 + gamma_N) absref64) = {worst:.3g}")
    assert worst <= 1.0
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


@pytest.mark.parametrize("nq,nelmt", [((8, 8, 8), 20011), ((9, 9), 5003), ((6, 6, 12), 1001)], ids=lambda v: _ids(v))
def test_captured_graph_replay_matches_eager(sf, torch_mod, nq, nelmt):
    nmt, _ = _sizes(nq)
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 11)
    eager = p.run(sf)
    o = torch_mod.zeros(nelmt * nmt, dtype=torch_mod.float64, device="cuda")
    torch_mod.cuda.synchronize()
    side = torch_mod.cuda.Stream()
    side.wait_stream(torch_mod.cuda.current_stream())
    g = torch_mod.cuda.CUDAGraph()
    with torch_mod.cuda.stream(side):
        with torch_mod.cuda.graph(g, stream=side):
            p.run(sf, out=o, stream=side)
    torch_mod.cuda.current_stream().wait_stream(side)
    g.replay()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(o, eager)
    assert float(o.abs().max()) > 0


FIRST_CALL_CAPTURED = r"""
import sys
import torch
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
sf = ge.load_package()
for nq, nelmt in (((8, 8, 8), 5001), ((6, 6, 12), 301), ((9, 9), 2001), ((23, 5), 301)):
    f = sf.helmholtz_hex if len(nq) == 3 else sf.helmholtz_quad
    dim = len(nq)
    bs = [sf.fill_random((q - 1) * q, 40 + d) for d, q in enumerate(nq)]
    ds = [sf.fill_random(q * q, 50 + d) for d, q in enumerate(nq)]
    npt, nmo = 1, 1
    for q in nq:
        npt, nmo = npt * q, nmo * (q - 1)
    x = sf.fill_random(nelmt * nmo, 41)
    g = sf.fill_random(nelmt * npt * dim * (dim + 1) // 2, 43)
    w = sf.fill_random(nelmt * npt, 42)
    o = torch.zeros(nelmt * nmo, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(gr, stream=side):
            f(nq, *bs, *ds, g, w, 0.5, x, out=o, stream=side)     # the process's first call of this route
    torch.cuda.current_stream().wait_stream(side)
    gr.replay()
    torch.cuda.synchronize()
    eager = f(nq, *bs, *ds, g, w, 0.5, x)
    torch.cuda.synchronize()
    assert torch.equal(o, eager), nq
    assert float(o.abs().max()) > 0, nq
print("first calls captured")
"""


def test_first_call_inside_a_capture():
    """Capture-safe from the first call: a fresh child process whose first fused call of each route (3D wave, 3D
    fallback, 2D wave, 2D fallback) is inside a stream capture; the replay equals an eager call made afterwards."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", FIRST_CALL_CAPTURED, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first calls captured" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_two_streams_in_flight(sf, torch_mod):
    """Two problems enqueued on two streams before either is waited for; each against fp64 CPU sweeps."""
    jobs = [((7, 7, 7), 30011), ((12, 12), 100003)]
    streams = [torch_mod.cuda.Stream(), torch_mod.cuda.Stream()]
    probs = [Problem(sf, torch_mod, nq, nelmt, "float64", nelmt % 97) for nq, nelmt in jobs]
    torch_mod.cuda.synchronize()
    outs = []
    for p, st in zip(probs, streams):
        with torch_mod.cuda.stream(st):
            outs.append(p.run(sf, stream=st))
    torch_mod.cuda.synchronize()
    for p, o in zip(probs, outs):
        out64, abs64 = helmholtz_f64(p.nq, p.nelmt, [_np(b) for b in p.bs], [_np(d) for d in p.ds], _np(p.g), _np(p.w),
                                     LAM, _np(p.x))
        gN = gamma(helm_n(p.nq), U64)
        q = helm_excess(_np(o), out64, abs64, p.nq, U64, factor=2 * (1 + gN))
        print(f"stream job {p.nq}: {q:.3g}")
        assert q <= 1.0, p.nq


def test_overlap_is_refused(sf, torch_mod):
    """out == in, out inside g, out inside w: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    keep = p.x.clone()
    for o in (p.x, p.g[512:512 + nelmt * 343], p.w[:nelmt * 343]):
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, out=o)
        assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(p.x, keep)
