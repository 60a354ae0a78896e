"""GPU tests of the fused Helmholtz operator (include/sumfact.h sf_helmholtz_*), y_e = B^T [lambda diag(w_e) + sum_ab
D_a^T diag(G_ab,e) D_b] B x_e in one kernel, that are the family's own: scalar-aligned views, the Laplacian that never
reads `w`, the mass limit, every metric component on its own, symmetry and semidefiniteness, the Gauss-Lobatto
null-space and energy identities, a 262 144-element batch and refused overlaps.  install() adds the family's cases of
the parametrised tests the fused families share (tests/fused_common.py: every wave order through AUTO, ragged counts,
the fallback, explicit variants, guard bands); refusals, stream capture and two streams in flight are
tests/test_gpu_fused_common.py.

Reference and bound: tests/helm_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double reference,
gamma_N = N u / (1 - N u), N = 2 sum nq_d + 2 max nq_d + 2 d + 3, u = 2^-53 (fp64) or 2^-24 (fp32); where long double
would be too slow, 2 gamma_N (1 + gamma_N) * absref64 against fp64 CPU sweeps (both sides within gamma_N of the truth).
Data: seeded, per-value distinct; g uniform in (-1, 1) and so not definite -- every component and sign is exercised.
"""
import math

import numpy as np
import pytest

from fused_common import install
from fused_families import BY_NAME, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from helm_ref import (COMPONENTS, U64, exact_energy, gamma, gll_setup, helm_excess, helm_n, helmholtz_f64, ref_helmholtz,
                      symmetry_bound, unit_roundoff)
from mass_ref import mass_excess, mass_n, ref_mass

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["helmholtz"])

LAM = 0.75


def _ncomp(nq):
    return len(COMPONENTS[len(nq)])


class Problem:
    """Seeded data of one case, on the device."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.nq, self.nelmt, self.dtype_name = tuple(nq), nelmt, dtype_name
        nmt, nqt = sizes(nq)
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
        ref, absref = ref_helmholtz(self.nq, self.nelmt, [to_host(b) for b in self.bs], [to_host(d) for d in self.ds], to_host(g),
                                    to_host(w), lam, to_host(x))
        q = helm_excess(to_host(got), ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt} lam={lam}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, self.nelmt, q)
        assert float(np.max(np.abs(ref))) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """Scalar-aligned views of in, out, g and w.  AUTO is correct through the fallback when in or out lacks 16-byte
    alignment, and through the wave kernel when only g / w do; guards on both sides of out are untouched; variant "wave"
    refuses in / out with SF_EALIGN."""
    nelmt = 133
    nmt, nqt = sizes(nq)
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


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((4, 4, 4), "float32"), ((12, 12), "float64"),
                                           ((7, 7), "float32"), ((6, 6, 12), "float64"), ((4, 9), "float64")],
                         ids=lambda v: case_id(v))
def test_mass_limit(sf, torch_mod, nq, dtype_name):
    """g = 0, lambda = 1 is the mass operator: against tests/mass_ref.py with ITS bound (N = 2 sum nq + 1 roundings; the
    zero fluxes add exact zeros)."""
    p = Problem(sf, torch_mod, nq, 257, dtype_name, 31)
    got = p.run(sf, lam=1.0, g=torch_mod.zeros_like(p.g))
    torch_mod.cuda.synchronize()
    ref, absref = ref_mass(nq, p.nelmt, [to_host(b) for b in p.bs], to_host(p.w), to_host(p.x))
    q = mass_excess(to_host(got), ref, absref, nq, unit_roundoff(dtype_name))
    print(f"mass limit {nq} {dtype_name}: max |err| / (gamma_{mass_n(nq)} absref) = {q:.3g}")
    assert q <= 1.0


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (7, 7), (4, 9)], ids=case_id)
def test_each_metric_component_alone(sf, torch_mod, nq):
    """One-hot component planes: pins the component order and that an off-diagonal plane enters both (a,b) and (b,a)."""
    nmt, nqt = sizes(nq)
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
    a, b = to_host(a).reshape(nelmt, -1), to_host(b).reshape(nelmt, -1)
    return [math.fsum(a[e] * b[e]) for e in range(nelmt)]


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12), (5, 5, 5), (6, 6, 12)], ids=case_id)
def test_symmetry_and_semidefiniteness(sf, torch_mod, nq):
    """|<A x, y> - <x, A y>| <= 2 (gamma_N + gamma_m) sum_e <|A||x|, |y|>_e for an indefinite g; and <A x, x> >= -bound
    per element for G = L L^T per point with lambda w >= 0."""
    nelmt = 503
    dim = len(nq)
    nmt, nqt = sizes(nq)
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
    nmt, nqt = sizes(ext)
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
    q = helm_excess(to_host(yc), ref, absref, ext, U64)
    print(f"null space {ext}: max |A 1| = {float(yc.abs().max()):.3e}, excess {q:.3g}")
    assert q <= 1.0
    assert float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))) <= gamma(helm_n(ext), U64) * float(np.max(absref))
    x = sf.fill_random(nelmt * nmt, 77)
    y = f(ext, *tb, *td, tg, None, 0.0, x)
    yabs = f(ext, *[b.abs() for b in tb], *[d.abs() for d in td], tg, None, 0.0, x.abs())
    torch_mod.cuda.synchronize()
    got, slack = _dots(y, x, nelmt), _dots(yabs, x.abs(), nelmt)
    xs = to_host(x).reshape(nelmt, -1)
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
    pick = lambda t, n: to_host(t.view(nelmt, n)[idx].reshape(-1))      # noqa: E731
    out64, abs64 = helmholtz_f64(nq, len(sample), [to_host(b) for b in p.bs], [to_host(d) for d in p.ds], pick(p.g, 6 * nqt),
                                 pick(p.w, nqt), LAM, pick(p.x, nmt))
    gN = gamma(helm_n(nq), U64)
    worst = helm_excess(pick(y, nmt), out64, abs64, nq, U64, factor=2 * (1 + gN))
    print(f"large batch ({len(sample)} sampled elements): max |err| / (2 gamma_N (1 + gamma_N) absref64) = {worst:.3g}")
    assert worst <= 1.0
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


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
