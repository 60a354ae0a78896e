"""GPU tests of the fused Helmholtz operator on affine elements (include/sumfact.h sf_affine_helmholtz_*) that are the
family's own: scalar-aligned views, the Laplacian that never reads je, every ge component on its own, the mass limit,
agreement with sf_helmholtz_* on expanded planes, the null-space and energy identities on affine geometry, symmetry, a
20 011-element batch and refused overlaps.  install() adds the family's cases of the parametrised tests the fused
families share (tests/fused_common.py: every wave order through AUTO, ragged counts, the fallback, explicit variants,
guard bands); refusals, stream capture and two streams in flight are tests/test_gpu_fused_common.py.

Reference and bound: tests/affine_ref.py.  Elementwise |gpu - ref| <= gamma_N' * absref against a long-double reference
on the expanded planes, N' = helm_n(nq) + d, u = 2^-53 (fp64) or 2^-24 (fp32).  Data: seeded, distinct per element and
per value, uniform in [-1, 1) -- the signs of qw, ge and je included, so ge is not definite.  A reference is computed
once per problem; a run on fewer elements takes a prefix of the same arrays and is compared with the prefix of it.
"""
import math

import numpy as np
import pytest

from affine_ref import (affine_excess, affine_geometry, affine_n, exact_energy_affine, expand, gll_affine_setup,
                        ref_affine)
from fused_common import install
from fused_families import BY_NAME, case_id, sf, to_host, torch_mod  # noqa: F401
from helm_ref import COMPONENTS, U64, gamma, symmetry_bound, unit_roundoff
from mass_ref import mass_excess, mass_n, ref_mass

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["affine"])

LAM = 0.75


def _nmt(nq):
    return int(np.prod([q - 1 for q in nq]))


def _ncomp(nq):
    return len(COMPONENTS[len(nq)])


class Problem:
    """Seeded data of one case on the device, and its long-double references (computed on first use, per lambda)."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.sf, self.nq, self.nelmt, self.dtype_name = sf, tuple(nq), nelmt, dtype_name
        self.nmt, self.nc = _nmt(nq), _ncomp(nq)
        self.bs = [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ds = [sf.fill_random(q * q, 600 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.qs = [sf.fill_random(q, 700 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ge = sf.fill_random(nelmt * self.nc, 8000 + seed, dtype=dtype)
        self.je = sf.fill_random(nelmt, 7000 + seed, dtype=dtype)
        self.x = sf.fill_random(nelmt * self.nmt, 10 + seed, dtype=dtype)
        self._refs = {}

    def run(self, lam=LAM, n=None, **kw):
        """The operator on the first n elements (all by default); je=None with lam == 0."""
        n = self.nelmt if n is None else n
        x = kw.pop("x", self.x)[:n * self.nmt]
        ge = kw.pop("ge", self.ge)[:n * self.nc]
        je = kw.pop("je", self.je if lam != 0 else None)
        je = None if je is None else je[:n]
        bs, ds, qs = kw.pop("bs", self.bs), kw.pop("ds", self.ds), kw.pop("qs", self.qs)
        f = self.sf.affine_helmholtz_hex if len(self.nq) == 3 else self.sf.affine_helmholtz_quad
        return f(self.nq, *bs, *ds, *qs, ge, je, lam, x, **kw)

    def ref(self, lam=LAM):
        if lam not in self._refs:
            self._refs[lam] = ref_affine(self.nq, self.nelmt, [to_host(b) for b in self.bs], [to_host(d) for d in self.ds],
                                         [to_host(q) for q in self.qs], to_host(self.ge), to_host(self.je) if lam != 0 else None, lam,
                                         to_host(self.x))
        return self._refs[lam]

    def check(self, got, what, lam=LAM, n=None):
        n = self.nelmt if n is None else n
        ref, absref = self.ref(lam)
        ref, absref = ref[:n * self.nmt], absref[:n * self.nmt]
        q = affine_excess(to_host(got), ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={n} lam={lam}: max |err| / (gamma_N' absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, n, q)
        assert float(np.max(np.abs(ref))) > 0

    def check_other(self, got, what, lam, **data):
        """Against a reference of its own, for a run with some array replaced (host copies given by name)."""
        a = {"bs": [to_host(b) for b in self.bs], "ds": [to_host(d) for d in self.ds], "qs": [to_host(q) for q in self.qs],
             "ge": to_host(self.ge), "je": to_host(self.je) if lam != 0 else None, "x": to_host(self.x)}
        a.update(data)
        ref, absref = ref_affine(self.nq, self.nelmt, a["bs"], a["ds"], a["qs"], a["ge"], a["je"], lam, a["x"])
        q = affine_excess(to_host(got), ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt} lam={lam}: max |err| / (gamma_N' absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, q)
        assert float(np.max(np.abs(ref))) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """in or out at a scalar offset: correct through the fallback, WAVE answers SF_EALIGN.  ge / je / qw at odd scalar
    offsets: still the wave kernel, bit-equal to WAVE.  Guards on both sides of out are untouched."""
    nelmt = 133
    cases = (("float64", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 3, 3))), ("float32", ((1, 0, 0), (0, 1, 0), (0, 0, 1), (3, 1, 3))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 4)

        def view(t, off):
            buf = torch_mod.full((t.numel() + 8,), float("nan"), dtype=dtype, device="cuda")
            buf[off:off + t.numel()] = t
            return buf[off:off + t.numel()]

        for off_in, off_out, off_c in offsets:
            x, ge, je = view(p.x, off_in), view(p.ge, off_c), view(p.je, off_c)
            qs = [view(q, off_c) for q in p.qs]
            assert not off_c or ge.data_ptr() % (2 * ge.element_size()) != 0
            obuf = torch_mod.full((nelmt * p.nmt + 16,), 7.25, dtype=dtype, device="cuda")
            o = obuf[off_out:off_out + nelmt * p.nmt]
            p.run(x=x, ge=ge, je=je, qs=qs, out=o)
            torch_mod.cuda.synchronize()
            p.check(o, f"view {off_in}/{off_out}/{off_c}")
            assert bool((obuf[:off_out] == 7.25).all()) and bool((obuf[off_out + nelmt * p.nmt:] == 7.25).all())
            if dtype_name == "float64":
                if off_in or off_out:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        p.run(x=x, ge=ge, je=je, qs=qs, out=o, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                    gen = p.run(x=x, ge=ge, je=je, qs=qs, variant="generic")
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(gen, o)      # AUTO took the fallback
                else:
                    wave = p.run(variant="wave")        # the aligned originals
                    torch_mod.cuda.synchronize()
                    assert torch_mod.equal(wave, o)     # ge, je and qw need only scalar alignment on the wave route


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (3, 3), (6, 6, 12), (23, 5)], ids=case_id)
def test_laplacian_never_reads_je(sf, torch_mod, nq):
    """lambda == 0 with je=None equals lambda == 0 with a NaN-filled je, bit for bit, in both precisions."""
    for dtype_name in ("float64", "float32"):
        p = Problem(sf, torch_mod, nq, 301, dtype_name, 21)
        none = p.run(lam=0.0)
        nan = p.run(lam=0.0, je=torch_mod.full_like(p.je, float("nan")))
        torch_mod.cuda.synchronize()
        assert not bool(torch_mod.isnan(none).any())
        assert torch_mod.equal(none, nan), (nq, dtype_name)
        p.check(none, "laplacian", lam=0.0)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (4, 9)], ids=case_id)
def test_each_ge_component_alone(sf, torch_mod, nq):
    """One-hot components: pins the component order and that an off-diagonal component enters both (a,b) and (b,a)."""
    p = Problem(sf, torch_mod, nq, 67, "float64", 41)
    for c in range(p.nc):
        ge = torch_mod.zeros_like(p.ge).view(p.nelmt, p.nc)
        ge[:, c] = p.ge.view(p.nelmt, p.nc)[:, c]
        ge = ge.reshape(-1)
        got = p.run(lam=0.0, ge=ge)
        torch_mod.cuda.synchronize()
        p.check_other(got, f"component {COMPONENTS[len(nq)][c]}", 0.0, ge=to_host(ge))
        assert float(got.abs().max()) > 0


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((4, 4, 4), "float32"), ((12, 12), "float64"),
                                           ((7, 7), "float32"), ((6, 6, 12), "float64"), ((4, 9), "float64")],
                         ids=lambda v: case_id(v))
def test_mass_limit(sf, torch_mod, nq, dtype_name):
    """ge = 0, lambda = 1 is the mass operator with w = je (x) qw: against tests/mass_ref.py on the w expanded in long
    double.  mass_ref counts one rounding for the weight (N = 2 sum nq + 1); here the weight takes d + 1 -- d - 1 for q,
    one for je q, one times u (lambda je is exact at lambda = 1) -- so the bound is gamma_(N + d) absref; the zero fluxes
    add exact zeros."""
    p = Problem(sf, torch_mod, nq, 131, dtype_name, 31)
    got = p.run(lam=1.0, ge=torch_mod.zeros_like(p.ge))
    torch_mod.cuda.synchronize()
    _, w = expand(nq, p.nelmt, [to_host(q) for q in p.qs], np.zeros(p.nelmt * p.nc), to_host(p.je))
    ref, absref = ref_mass(nq, p.nelmt, [to_host(b) for b in p.bs], w, to_host(p.x))
    u = unit_roundoff(dtype_name)
    n = mass_n(nq)
    q = mass_excess(to_host(got), ref, absref, nq, u, factor=gamma(n + len(nq), u) / gamma(n, u))
    print(f"mass limit {nq} {dtype_name}: max |err| / (gamma_{n + len(nq)} absref) = {q:.3g}")
    assert q <= 1.0 and float(np.max(np.abs(ref))) > 0


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((5, 5, 5), "float32"), ((12, 12), "float64"),
                                           ((6, 6, 12), "float64"), ((9, 9), "float32")], ids=lambda v: case_id(v))
def test_agrees_with_helmholtz_on_expanded_planes(sf, torch_mod, nq, dtype_name):
    """sf_helmholtz_* on g and w expanded on the device in working precision, and sf_affine_helmholtz_*: both inside the
    bound of the same long-double reference."""
    p = Problem(sf, torch_mod, nq, 203, dtype_name, 51)
    q = p.qs[0]
    for qd in p.qs[1:]:
        q = torch_mod.outer(qd, q.reshape(-1)).reshape(-1)
    g = (p.ge.view(p.nelmt, p.nc, 1) * q.view(1, 1, -1)).reshape(-1).contiguous()
    w = (p.je.view(p.nelmt, 1) * q.view(1, -1)).reshape(-1).contiguous()
    helm = sf.helmholtz_hex if len(nq) == 3 else sf.helmholtz_quad
    for lam in (LAM, 0.0):
        deformed = helm(nq, *p.bs, *p.ds, g, w if lam != 0 else None, lam, p.x)
        affine = p.run(lam=lam)
        torch_mod.cuda.synchronize()
        p.check(affine, "affine", lam=lam)
        p.check(deformed, "deformed on expanded planes", lam=lam)


def _dots(a, b, nelmt):
    a, b = to_host(a).reshape(nelmt, -1), to_host(b).reshape(nelmt, -1)
    return [math.fsum(a[e] * b[e]) for e in range(nelmt)]


@pytest.mark.parametrize("dim,nq", [(3, 5), (3, 8), (2, 8), (2, 12)], ids=["3d-nq5", "3d-nq8", "2d-nq8", "2d-nq12"])
def test_affine_geometry_null_space_and_energy(sf, torch_mod, dim, nq):
    """Legendre modal basis at the Gauss-Lobatto points, the GLL differentiation matrix and weights, seeded Jacobians
    J_e = I + 0.3 U(-1, 1), ge = |det J| J^-1 J^-T: a constant field is in the null space of the Laplacian (within
    gamma_N' absref), and x^T A x equals the exact int |grad u|^2 over the physical element -- Gauss-Legendre integrals,
    the mixed terms included -- within symmetry_bound * sum <|A||x|, |x|>."""
    nelmt = 67
    ext = (nq,) * dim
    nmt = _nmt(ext)
    bases, derivs, qws = gll_affine_setup(nq, dim)
    J, ge, je = affine_geometry(dim, nelmt, 100 + nq)
    dev = lambda a: torch_mod.tensor(np.ascontiguousarray(a), device="cuda")      # noqa: E731
    tb, td, tq, tge = [dev(b) for b in bases], [dev(d) for d in derivs], [dev(q) for q in qws], dev(ge)
    f = sf.affine_helmholtz_hex if dim == 3 else sf.affine_helmholtz_quad
    const = np.zeros((nelmt, nmt))
    const[:, 0] = 1.0 + np.arange(nelmt)                        # mode (0,0,0) is the constant P_0
    yc = f(ext, *tb, *td, *tq, tge, None, 0.0, dev(const.reshape(-1)))
    torch_mod.cuda.synchronize()
    ref, absref = ref_affine(ext, nelmt, bases, derivs, qws, ge, None, 0.0, const.reshape(-1))
    q = affine_excess(to_host(yc), ref, absref, ext, U64)
    print(f"null space {ext}: max |A 1| = {float(yc.abs().max()):.3e}, excess {q:.3g}")
    assert q <= 1.0
    assert float(np.max(np.abs(np.asarray(ref, dtype=np.float64)))) <= gamma(affine_n(ext), U64) * float(np.max(absref))
    x = sf.fill_random(nelmt * nmt, 77)
    y = f(ext, *tb, *td, *tq, tge, None, 0.0, x)
    yabs = f(ext, *[b.abs() for b in tb], *[d.abs() for d in td], *tq, tge.abs(), None, 0.0, x.abs())
    torch_mod.cuda.synchronize()
    got, slack = _dots(y, x, nelmt), _dots(yabs, x.abs(), nelmt)
    xs = to_host(x).reshape(nelmt, -1)
    fac = symmetry_bound(ext, U64)
    worst = 0.0
    for e in range(nelmt):
        exact = exact_energy_affine(nq, dim, xs[e], J[e])
        worst = max(worst, abs(got[e] - exact) / (fac * slack[e]))
        assert exact > 0
    print(f"energy {ext}: max |x^T A x - exact| / bound = {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12), (6, 6, 12)], ids=case_id)
def test_symmetry(sf, torch_mod, nq):
    """|<A x, y> - <x, A y>| <= symmetry_bound * sum_e <|A||x|, |y|>_e for an indefinite ge and weights of both signs."""
    nelmt = 257
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 12)
    y = sf.fill_random(nelmt * p.nmt, 122)
    ax, ay = p.run(), p.run(x=y)
    aabs = p.run(bs=[b.abs() for b in p.bs], ds=[d.abs() for d in p.ds], qs=[q.abs() for q in p.qs], ge=p.ge.abs(),
                 je=p.je.abs(), x=p.x.abs())
    torch_mod.cuda.synchronize()
    lhs, rhs = math.fsum(_dots(ax, y, nelmt)), math.fsum(_dots(p.x, ay, nelmt))
    bound = symmetry_bound(nq, U64) * math.fsum(_dots(aabs, y.abs(), nelmt))
    print(f"symmetry {nq}: |lhs - rhs| = {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound and abs(lhs) > 0


def test_batch_of_20011_hex8(sf, torch_mod):
    """20 011 elements at 3D nq = 8 (many workgroups, a ragged tail): a seeded sample of 64 elements and the last three
    against the long-double reference; a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 20011
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 8)
    y = p.run()
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(20240611)
    sample = np.unique(np.concatenate((rng.choice(nelmt - 3, 64, replace=False), [nelmt - 3, nelmt - 2, nelmt - 1])))
    assert len(sample) == 67
    idx = torch_mod.tensor(sample, device="cuda")
    pick = lambda t, n: to_host(t.view(nelmt, n)[idx].reshape(-1))      # noqa: E731
    ref, absref = ref_affine(nq, len(sample), [to_host(b) for b in p.bs], [to_host(d) for d in p.ds], [to_host(q) for q in p.qs],
                             pick(p.ge, p.nc), pick(p.je, 1), LAM, pick(p.x, p.nmt))
    worst = affine_excess(pick(y, p.nmt), ref, absref, nq, U64)
    print(f"20011 elements ({len(sample)} sampled): max |err| / (gamma_N' absref) = {worst:.3g}")
    assert worst <= 1.0
    again = p.run()
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


def test_overlap_is_refused(sf, torch_mod):
    """out == in, out over ge, out over je: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (3, 3, 3), 50
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    n = nelmt * p.nmt                                       # 400 scalars: longer than ge (300) and je (50)
    big = sf.fill_random(3 * n, 5)
    ge, je = big[n:n + nelmt * p.nc], big[2 * n - nelmt:2 * n]
    keep = big.clone()
    for o in (p.x, big[n - 8:2 * n - 8], big[n:2 * n]):     # in; the head of ge; ge and je
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(ge=ge, je=je, out=o)
        assert ei.value.rc == sf.capi.SF_EINVAL
    with pytest.raises(sf.capi.SumfactError) as ei:         # je alone: refused with lambda != 0 ...
        p.run(je=je, out=big[2 * n - 8:3 * n - 8])
    assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(big, keep)
    o = big[2 * n - 8:3 * n - 8]                            # ... and no argument at all with lambda == 0
    p.run(lam=0.0, je=je, out=o)
    torch_mod.cuda.synchronize()
    p.check(o, "out over an unused je", lam=0.0)
