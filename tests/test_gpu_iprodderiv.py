"""GPU tests of IProductWRTDerivBase (include/sumfact.h sf_iprodderiv_*), out = sum_b B^T D_b^T (w sum_a df_ab f_a) in
one kernel, that are the family's own: an 8-byte-aligned `out`, scalar-aligned input views, df / w never read when None,
identity planes and a unit weight, every plane of df on its own, adjointness to sf_physderiv_* on the device,
composition against sf_helmholtz_*, physderiv_autograd, the three input forms, a 20 011-element batch and refused
overlaps.  install() adds the family's cases of the parametrised tests the fused families share (tests/fused_common.py:
every wave order through AUTO, ragged counts, the fallback, explicit variants, guard bands); refusals, stream capture
and two streams in flight are tests/test_gpu_fused_common.py.

Reference and bound: tests/iprodderiv_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double
reference, gamma_N = N u / (1 - N u), N = sum nq_d + max nq_d + 2 d, u = 2^-53 (fp64) or 2^-24 (fp32).
Data: seeded, per-value distinct (sf.fill_random); df and w uniform in (-1, 1), so every component and sign is exercised.
"""

import numpy as np
import pytest

from fused_common import install
from fused_families import BY_NAME, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from helm_ref import COMPONENTS, helm_n, ref_helmholtz
from iprodderiv_ref import (U64, gamma, iprodderiv_excess, iprodderiv_f64, iprodderiv_n, ref_iprodderiv, unit_roundoff)
from physderiv_ref import physderiv_n, ref_physderiv

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["iprodderiv"])



class Problem:
    """Seeded data of one case, on the device.  f: a contiguous (d, n) tensor."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.nq, self.nelmt, self.dtype_name, self.dim = tuple(nq), nelmt, dtype_name, len(nq)
        nmt, nqt = sizes(nq)
        self.bs = [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ds = [sf.fill_random(q * q, 600 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.df = sf.fill_random(nelmt * self.dim ** 2 * nqt, 8000 + seed, dtype=dtype)
        self.w = sf.fill_random(nelmt * nqt, 9000 + seed, dtype=dtype)
        self.f = sf.fill_random(self.dim * nelmt * nqt, 10 + seed, dtype=dtype).view(self.dim, nelmt * nqt)
        self.x = sf.fill_random(nelmt * nmt, 20 + seed, dtype=dtype)       # modes, for the tests that also run physderiv

    def run(self, sf, df="self", w="self", f=None, **kw):
        df = self.df if isinstance(df, str) else df
        w = self.w if isinstance(w, str) else w
        fn = sf.iprodderiv_hex if self.dim == 3 else sf.iprodderiv_quad
        return fn(self.nq, *self.bs, *self.ds, df, w, self.f if f is None else f, **kw)

    def physderiv(self, sf, df="self", **kw):
        df = self.df if isinstance(df, str) else df
        fn = sf.physderiv_hex if self.dim == 3 else sf.physderiv_quad
        return fn(self.nq, *self.bs, *self.ds, df, self.x, **kw)

    def reference(self, df="self", w="self", f=None):
        df = self.df if isinstance(df, str) else df
        w = self.w if isinstance(w, str) else w
        f = self.f if f is None else f
        rows = [to_host(r) for r in f]
        return ref_iprodderiv(self.nq, self.nelmt, [to_host(b) for b in self.bs], [to_host(d) for d in self.ds], to_host(df), to_host(w),
                              rows)

    def check(self, got, what, ref=None, **kw):
        ref, absref = self.reference(**kw) if ref is None else ref
        assert float(np.max(np.abs(ref))) > 0
        got = to_host(got)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        q = iprodderiv_excess(got, ref, absref, self.nq, unit_roundoff(self.dtype_name))
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, self.nelmt, q)


def test_wave_refuses_an_eight_byte_aligned_out(sf, torch_mod):
    """An 8-byte-aligned out: WAVE refuses it, AUTO takes the fallback and is correct."""
    for nq in ((8, 8, 8), (12, 12)):
        p = Problem(sf, torch_mod, nq, 19, "float64", 3)
        nmt, _ = sizes(nq)
        obuf = torch_mod.full((19 * nmt + 8,), 7.25, dtype=torch_mod.float64, device="cuda")
        out = obuf[1:1 + 19 * nmt]
        assert out.data_ptr() % 16 == 8
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, out=out, variant="wave")
        assert ei.value.rc == sf.capi.SF_EALIGN, nq
        p.run(sf, out=out)
        gen = p.run(sf, variant="generic")
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(out, gen)                               # AUTO took the fallback
        assert float(obuf[0]) == 7.25 and bool((obuf[1 + 19 * nmt:] == 7.25).all())
        p.check(out, "auto on an 8-byte-aligned out")


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (3, 3, 3), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_input_views(sf, torch_mod, nq):
    """Every in_a, df and w offset by one scalar (not 16-byte aligned), out 16-byte aligned: the inputs need scalar
    alignment only, so variant "wave" runs, AUTO gives its bits, and both sit inside the bound."""
    nelmt, dim = 45, len(nq)
    _, nqt = sizes(nq)
    n = nelmt * nqt
    for dtype_name in ("float64", "float32"):
        dtype = getattr(torch_mod, dtype_name)
        size = 8 if dtype_name == "float64" else 4
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 4)
        stride = (n + 8) // 4 * 4 + 4                                  # rows start 16-byte aligned, the views one scalar in
        fbuf = sf.fill_random(dim * stride, 50, dtype=dtype).view(dim, stride)
        fs = [fbuf[a, 1:1 + n] for a in range(dim)]
        df = sf.fill_random(dim * dim * n + 8, 60, dtype=dtype)[1:1 + dim * dim * n]
        w = sf.fill_random(n + 8, 61, dtype=dtype)[1:1 + n]
        for t in fs + [df, w]:
            assert t.data_ptr() % 16 == size
        got = p.run(sf, df=df, w=w, f=fs)
        torch_mod.cuda.synchronize()
        assert got.data_ptr() % 16 == 0
        p.check(got, "scalar-aligned inputs", df=df, w=w, f=fs)
        if dtype_name == "float64":
            wave = p.run(sf, df=df, w=w, f=fs, variant="wave")             # must not be refused
            torch_mod.cuda.synchronize()
            assert torch_mod.equal(got, wave)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (6, 6, 12), (23, 5)], ids=case_id)
def test_df_and_w_are_never_read_when_none(sf, torch_mod, nq):
    """df=None / w=None with no such buffer in existence (the problem's own are freed first; what stands beside them is
    a NaN-filled array of size 1): the result is finite and equals the reference, on wave and fallback shapes, in both
    precisions."""
    for dtype_name in ("float64", "float32"):
        p = Problem(sf, torch_mod, nq, 41, dtype_name, 21)
        ref = p.reference(df=None, w=None)
        p.df = p.w = None
        torch_mod.cuda.empty_cache()
        nan = torch_mod.full((1,), float("nan"), dtype=getattr(torch_mod, dtype_name), device="cuda")
        got = p.run(sf, df=None, w=None)
        torch_mod.cuda.synchronize()
        assert bool(torch_mod.isfinite(got).all()) and bool(torch_mod.isnan(nan).all())
        p.check(got, "df=None w=None", ref=ref)


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((7, 7), "float32"), ((6, 6, 12), "float64"),
                                           ((9, 9, 9), "float32"), ((12, 12), "float64")], ids=lambda v: case_id(v))
def test_identity_planes_and_unit_weight(sf, torch_mod, nq, dtype_name):
    """Identity planes of df give the values of df=None within the bound; a w of all ones is bit-identical to w=None
    (1 * t is exact)."""
    dim = len(nq)
    _, nqt = sizes(nq)
    p = Problem(sf, torch_mod, nq, 37, dtype_name, 51)
    ident = torch_mod.zeros_like(p.df).view(p.nelmt, dim, dim, nqt)
    for a in range(dim):
        ident[:, a, a] = 1.0
    got, none = p.run(sf, df=ident.reshape(-1)), p.run(sf, df=None)
    torch_mod.cuda.synchronize()
    p.check(got, "identity planes against df=None", df=None)
    p.check(none, "df=None", df=None)
    ones = torch_mod.ones_like(p.w)
    for df in (p.df, None):
        a, b = p.run(sf, df=df, w=ones), p.run(sf, df=df, w=None)
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(a, b)
        assert float(b.abs().max()) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (6, 4, 5), (12, 12), (4, 9)], ids=case_id)
def test_each_plane_alone(sf, torch_mod, nq):
    """One plane of df all ones, the others zero: out = B^T D_b^T (w f_a) for the plane c = a d + b.  A transposed
    a d + b would take another input and another derivative; the reference tells."""
    dim = len(nq)
    _, nqt = sizes(nq)
    p = Problem(sf, torch_mod, nq, 21, "float64", 41)
    seen = []
    for c in range(dim * dim):
        df = torch_mod.zeros_like(p.df).view(p.nelmt, dim * dim, nqt)
        df[:, c] = 1.0
        df = df.reshape(-1)
        got = p.run(sf, df=df)
        torch_mod.cuda.synchronize()
        p.check(got, f"plane {c}", df=df)
        seen.append(to_host(got))
    for c in range(dim * dim):
        for c2 in range(c):
            assert not np.array_equal(seen[c], seen[c2]), (c, c2)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (16, 16), (6, 6, 12)], ids=case_id)
def test_adjoint_of_physderiv_on_the_device(sf, torch_mod, nq, dtype_name):
    """<physderiv(x), f> against <x, iprodderiv(df, None, f)>, both products of the device results formed on the host in
    long double: the difference is at most (gamma_Nphys + gamma_N) times the inner product of absolute values,
    <|physderiv|(|x|), |f|> -- each side is within its elementwise bound of the same exact bilinear form."""
    ld = np.longdouble
    p = Problem(sf, torch_mod, nq, 29, dtype_name, 31)
    u = unit_roundoff(dtype_name)
    for df in (p.df, None):
        grad = p.physderiv(sf, df=df)
        div = p.run(sf, df=df, w=None)
        torch_mod.cuda.synchronize()
        f, x = to_host(p.f).astype(ld), to_host(p.x).astype(ld)
        lhs = np.sum(to_host(grad).astype(ld) * f)
        rhs = np.sum(x * to_host(div).astype(ld))
        _, gabs = ref_physderiv(nq, p.nelmt, [to_host(b) for b in p.bs], [to_host(d) for d in p.ds], to_host(df), to_host(p.x))
        bound = (gamma(physderiv_n(nq), u) + gamma(iprodderiv_n(nq), u)) * np.sum(gabs * np.abs(f))
        print(f"adjoint {nq} {dtype_name} df={'yes' if df is not None else 'None'}: |lhs - rhs| = "
              f"{float(abs(lhs - rhs)):.3e}, bound {float(bound):.3e}")
        assert abs(lhs - rhs) <= bound and abs(lhs) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (12, 12)], ids=case_id)
def test_composition_is_the_helmholtz_operator(sf, torch_mod, nq):
    """iprodderiv(df, w, physderiv(df, x)) against helmholtz(g, None, 0, x) with g_ab = w sum_c df_ca df_cb built on the
    host (long double, rounded once).  Both approximate the same exact operator: the composition within
    gamma_{Nphys + N + 1} of the operator on absolute values (the two chained bounds, one more rounding for g), the
    Helmholtz kernel within its own gamma_Nhelm absref; their difference is at most the sum of the two bounds."""
    ld = np.longdouble
    dim = len(nq)
    _, nqt = sizes(nq)
    p = Problem(sf, torch_mod, nq, 23, "float64", 61)
    dd = to_host(p.df).astype(ld).reshape(p.nelmt, dim * dim, nqt)
    ww = to_host(p.w).astype(ld).reshape(p.nelmt, nqt)
    g = np.empty((p.nelmt, len(COMPONENTS[dim]), nqt), dtype=ld)
    gabs = np.empty_like(g)
    for c, (a, b) in enumerate(COMPONENTS[dim]):
        g[:, c] = ww * sum(dd[:, k * dim + a] * dd[:, k * dim + b] for k in range(dim))
        gabs[:, c] = np.abs(ww) * sum(np.abs(dd[:, k * dim + a] * dd[:, k * dim + b]) for k in range(dim))
    g64 = torch_mod.tensor(g.astype(np.float64).reshape(-1), device="cuda")
    comp = p.run(sf, f=p.physderiv(sf))
    helm = (sf.helmholtz_hex if dim == 3 else sf.helmholtz_quad)(nq, *p.bs, *p.ds, g64, None, 0.0, p.x)
    torch_mod.cuda.synchronize()
    bases, derivs = [to_host(b) for b in p.bs], [to_host(d) for d in p.ds]
    _, habs = ref_helmholtz(nq, p.nelmt, bases, derivs, to_host(g64), None, 0.0, to_host(p.x))
    # the composition on absolute values is the Helmholtz operator on |B|, |D|, |x| with the metric of absolute values
    _, cabs = ref_helmholtz(nq, p.nelmt, bases, derivs, gabs.reshape(-1), None, 0.0, to_host(p.x))
    bound = gamma(physderiv_n(nq) + iprodderiv_n(nq) + 1, U64) * cabs + gamma(helm_n(nq), U64) * habs
    err = np.abs(to_host(comp).astype(ld) - to_host(helm).astype(ld))
    q = float(np.max(err / bound))
    print(f"composition {nq}: max |iprodderiv(physderiv) - helmholtz| / (sum of bounds) = {q:.3g}")
    assert q <= 1.0 and float(helm.abs().max()) > 0


@pytest.mark.parametrize("nq", [(8, 8, 8), (9, 9)], ids=case_id)
def test_physderiv_autograd(sf, torch_mod, nq):
    """.backward() of (out * f).sum() gives exactly iprodderiv_*(df, None, f); constants that require grad are refused."""
    p = Problem(sf, torch_mod, nq, 31, "float64", 71)
    for df in (p.df, None):
        x = p.x.clone().requires_grad_()
        out = sf.physderiv_autograd(nq, p.bs, p.ds, df, x)
        plain = p.physderiv(sf, df=df)
        torch_mod.cuda.synchronize()
        assert torch_mod.equal(out.detach(), plain)
        (out * p.f).sum().backward()
        want = p.run(sf, df=df, w=None)
        torch_mod.cuda.synchronize()
        assert x.grad is not None and x.grad.shape == x.shape
        assert torch_mod.equal(x.grad, want)
        assert float(want.abs().max()) > 0
    with pytest.raises(ValueError, match="constants"):
        sf.physderiv_autograd(nq, p.bs, p.ds, p.df.clone().requires_grad_(), p.x)
    with pytest.raises(ValueError, match="constants"):
        sf.physderiv_autograd(nq, [p.bs[0].clone().requires_grad_()] + p.bs[1:], p.ds, p.df, p.x)


@pytest.mark.parametrize("nq", [(7, 7, 7), (8, 8, 8), (9, 9), (4, 9)], ids=case_id)
def test_input_forms(sf, torch_mod, nq):
    """The (d, n) tensor physderiv_* returns (rows 256-byte aligned, the whole not contiguous for these odd n, taken
    without a copy), a sequence of d tensors and a contiguous (d n) tensor give bit-identical results."""
    p = Problem(sf, torch_mod, nq, 15, "float64", 81)
    grad = p.physderiv(sf)
    a = p.run(sf, f=grad)
    b = p.run(sf, f=[grad[i] for i in range(p.dim)])
    c = p.run(sf, f=tuple(grad[i].clone() for i in range(p.dim)))
    d = p.run(sf, f=grad.contiguous().reshape(-1))
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(a, b) and torch_mod.equal(a, c) and torch_mod.equal(a, d)
    p.check(a, "input forms", f=grad)


def test_larger_batch_hex8(sf, torch_mod):
    """20 011 elements at 3D nq = 8 against the fp64 reference (numpy matmuls); a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), 20011
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 8)
    y = p.run(sf)
    torch_mod.cuda.synchronize()
    ref, absref = iprodderiv_f64(nq, nelmt, [to_host(b) for b in p.bs], [to_host(d) for d in p.ds], to_host(p.df), to_host(p.w),
                                 [to_host(r) for r in p.f])
    worst = iprodderiv_excess(to_host(y), ref, absref, nq, U64)
    print(f"larger batch: max |err| / (gamma_{iprodderiv_n(nq)} absref) = {worst:.3g}")
    assert worst <= 1.0
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


def test_overlap_is_refused(sf, torch_mod):
    """`out` inside an in_a, inside df, inside w: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    keep_f, keep_df, keep_w = p.f.clone(), p.df.clone(), p.w.clone()
    m = nelmt * 343
    for out in [p.f[a][16:16 + m] for a in range(3)] + [p.df[512:512 + m], p.df[-m:], p.w[:m], p.w[-m:]]:
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, out=out)
        assert ei.value.rc == sf.capi.SF_EINVAL
    # without df / w their memory is no operand: an out there is fine
    got = p.run(sf, df=None, w=None, out=p.df[:m])
    torch_mod.cuda.synchronize()
    p.check(got, "out in the memory of an unused df", df=None, w=None)
    assert torch_mod.equal(p.f, keep_f) and torch_mod.equal(p.w, keep_w) and torch_mod.equal(p.df[m:], keep_df[m:])
