"""GPU tests of BwdTrans fused with the physical-space gradient (include/sumfact.h sf_physderiv_*), out_a = sum_b df_ab
D_b B x_e in one kernel, that are the family's own: scalar-aligned views, df never read when it is None, every plane of
df on its own, identity planes against df=None, consistency with sf_bwdtrans_*, an analytic gradient, a 131 075-element
batch and refused overlaps.  install() adds the family's cases of the parametrised tests the fused families share
(tests/fused_common.py: every wave order through AUTO, ragged counts, the fallback, explicit variants, guard bands);
refusals, stream capture and two streams in flight are tests/test_gpu_fused_common.py.

Reference and bound: tests/physderiv_ref.py.  Elementwise |gpu - ref| <= gamma_N * absref against a long-double
reference, gamma_N = N u / (1 - N u), N = sum nq_d + max nq_d + d, u = 2^-53 (fp64) or 2^-24 (fp32).
Data: seeded, per-value distinct (sf.fill_random); df uniform in (-1, 1), so every component and sign is exercised.
"""

import numpy as np
import pytest

from fused_common import install
from fused_families import BY_NAME, case_id, sf, sizes, to_host, torch_mod  # noqa: F401
from mass_ref import _forward_sweeps
from physderiv_ref import U64, analytic_case, physderiv_excess, physderiv_n, ref_physderiv, unit_roundoff

pytestmark = pytest.mark.gpu
install(globals(), BY_NAME["physderiv"])


class Problem:
    """Seeded data of one case, on the device."""

    def __init__(self, sf, torch_mod, nq, nelmt, dtype_name, seed):
        dtype = getattr(torch_mod, dtype_name)
        self.nq, self.nelmt, self.dtype_name, self.dim = tuple(nq), nelmt, dtype_name, len(nq)
        nmt, nqt = sizes(nq)
        self.bs = [sf.fill_random((q - 1) * q, 500 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.ds = [sf.fill_random(q * q, 600 + 7 * seed + d, dtype=dtype) for d, q in enumerate(nq)]
        self.df = sf.fill_random(nelmt * self.dim ** 2 * nqt, 8000 + seed, dtype=dtype)
        self.x = sf.fill_random(nelmt * nmt, 10 + seed, dtype=dtype)

    def run(self, sf, **kw):
        x = kw.pop("x", self.x)
        df = kw.pop("df", self.df)
        bs = kw.pop("bs", self.bs)
        ds = kw.pop("ds", self.ds)
        f = sf.physderiv_hex if self.dim == 3 else sf.physderiv_quad
        return f(self.nq, *bs, *ds, df, x, **kw)

    def excess(self, got, x=None, df="self", ds=None):
        x = self.x if x is None else x
        df = self.df if isinstance(df, str) else df
        ds = self.ds if ds is None else ds
        ref, absref = ref_physderiv(self.nq, self.nelmt, [to_host(b) for b in self.bs], [to_host(d) for d in ds], to_host(df), to_host(x))
        assert float(np.max(np.abs(ref))) > 0
        got = np.stack([to_host(g) for g in got]) if isinstance(got, (tuple, list)) else to_host(got)
        assert got.shape == ref.shape, (got.shape, ref.shape)
        return physderiv_excess(got, ref, absref, self.nq, unit_roundoff(self.dtype_name))

    def check(self, got, what, **kw):
        q = self.excess(got, **kw)
        print(f"{what}: {self.nq} {self.dtype_name} nelmt={self.nelmt}: max |err| / (gamma_N absref) = {q:.3g}")
        assert q <= 1.0, (what, self.nq, self.dtype_name, self.nelmt, q)


@pytest.mark.parametrize("nq", [(8, 8, 8), (7, 7, 7), (8, 8), (11, 11)], ids=case_id)
def test_scalar_aligned_views(sf, torch_mod, nq):
    """Scalar-aligned views of in, of one output and of df.  AUTO is correct through the fallback when in or any out_a
    lacks 16-byte alignment, and through the wave kernel when only df does; guards on both sides of every output are
    untouched; variant "wave" refuses in / out_a with SF_EALIGN."""
    nelmt, dim = 133, len(nq)
    nmt, nqt = sizes(nq)
    n = nelmt * nqt
    cases = (("float64", ((1, None, 0), (0, 0, 0), (0, dim - 1, 0), (0, None, 1), (1, 1, 3))),
             ("float32", ((2, None, 0), (0, 0, 0), (0, dim - 1, 0), (0, None, 3), (1, 1, 1))))
    for dtype_name, offsets in cases:
        dtype = getattr(torch_mod, dtype_name)
        one = 1 if dtype_name == "float64" else 2          # 8 bytes: scalar-aligned, not 16-byte aligned
        p = Problem(sf, torch_mod, nq, nelmt, dtype_name, 4)
        for off_in, odd_out, off_df in offsets:
            xbuf = sf.fill_random(nelmt * nmt + 8, 50 + off_in, dtype=dtype)
            x = xbuf[off_in:off_in + nelmt * nmt]
            dbuf = sf.fill_random(nelmt * dim * dim * nqt + 8, 60 + off_df, dtype=dtype)
            df = dbuf[off_df:off_df + nelmt * dim * dim * nqt]
            pad = 16
            stride = (n + 2 * pad + 3) // 4 * 4                 # every row of obuf starts 16-byte aligned
            obuf = torch_mod.full((dim, stride), 7.25, dtype=dtype, device="cuda")
            offs = [pad + (one if a == odd_out else 0) for a in range(dim)]
            outs = [obuf[a, offs[a]:offs[a] + n] for a in range(dim)]
            p.run(sf, x=x, df=df, out=outs)
            torch_mod.cuda.synchronize()
            p.check(outs, f"view {off_in}/{odd_out}/{off_df}", x=x, df=df)
            for a in range(dim):
                assert bool((obuf[a, :offs[a]] == 7.25).all()) and bool((obuf[a, offs[a] + n:] == 7.25).all())
            if dtype_name == "float64":
                if off_in or odd_out is not None:
                    with pytest.raises(sf.capi.SumfactError) as ei:
                        p.run(sf, x=x, df=df, out=outs, variant="wave")
                    assert ei.value.rc == sf.capi.SF_EALIGN
                    gen = p.run(sf, x=x, df=df, variant="generic")
                    torch_mod.cuda.synchronize()
                    assert all(torch_mod.equal(gen[a], outs[a]) for a in range(dim))      # AUTO took the fallback
                else:
                    wave = p.run(sf, x=x, df=df, variant="wave")
                    torch_mod.cuda.synchronize()
                    assert all(torch_mod.equal(wave[a], outs[a]) for a in range(dim))     # df needs scalar alignment only


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (12, 12), (6, 6, 12), (23, 5)], ids=case_id)
def test_df_is_never_read_when_none(sf, torch_mod, nq):
    """df=None with no df buffer in existence (the problem's own is freed first): the reference-space derivatives, on a
    wave shape and a fallback shape, in both precisions."""
    for dtype_name in ("float64", "float32"):
        p = Problem(sf, torch_mod, nq, 301, dtype_name, 21)
        p.df = None
        torch_mod.cuda.empty_cache()
        got = p.run(sf, df=None)
        torch_mod.cuda.synchronize()
        assert bool(torch_mod.isfinite(got).all())
        p.check(got, "df=None", df=None)


@pytest.mark.parametrize("nq", [(8, 8, 8), (5, 5, 5), (6, 4, 5), (12, 12), (7, 7), (4, 9)], ids=case_id)
def test_each_plane_alone(sf, torch_mod, nq):
    """One plane of df non-zero, the others zero: pins the component order c = a d + b (a transposed or permuted index
    would put the result into another output, or take another derivative)."""
    dim = len(nq)
    _, nqt = sizes(nq)
    p = Problem(sf, torch_mod, nq, 131, "float64", 41)
    for c in range(dim * dim):
        df = torch_mod.zeros_like(p.df).view(p.nelmt, dim * dim, nqt)
        df[:, c] = p.df.view(p.nelmt, dim * dim, nqt)[:, c]
        df = df.reshape(-1)
        got = p.run(sf, df=df)
        torch_mod.cuda.synchronize()
        p.check(got, f"plane {c}", df=df)
        for a in range(dim):
            assert (float(got[a].abs().max()) > 0) == (a == c // dim), (c, a)


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((7, 7), "float32"), ((6, 6, 12), "float64"),
                                           ((9, 9, 9), "float32"), ((12, 12), "float64")], ids=lambda v: case_id(v))
def test_identity_planes_equal_none(sf, torch_mod, nq, dtype_name):
    """Identity planes (1 on a == b, 0 elsewhere) give exactly the df=None result: 1 * x, then FMAs with exact zeros."""
    dim = len(nq)
    _, nqt = sizes(nq)
    p = Problem(sf, torch_mod, nq, 211, dtype_name, 51)
    ident = torch_mod.zeros_like(p.df).view(p.nelmt, dim, dim, nqt)
    for a in range(dim):
        ident[:, a, a] = 1.0
    got, none = p.run(sf, df=ident.reshape(-1)), p.run(sf, df=None)
    torch_mod.cuda.synchronize()
    assert np.array_equal(to_host(got), to_host(none))
    assert float(none.abs().max()) > 0


@pytest.mark.parametrize("nq,dtype_name", [((8, 8, 8), "float64"), ((5, 5, 5), "float32"), ((12, 12), "float64"),
                                           ((6, 6, 12), "float64"), ((4, 9), "float32")], ids=lambda v: case_id(v))
def test_identity_derivative_is_bwdtrans(sf, torch_mod, nq, dtype_name):
    """deriv_d = I and identity planes: every out_a is BwdTrans of the input, inside the bound of sf_bwdtrans_*'s own
    result (both within gamma_N absref of the long-double BwdTrans)."""
    dim = len(nq)
    _, nqt = sizes(nq)
    dtype = getattr(torch_mod, dtype_name)
    p = Problem(sf, torch_mod, nq, 257, dtype_name, 61)
    eye = [torch_mod.eye(q, dtype=dtype, device="cuda").reshape(-1) for q in nq]
    ident = torch_mod.zeros_like(p.df).view(p.nelmt, dim, dim, nqt)
    for a in range(dim):
        ident[:, a, a] = 1.0
    got = p.run(sf, ds=eye, df=ident.reshape(-1))
    bwd = (sf.bwdtrans_hex if dim == 3 else sf.bwdtrans_quad)(nq, *p.bs, p.x)
    torch_mod.cuda.synchronize()
    ld = np.longdouble
    ref = _forward_sweeps(nq, p.nelmt, [to_host(b).astype(ld) for b in p.bs], to_host(p.x), ld)
    absref = _forward_sweeps(nq, p.nelmt, [np.abs(to_host(b)).astype(ld) for b in p.bs], np.abs(to_host(p.x)), ld)
    u = unit_roundoff(dtype_name)
    qb = physderiv_excess(to_host(bwd), ref, absref, nq, u)
    assert qb <= 1.0
    for a in range(dim):
        q = physderiv_excess(to_host(got[a]), ref, absref, nq, u)
        print(f"bwdtrans consistency {nq} {dtype_name} out_{a}: {q:.3g} (sf_bwdtrans itself {qb:.3g})")
        assert q <= 1.0


@pytest.mark.parametrize("dim,nq", [(3, 8), (2, 12)], ids=["3d-nq8", "2d-nq12"])
def test_analytic_gradient(sf, torch_mod, dim, nq):
    """Legendre modal basis at the Gauss-Lobatto points on affine elements x = A_e xi + c: within 1.5 gamma_N absref of
    the analytic gradient of the polynomial (1 for the kernel, 0.5 granted to the reference in test_physderiv_cpu.py)."""
    nelmt, ext = 67, (nq,) * dim
    bases, derivs, df, x, exact = analytic_case(nq, dim, nelmt)
    t = lambda a: torch_mod.tensor(a, device="cuda")      # noqa: E731
    f = sf.physderiv_hex if dim == 3 else sf.physderiv_quad
    for variant in ("auto", "generic"):
        got = f(ext, *[t(b) for b in bases], *[t(d) for d in derivs], t(df), t(x), variant=variant)
        torch_mod.cuda.synchronize()
        _, absref = ref_physderiv(ext, nelmt, bases, derivs, df, x)
        q = physderiv_excess(to_host(got), exact, absref, ext, U64, factor=1.5)
        print(f"analytic {ext} {variant}: max |gpu - analytic| / (1.5 gamma_N absref) = {q:.3g}")
        assert q <= 1.0


def _sampled_excess(torch_mod, p, got, sample):
    """The excess of the elements `sample` of a large batch against the long-double reference of just those."""
    dim = p.dim
    nmt, nqt = sizes(p.nq)
    idx = torch_mod.tensor(sample, device="cuda")
    pick = lambda t, n: to_host(t.view(p.nelmt, n)[idx].reshape(-1))      # noqa: E731
    ref, absref = ref_physderiv(p.nq, len(sample), [to_host(b) for b in p.bs], [to_host(d) for d in p.ds],
                                pick(p.df, dim * dim * nqt), pick(p.x, nmt))
    sub = np.stack([pick(got[a], nqt) for a in range(dim)])
    return physderiv_excess(sub, ref, absref, p.nq, U64)


def test_large_batch_hex8(sf, torch_mod):
    """131 075 elements at 3D nq = 8 (an odd count above 2^17): a fixed seeded sample of elements against the long-double
    reference; a second run is bit-identical."""
    nq, nelmt = (8, 8, 8), (1 << 17) + 3
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 8)
    y = p.run(sf)
    torch_mod.cuda.synchronize()
    rng = np.random.default_rng(20240611)
    sample = np.unique(np.concatenate(([0, 1, 7, 8, nelmt - 9, nelmt - 8, nelmt - 1], rng.integers(0, nelmt, 1024))))
    worst = _sampled_excess(torch_mod, p, y, sample)
    print(f"large batch ({len(sample)} sampled elements): max |err| / (gamma_{physderiv_n(nq)} absref) = {worst:.3g}")
    assert worst <= 1.0
    again = p.run(sf)
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(y, again)


def test_overlap_is_refused(sf, torch_mod):
    """An output on `in`, inside df, or two outputs on the same memory: SF_EINVAL from the C ABI, nothing launched."""
    nq, nelmt = (8, 8, 8), 50
    n = nelmt * 512
    p = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    keep = p.x.clone()
    good = [torch_mod.zeros(n, dtype=torch_mod.float64, device="cuda") for _ in range(3)]
    big_in = sf.fill_random(n, 3)                                # an `in` long enough to hold an output
    for outs in ([good[0], good[0], good[2]], [good[0], good[1], p.df[512:512 + n]], [good[1], good[0], good[1]]):
        with pytest.raises(sf.capi.SumfactError) as ei:
            p.run(sf, out=outs)
        assert ei.value.rc == sf.capi.SF_EINVAL
    q = Problem(sf, torch_mod, nq, nelmt, "float64", 1)
    with pytest.raises(sf.capi.SumfactError) as ei:
        q.run(sf, out=[good[0], good[1], big_in], x=big_in[:nelmt * 343])
    assert ei.value.rc == sf.capi.SF_EINVAL
    torch_mod.cuda.synchronize()
    assert torch_mod.equal(p.x, keep)
